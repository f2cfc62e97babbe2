"""The ``skinny_gemm`` switch off the GPU: the context manager's state, the row limits, the flag being inert on a float32
CPU model, and the argument errors, which are raised before any device work."""
import pytest
import torch

from batch_decode_common import PROMPTS, make_model
from scaling_amd.ops import gemm


@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


def test_context_restores_its_state():
    assert gemm.GEMV_MAX_ROWS == 4 and gemm.SKINNY_MAX_ROWS == 16 and 1 <= gemm.SKINNY_MIN_ROWS <= 16
    assert gemm.decode_rows_limit() == 4
    with gemm.skinny_gemm():
        assert gemm.decode_rows_limit() == 16
        with gemm.skinny_gemm(False):  # nested: off inside on
            assert gemm.decode_rows_limit() == 4
            with gemm.skinny_gemm(True):
                assert gemm.decode_rows_limit() == 16
            assert gemm.decode_rows_limit() == 4
        assert gemm.decode_rows_limit() == 16
    assert gemm.decode_rows_limit() == 4
    with pytest.raises(KeyError):
        with gemm.skinny_gemm():
            assert gemm.decode_rows_limit() == 16
            raise KeyError("x")
    assert gemm.decode_rows_limit() == 4
    with gemm.skinny_gemm(False):
        assert gemm.decode_rows_limit() == 4
        with pytest.raises(KeyError):
            with gemm.skinny_gemm(True):
                raise KeyError("x")
        assert gemm.decode_rows_limit() == 4
    assert gemm.decode_rows_limit() == 4


def test_rows_that_take_the_mfma_kernel():
    assert not any(gemm.use_skinny(r) for r in range(0, 20))
    with gemm.skinny_gemm():
        took = [r for r in range(0, 20) if gemm.use_skinny(r)]
    assert took == list(range(gemm.SKINNY_MIN_ROWS, 17))


def test_flag_is_inert_off_gpu(model):
    prompts = PROMPTS[:5]
    want = model.generate_batch(6, input_tokens=prompts, stop_tokens=[])
    got = model.generate_batch(6, input_tokens=prompts, stop_tokens=[], skinny_gemm=True)
    for g, w in zip(got, want):
        assert g.completion_tokens == w.completion_tokens
        assert torch.equal(g.completion_logits, w.completion_logits)
    assert gemm.decode_rows_limit() == 4


def test_graph_limits_are_checked_first(model, monkeypatch):
    """Both errors are raised before the prompts are prefilled (no device work)."""
    monkeypatch.setattr(model, "batch_decoder", lambda *a, **k: pytest.fail("prefill started"))
    monkeypatch.setattr(model, "forward", lambda *a, **k: pytest.fail("forward started"))
    with pytest.raises(ValueError, match="at most 16"):
        model.generate_batch(4, input_tokens=[[1, 2]] * 17, stop_tokens=[], use_cuda_graph=True, skinny_gemm=True)
    with pytest.raises(ValueError, match="at most 4"):
        model.generate_batch(4, input_tokens=[[1, 2]] * 5, stop_tokens=[], use_cuda_graph=True)
