"""The ``wide`` switch off the GPU: ``skinny_gemm(wide=...)``'s state, the rows each kernel takes, ``wide_batch`` being inert
on a float32 CPU model, and the row-limit errors, which are raised before any prefill."""
import pytest
import torch

from batch_decode_common import PROMPTS, make_model
from scaling_amd.ops import gemm


@pytest.fixture(scope="module")
def model():
    return make_model("cpu", "float32")


def _state():
    return gemm.decode_rows_limit(), gemm.use_skinny(9), gemm.use_wide(17)


def test_wide_context_nests_and_restores():
    off, skinny, wide = (4, False, False), (16, True, False), (64, True, True)
    assert gemm.WIDE_MAX_ROWS == 64 and _state() == off
    with gemm.skinny_gemm(wide=True):
        assert _state() == wide
        with gemm.skinny_gemm():  # nested: skinny alone inside wide
            assert _state() == skinny
            with gemm.skinny_gemm(False, wide=True):  # off is off
                assert _state() == off
            with pytest.raises(KeyError):
                with gemm.skinny_gemm(True, wide=True):
                    assert _state() == wide
                    raise KeyError("x")
            assert _state() == skinny
        assert _state() == wide
    assert _state() == off


def test_rows_each_kernel_takes():
    rows = range(0, 71)
    assert not any(gemm.use_wide(r) or gemm.use_skinny(r) for r in rows)
    with gemm.skinny_gemm():
        assert not any(gemm.use_wide(r) for r in rows)
        assert [r for r in rows if gemm.use_skinny(r)] == list(range(gemm.SKINNY_MIN_ROWS, 17))
    with gemm.skinny_gemm(wide=True):
        assert [r for r in rows if gemm.use_wide(r)] == list(range(17, 65))
        assert [r for r in rows if gemm.use_skinny(r)] == list(range(gemm.SKINNY_MIN_ROWS, 17))


def test_wide_batch_is_inert_off_gpu(model):
    prompts = [PROMPTS[i % 6][: 1 + i % 5] for i in range(18)]
    want = model.generate_batch(3, input_tokens=prompts, stop_tokens=[])
    got = model.generate_batch(3, input_tokens=prompts, stop_tokens=[], wide_batch=True)
    for g, w in zip(got, want):
        assert g.completion_tokens == w.completion_tokens and torch.equal(g.completion_logits, w.completion_logits)
    assert _state() == (4, False, False)


def test_wide_limits_are_checked_first(model, monkeypatch):
    monkeypatch.setattr(model, "batch_decoder", lambda *a, **k: pytest.fail("prefill started"))
    monkeypatch.setattr(model, "forward", lambda *a, **k: pytest.fail("forward started"))
    with pytest.raises(ValueError, match="at most 64"):
        model.generate_batch(4, input_tokens=[[1, 2]] * 65, stop_tokens=[], use_cuda_graph=True, wide_batch=True)
    with pytest.raises(ValueError, match="at most 64"):
        model.generate_continuous(4, input_tokens=[[1, 2]] * 70, max_batch=65, page_size=32, stop_tokens=[],
                                  use_cuda_graph=True, wide_batch=True)
