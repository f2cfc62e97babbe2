"""Batched generation on the wide MFMA kernels (``generate_batch(..., wide_batch=True)``, up to 64 rows under one HIP
graph): graph versus eager, quantised weights, the FP8 KV cache, continuous batching over pages, batched versus
single-sequence logits (teacher-forced), the kernels taken, the row limit (GPU only).  The model is that of
``tests/batch_decode_common.py``; the 64 prompts cycle through its ``PROMPTS`` at lengths 1..33."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import PROMPTS, make_model  # noqa: E402
from scaling_amd.ops import gemm  # noqa: E402
from test_batch_decode_skinny_gpu import GEMV, LAYERS, SKINNY, _assert_same, _count, _sampler  # noqa: E402
from test_paged_decode_gpu import _bitwise, _static  # noqa: E402

TOKENS = 12
# prompt i: PROMPTS[i % 6] shifted by 3 i, cut to 1 + 7 i mod its length (2 and 20 whole: 33 tokens, two pages of 32)
PROMPTS64 = [[(t + 3 * i) % 255 + 1 for t in PROMPTS[i % 6]][: 33 if i in (2, 20) else 1 + (7 * i) % len(PROMPTS[i % 6])]
             for i in range(64)]
assert len({len(p) for p in PROMPTS64}) > 10 and len(PROMPTS64[2]) == len(PROMPTS64[20]) == 33
WIDE = tuple(n.replace("skinny", "wide") for n in SKINNY)


@pytest.fixture(scope="module")
def model():
    return make_model(0, "bfloat16")


def _graph_equals_eager(m, B, **kw):
    kw = dict(kw, wide_batch=True, input_tokens=PROMPTS64[:B], stop_tokens=[])
    eager = m.generate_batch(TOKENS, **kw)
    graph = m.generate_batch(TOKENS, use_cuda_graph=True, **kw)
    assert all(len(o.completion_tokens) == TOKENS for o in eager)
    _assert_same(graph, eager)
    assert gemm.decode_rows_limit() == 4 and not gemm.use_wide(17)  # the switch does not outlive the call


@pytest.mark.parametrize("B", [17, 33, 64])
def test_wide_graph_equals_eager(model, B):
    _graph_equals_eager(model, B)


@pytest.mark.parametrize("case", ["sampled", "fp8_e4m3", "mxfp4", "kv_fp8"])
def test_wide_graph_equals_eager_variants(model, case):
    if case in ("fp8_e4m3", "mxfp4"):
        model = make_model(0, "bfloat16")
        assert model.quantize_weights(case)["skipped"] == {}
    kw = _sampler(True) if case == "sampled" else {"kv_cache": "fp8_e4m3"} if case == "kv_fp8" else {}
    _graph_equals_eager(model, 24, **kw)


def test_wide_continuous_equals_static_row_for_row(model):
    """40 requests through 24 rows over 32-token pages under one graph: each is bitwise the same request in a static
    paged batch of 24 (the same kernels, whose rows do not depend on each other, and the same two-page split plan)."""
    reqs = (PROMPTS64[:40], [3 + (7 * i) % 18 for i in range(40)])
    out = model.generate_continuous(reqs[1], input_tokens=reqs[0], max_batch=24, page_size=32, stop_tokens=[],
                                    use_cuda_graph=True, wide_batch=True)
    for lo in (0, 16):  # requests 0..23 and 16..39
        _, ref = _static(model, reqs[0][lo: lo + 24], 20, True, wide_batch=True, page_size=32)
        got = [(o.completion_tokens, o.completion_logits) for o in out[lo: lo + 24]]
        assert [len(t) for t, _ in got] == reqs[1][lo: lo + 24]
        _bitwise(got, [(t[: len(g[0])], lg[: len(g[0])]) for (t, lg), g in zip(ref, got)], f"continuous vs static {lo}")


def test_wide_batched_follows_single_teacher_forced(model):
    """B = 64 under the graph, each row fed its own single-sequence greedy tokens: logits within the 16-row test's 5e-2."""
    singles = [model.generate(TOKENS, input_tokens=p, stop_tokens=[], use_cache=True) for p in PROMPTS64]
    dec = model.batch_decoder(TOKENS, PROMPTS64, wide_batch=True)
    dec.capture()
    ref = torch.stack([s.completion_logits.float() for s in singles], dim=1)  # [steps, B, V]
    assert torch.equal(dec.logits[0].float(), ref[0])
    for k in range(1, TOKENS):
        dec.tok.copy_(torch.tensor([[s.completion_tokens[k - 1]] for s in singles], device=dec.tok.device))
        dec.step()
    dec.state.check()
    got = dec.logits[:TOKENS].float()
    print("B=64 graph, wide: max |logit difference| per step:", [round(float(d), 4) for d in (got - ref).abs().amax(dim=(1, 2))])
    torch.testing.assert_close(got, ref, rtol=5e-2, atol=5e-2)


@pytest.mark.parametrize("scheme", [None, "fp8_e4m3", "mxfp4"])
def test_wide_step_takes_wide_kernels(model, monkeypatch, scheme):
    """B = 33, warm-up + capture: per layer wide_norm twice, wide_residual once, the o-projection; no GEMV, no skinny."""
    p = "wide"
    if scheme is not None:
        model, p = make_model(0, "bfloat16"), "wide_w8" if scheme == "fp8_e4m3" else "wide_w4"
        model.quantize_weights(scheme)
    w4 = tuple(n.replace("w8", "w4") for n in WIDE + SKINNY + GEMV if "w8" in n)
    dec = model.batch_decoder(4, PROMPTS64[:33], wide_batch=True)
    calls = _count(monkeypatch, ("rope_kv_append_batch",) + GEMV + SKINNY + WIDE + w4)
    dec.capture()
    dec.step()
    steps = 2  # warm-up + capture
    assert calls.get(p + "_norm", 0) == 2 * LAYERS * steps and calls.get(p + "_residual", 0) == LAYERS * steps, calls
    assert calls.get(p, 0) >= LAYERS * steps and calls.get("rope_kv_append_batch", 0) == LAYERS * steps, calls
    assert all(v == 0 for k, v in calls.items() if not k.startswith(("wide", "rope"))), calls
    if scheme is not None:  # (ext().wide serves the tied, never-quantised head alone)
        assert calls.get("wide", 0) == steps and calls.get("wide_norm", 0) == 0, calls


def test_wide_graph_limit(model):
    with pytest.raises(ValueError, match="at most 64"):
        model.generate_batch(4, input_tokens=PROMPTS64 + [[5, 6]], stop_tokens=[], use_cuda_graph=True, wide_batch=True)
    with pytest.raises(ValueError, match="at most 64"):
        model.continuous_decoder(65, page_size=32, use_cuda_graph=True, wide_batch=True)
