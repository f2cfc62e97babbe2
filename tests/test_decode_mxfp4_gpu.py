"""MXFP4 weight-only decoding end to end (``TransformerInferenceModule.quantize_weights("mxfp4")``) on the small
Llama-layout model of ``tests/test_decode_fp8_gpu.py`` (hidden 256): graph decoding equals eager decoding (single and
batched, with the skinny kernel, the FP8 KV cache and pages), the ``_w4`` kernels are the ones taken, the logits follow a
never-quantised twin that carries the dequantised weights, and a modified weight falls back to bf16."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import quant  # noqa: E402
from tests.test_decode_fp8_gpu import BF16, LAYERS, PROMPT, W8, _count, _model, _teacher_forced  # noqa: E402

W4 = ("gemv_w4", "gemv_w4_residual", "gemv_w4_swiglu", "gemv_w4_norm")
SK4 = ("skinny_w4", "skinny_w4_residual", "skinny_w4_swiglu", "skinny_w4_norm")
SK = ("skinny", "skinny_residual", "skinny_swiglu", "skinny_norm",
      "skinny_w8", "skinny_w8_residual", "skinny_w8_swiglu", "skinny_w8_norm")
PROMPTS = [[3, 17, 42, 99, 5, 7, 11], [8, 1, 200, 31], [77, 78, 79, 80, 81, 82, 83, 84, 85], [5, 250],
           [9, 19, 29, 39, 49, 59]]


def _twin_of(m, **kw):
    """A never-quantised module carrying m's (dequantised) weights."""
    t = _model(**kw)
    with torch.no_grad():
        for (n, p), (n2, p2) in zip(m.named_parameters(), t.named_parameters()):
            assert n == n2
            p2.copy_(p)
    assert not any(quant.has_copy(p) for p in t.parameters())
    return t


@pytest.fixture(scope="module")
def pair():
    """(quantised model, never-quantised twin on the dequantised weights, the twin's greedy tokens)."""
    m = _model()
    info = m.quantize_weights("mxfp4")
    assert info["tensors"] == 7 * LAYERS and info["skipped"] == {} and info["fp8_bytes"] == 0
    assert info["quantized_bytes"] * 64 == info["bf16_bytes"] * 17
    t = _twin_of(m)
    greedy = t.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True).completion_tokens
    return m, t, greedy


def test_mxfp4_graph_decode_matches_eager(pair):
    from scaling_amd.transformer.inference import Sampler

    m = pair[0]
    for kw in ({}, {"sample_fn": Sampler(0.8, 40, 0.95, seed=1)}):
        eager = m.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True, **kw)
        graph = m.generate(20, input_tokens=PROMPT, stop_tokens=[], use_cache=True, use_cuda_graph=True, **kw)
        assert len(eager.completion_tokens) == 20
        assert graph.completion_tokens == eager.completion_tokens, (graph.completion_tokens, eager.completion_tokens)
        torch.testing.assert_close(graph.completion_logits.float().cpu(), eager.completion_logits.float().cpu(),
                                   rtol=1e-2, atol=1e-2)
    assert all(quant.w4_of(p) is not None for p in m.parameters() if hasattr(p, "_sa_w4"))


@pytest.mark.parametrize("B,skinny", [(2, False), (5, True)])
def test_mxfp4_batched_graph_matches_eager(pair, monkeypatch, B, skinny):
    m = pair[0]
    kw = {"skinny_gemm": True} if skinny else {}
    calls = _count(monkeypatch, W4 + SK4 + SK + W8 + BF16)
    eager = m.generate_batch(8, input_tokens=PROMPTS[:B], stop_tokens=[], **kw)
    taken = dict(calls)
    graph = m.generate_batch(8, input_tokens=PROMPTS[:B], stop_tokens=[], use_cuda_graph=True, **kw)
    assert [g.completion_tokens for g in graph] == [e.completion_tokens for e in eager]
    assert all(len(e.completion_tokens) == 8 for e in eager)
    mine = SK4 if skinny else W4
    assert taken.get(mine[3], 0) > 0 and taken.get(mine[1], 0) > 0 and taken.get(mine[0], 0) > 0, taken
    # no dense or FP8 kernel in the quantised layers (gemv / skinny still serve the tied, never-quantised head)
    assert all(taken.get(k, 0) == 0 for k in W8 + SK[1:4] + SK[4:] + BF16[1:]), taken


def test_mxfp4_with_fp8_kv_cache_and_pages(pair):
    m = pair[0]
    kw = dict(kv_cache="fp8_e4m3", page_size=32, skinny_gemm=True)
    eager = m.generate_batch(8, input_tokens=PROMPTS[:3], stop_tokens=[], **kw)
    graph = m.generate_batch(8, input_tokens=PROMPTS[:3], stop_tokens=[], use_cuda_graph=True, **kw)
    assert [g.completion_tokens for g in graph] == [e.completion_tokens for e in eager]
    cont = m.generate_continuous(6, input_tokens=PROMPTS, max_batch=3, page_size=32, skinny_gemm=True,
                                 kv_cache="fp8_e4m3", stop_tokens=[])
    assert len(cont) == len(PROMPTS) and all(len(c.completion_tokens) == 6 for c in cont)


@pytest.mark.parametrize("graph", [False, True])
def test_mxfp4_kernels_are_taken(pair, monkeypatch, graph):
    """Per layer and decode step: q/k/v and gate/up through gemv_w4_norm, the attention output projection through
    gemv_w4, down + residual through gemv_w4_residual; no bf16 or FP8 GEMV in the quantised layers."""
    m = pair[0]
    steps = 4
    calls = _count(monkeypatch, W4 + W8 + BF16)
    m.generate(steps + 1, input_tokens=PROMPT, stop_tokens=[], use_cache=True, use_cuda_graph=graph)
    n = LAYERS * (1 if graph else steps)
    assert calls.get("gemv_w4_norm", 0) >= 2 * n and calls.get("gemv_w4_residual", 0) >= n, calls
    assert calls.get("gemv_w4", 0) >= n, calls
    assert all(calls.get(k, 0) == 0 for k in ("gemv_norm", "gemv_residual", "gemv_swiglu", "gemv_norm_rope") + W8), calls


def test_mxfp4_lm_head_is_counted(monkeypatch):
    m = _model(weight_tying=False)
    info = m.quantize_weights("mxfp4", include_lm_head=True)
    assert info["tensors"] == 7 * LAYERS + 1
    calls = _count(monkeypatch, W4 + W8 + BF16)
    steps = 3
    m.generate(steps + 1, input_tokens=PROMPT, stop_tokens=[], use_cache=True)
    assert calls.get("gemv_w4", 0) >= (LAYERS + 1) * steps, calls  # o-projection per layer + the head
    assert all(calls.get(k, 0) == 0 for k in BF16 + W8), calls


def test_mxfp4_teacher_forced_logits_follow_the_twin(pair):
    m, t, greedy = pair
    pa, sa = _teacher_forced(m, greedy)
    pb, sb = _teacher_forced(t, greedy)
    assert torch.equal(pa, pb)  # the prefill: same code, same weights
    assert sa.shape == sb.shape == (len(greedy), 256)
    diff = (sa.float() - sb.float()).abs().amax(dim=1)
    print("max |logit difference| per decode step:", [round(float(d), 4) for d in diff])
    torch.testing.assert_close(sa.float(), sb.float(), rtol=5e-2, atol=5e-2)  # every step, none left out


def test_mxfp4_stale_weight_falls_back(monkeypatch):
    m = _model()
    m.quantize_weights("mxfp4")
    w = m._layers[1].mlp.dense_out.weight
    with torch.no_grad():
        w.mul_(0.5)
    t = _twin_of(m)
    ref = t.generate(12, input_tokens=PROMPT, stop_tokens=[], use_cache=True)
    calls = _count(monkeypatch, W4 + W8 + BF16)
    quant._warned[0] = False
    with pytest.warns(RuntimeWarning, match="MXFP4 copy"):
        out = m.generate(12, input_tokens=PROMPT, stop_tokens=[], use_cache=True)
    assert not hasattr(w, "_sa_w4")
    # layer 1's down projection runs the bf16 kernel, the other layer's the MXFP4 one
    assert calls.get("gemv_residual", 0) == 11 and calls.get("gemv_w4_residual", 0) == 11 * (LAYERS - 1), calls
    tf_m, tf_t = _teacher_forced(m, ref.completion_tokens), _teacher_forced(t, ref.completion_tokens)
    assert torch.equal(tf_m[0], tf_t[0])
    torch.testing.assert_close(tf_m[1].float(), tf_t[1].float(), rtol=5e-2, atol=5e-2)
    assert len(out.completion_tokens) == 12
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m.generate(3, input_tokens=PROMPT, stop_tokens=[], use_cache=True)


def test_mxfp4_logit_drift_is_reported(pair):
    """Informational (no threshold): relative RMS difference of the logits between the original bf16 model and its
    quantised self."""
    orig = _model()
    a = orig.logits(input_tokens=PROMPT).float()
    b = pair[0].logits(input_tokens=PROMPT).float()
    rel = float((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt())
    print(f"relative RMS logit difference bf16 vs mxfp4: {rel:.4f}")
    assert rel == rel and rel > 0 and rel != float("inf")
