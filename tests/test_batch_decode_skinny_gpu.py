"""Batched generation on the MFMA weight-streaming kernels (``generate_batch(..., skinny_gemm=True)``, up to 16 rows under
one HIP graph): graph versus eager, batched versus single-sequence logits (teacher-forced), the kernels taken, the row
limits (GPU only).  The model and the first six prompts are those of ``tests/batch_decode_common.py``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import MAX_TOKENS, PROMPTS, make_model  # noqa: E402
from scaling_amd.ops import gemm  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

LAYERS = 2
# ten more fixed prompts, lengths between 1 and 40 (with max_tokens = 36 the longest row ends at key 76 of 128)
MORE_LENGTHS = [1, 40, 3, 26, 15, 8, 31, 2, 19, 36]
PROMPTS16 = PROMPTS + [[(37 * i + 11 * j * j + 7 * j + 5) % 251 + 1 for j in range(n)] for i, n in enumerate(MORE_LENGTHS)]
assert len(PROMPTS16) == 16 and all(1 <= len(p) <= 40 and all(0 < t < 256 for t in p) for p in PROMPTS16)


@pytest.fixture(scope="module")
def model():
    return make_model(0, "bfloat16")


@pytest.fixture(scope="module")
def qmodel():
    m = make_model(0, "bfloat16")
    info = m.quantize_weights()
    assert info["tensors"] == 7 * LAYERS and info["skipped"] == {}
    return m


@pytest.fixture(scope="module")
def hmodel():
    return make_model(0, "float16")


def _sampler(sampled):
    from scaling_amd.transformer.inference import Sampler

    return {"sample_fn": Sampler(0.8, 40, 0.95, seed=1)} if sampled else {}


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.completion_tokens == y.completion_tokens, (x.completion_tokens, y.completion_tokens)
        torch.testing.assert_close(x.completion_logits.float().cpu(), y.completion_logits.float().cpu(),
                                   rtol=1e-2, atol=1e-2)


def _bitwise(a, b):
    for x, y in zip(a, b):
        assert x.completion_tokens == y.completion_tokens and torch.equal(x.completion_logits, y.completion_logits)


def _graph_equals_eager(m, B, sampled, stops=True):
    kw = dict(_sampler(sampled), skinny_gemm=True)
    prompts = PROMPTS16[:B]
    eager = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=[], **kw)
    graph = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=[], use_cuda_graph=True, **kw)
    assert all(len(o.completion_tokens) == MAX_TOKENS for o in eager)
    _assert_same(graph, eager)
    _bitwise(m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=[], use_cuda_graph=True, **kw), graph)
    assert gemm.decode_rows_limit() == 4  # the switch does not outlive the call
    if not stops:
        return
    # per-row stop tokens: one taken from each row's own text, at a different step per row
    stops = [o.completion_tokens[2 + 2 * b] for b, o in enumerate(eager)]
    eager_s = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=stops, **kw)
    graph_s = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=stops, use_cuda_graph=True, **kw)
    _assert_same(graph_s, eager_s)
    for o, full in zip(eager_s, eager):
        n = len(o.completion_tokens)
        assert o.completion_tokens == full.completion_tokens[:n] and n <= 2 + 2 * (B - 1) + 1
        assert o.completion_tokens[-1] in stops and not any(t in stops for t in o.completion_tokens[:-1])
        assert o.completion_logits.shape[0] == n
    _bitwise(m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=stops, use_cuda_graph=True, **kw), graph_s)


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B", [5, 9, 16])
def test_skinny_graph_equals_eager(model, B, sampled):
    _graph_equals_eager(model, B, sampled)


def test_skinny_graph_equals_eager_fp8(qmodel):
    _graph_equals_eager(qmodel, 7, False)
    _graph_equals_eager(qmodel, 7, True)


def test_skinny_graph_equals_eager_fp16(hmodel):
    _graph_equals_eager(hmodel, 5, False)


@pytest.mark.parametrize("B", sorted({gemm.SKINNY_MIN_ROWS, max(gemm.SKINNY_MIN_ROWS, 4)}))
def test_skinny_graph_equals_eager_at_the_smallest_batches(model, B):
    _graph_equals_eager(model, B, False, stops=False)


@pytest.fixture(scope="module")
def singles(model):
    """Eager single-sequence greedy generation of every prompt (GEMV kernels), computed once."""
    return [model.generate(MAX_TOKENS, input_tokens=p, stop_tokens=[], use_cache=True) for p in PROMPTS16]


def test_skinny_batched_follows_single_teacher_forced(model, singles):
    """B = 16 under the graph: every row is fed the tokens of its own single-sequence greedy generation; its logits
    follow the single-sequence logits, step 0 bitwise (the same prefill), every later step of every row within 5e-2
    (the bound of ``test_batched_follows_single_teacher_forced``)."""
    B = 16
    assert all(len(s.completion_tokens) == MAX_TOKENS for s in singles)
    dec = model.batch_decoder(MAX_TOKENS, PROMPTS16, skinny_gemm=True)
    dec.capture()
    for b, s in enumerate(singles):
        assert torch.equal(dec.logits[0, b], s.completion_logits[0])
        assert int(dec.tokens[0, b]) == s.completion_tokens[0]
    for k in range(1, MAX_TOKENS):
        dec.tok.copy_(torch.tensor([[s.completion_tokens[k - 1]] for s in singles], device=dec.tok.device))
        dec.step()
    dec.state.check()
    got = dec.logits[:MAX_TOKENS].float()  # [steps, B, V]
    ref = torch.stack([s.completion_logits.float() for s in singles], dim=1)
    assert got.shape == ref.shape == (MAX_TOKENS, B, 256)
    diff = (got - ref).abs().amax(dim=2)
    print("B=16 graph, skinny: max |logit difference| per step (over rows):",
          [round(float(d), 4) for d in diff.amax(dim=1)])
    print("per row (over steps):", [round(float(d), 4) for d in diff.amax(dim=0)])
    torch.testing.assert_close(got, ref, rtol=5e-2, atol=5e-2)  # every step of every row, none left out


GEMV = ("gemv", "gemv_residual", "gemv_swiglu", "gemv_norm", "gemv_norm_rope",
        "gemv_w8", "gemv_w8_residual", "gemv_w8_swiglu", "gemv_w8_norm")
SKINNY = ("skinny", "skinny_residual", "skinny_swiglu", "skinny_norm",
          "skinny_w8", "skinny_w8_residual", "skinny_w8_swiglu", "skinny_w8_norm")


def _count(monkeypatch, names):
    calls: dict = {}
    mod = ext()
    for name in names:
        fn = getattr(mod, name)

        def wrapped(*a, _fn=fn, _name=name, **k):
            out = _fn(*a, **k)
            calls[_name] = calls.get(_name, 0) + (out is not None)
            return out

        monkeypatch.setattr(mod, name, wrapped)
    return calls


@pytest.mark.parametrize("fp8", [False, True])
def test_skinny_step_takes_mfma_kernels(model, qmodel, monkeypatch, fp8):
    """B = 9, counted over the decode steps alone (warm-up, capture; the prefills run before the counters exist): per
    layer and step skinny_norm twice (norm + q/k/v, add + norm + gate/up + SwiGLU), skinny_residual once (down +
    residual), the batched RoPE + K/V append once, and no GEMV at all."""
    m = qmodel if fp8 else model
    dec = m.batch_decoder(4, PROMPTS16[:9], skinny_gemm=True)
    calls = _count(monkeypatch, ("rope_kv_append_batch", "rope_kv_append") + GEMV + SKINNY)
    dec.capture()
    steps = 2  # warm-up + capture
    dec.step()
    p = "skinny_w8" if fp8 else "skinny"
    assert calls.get(p + "_norm", 0) >= 2 * LAYERS * steps and calls.get(p + "_residual", 0) >= LAYERS * steps, calls
    assert calls.get(p, 0) >= LAYERS * steps, calls  # the o-projection
    assert calls.get("rope_kv_append_batch", 0) == LAYERS * steps and calls.get("rope_kv_append", 0) == 0, calls
    assert all(calls.get(k, 0) == 0 for k in GEMV), calls
    if fp8:  # no dense MFMA kernel inside the layers (ext().skinny serves the tied, never-quantised head)
        assert all(calls.get(k, 0) == 0 for k in ("skinny_norm", "skinny_residual", "skinny_swiglu")), calls
        assert calls.get("skinny", 0) == steps, calls


def test_skinny_graph_limits(model):
    with pytest.raises(ValueError, match="at most 16"):
        model.generate_batch(4, input_tokens=PROMPTS16 + [[5, 6]], stop_tokens=[], use_cuda_graph=True, skinny_gemm=True)
    with pytest.raises(ValueError, match="at most 4"):
        model.generate_batch(4, input_tokens=PROMPTS16[:5], stop_tokens=[], use_cuda_graph=True)
    # eager with the flag above 16 rows: the library path, as without the flag
    outs = model.generate_batch(3, input_tokens=PROMPTS16 + [[5, 6]], stop_tokens=[], skinny_gemm=True)
    want = model.generate_batch(3, input_tokens=PROMPTS16 + [[5, 6]], stop_tokens=[])
    _bitwise(outs, want)
