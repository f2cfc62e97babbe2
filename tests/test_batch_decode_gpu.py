"""Batched generation on the GPU (``generate_batch`` / ``BatchDecoder``): the batched RoPE + K/V append kernel and
flash-decoding over key ranges against the existing one-sequence kernels (bit for bit), graph versus eager, batched
versus single-sequence logits (teacher-forced), the fused kernels taken, and FP8 weights."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import MAX_TOKENS, PROMPTS, make_model  # noqa: E402
from scaling_amd.ops import attention  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

DEV = "cuda"
LAYERS = 2


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
def singles(model):
    """Eager single-sequence greedy generation of every prompt, computed once."""
    return [model.generate(MAX_TOKENS, input_tokens=p, stop_tokens=[], use_cache=True) for p in PROMPTS]


# ---------------------------------------------------------------------------------------------- kernels
def _rope_tables(rows, rd):
    half = rd // 2
    inv = 1.0 / (10000 ** (torch.arange(0, half, device=DEV, dtype=torch.float32) / half))
    ang = torch.arange(rows, device=DEV, dtype=torch.float32)[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _append_case(B, positions, rd, interleaved, dtype):
    """(q, K, V, err) of the batched kernel and of B one-token calls on the slab views, plus the untouched caches."""
    nq, nkv, hd, cap = 4, 2, 64, 48
    cos, sin = _rope_tables(64, rd)
    g = torch.Generator(device=DEV).manual_seed(3 + B)
    qkv = torch.randn(B, nq + 2 * nkv, hd, device=DEV, dtype=dtype, generator=g)
    k0 = torch.randn(B * cap, nkv, hd, device=DEV, dtype=dtype, generator=g)
    v0 = torch.randn(B * cap, nkv, hd, device=DEV, dtype=dtype, generator=g)
    pos = torch.tensor(positions, device=DEV, dtype=torch.long)
    kc, vc, kr, vr = k0.clone(), v0.clone(), k0.clone(), v0.clone()
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    q = ext().rope_kv_append_batch(qkv, cos, sin, pos, nq, nkv, rd, interleaved, kc, vc, err, cap)
    assert q is not None and tuple(q.shape) == (B, nq, hd)
    q_ref, errs = [], []
    for b in range(B):
        e = torch.zeros(1, device=DEV, dtype=torch.int32)
        qb = ext().rope_kv_append(qkv[b : b + 1], cos, sin, pos[b : b + 1], nq, nkv, rd, interleaved,
                                  kr[b * cap : (b + 1) * cap], vr[b * cap : (b + 1) * cap], e)
        assert qb is not None
        q_ref.append(qb)
        errs.append(int(e.item()))
    return q, kc, vc, int(err.item()), torch.cat(q_ref), kr, vr, errs, k0, v0, cap


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("rd", [64, 32])
def test_batched_rope_append_bit_identical(rd, interleaved, dtype):
    for B in (1, 2, 3, 5):
        positions = [0, 29, 47, 7, 31][:B]
        q, kc, vc, err, q_ref, kr, vr, errs, k0, v0, cap = _append_case(B, positions, rd, interleaved, dtype)
        assert err == 0 and errs == [0] * B
        assert torch.equal(q, q_ref) and torch.equal(kc, kr) and torch.equal(vc, vr)
        written = torch.zeros(B * cap, dtype=torch.bool, device=DEV)
        written[[b * cap + p for b, p in enumerate(positions)]] = True
        assert torch.equal(kc[~written], k0[~written]) and torch.equal(vc[~written], v0[~written])
        assert not torch.equal(kc[written], k0[written]) and not torch.equal(vc[written], v0[written])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("interleaved", [False, True])
def test_batched_rope_append_out_of_range_rows(interleaved, dtype):
    """Rows at pos = cap and pos = -1: the error word is set, their slabs are untouched and their q rows zero; the
    other rows are unaffected."""
    positions = [0, 48, 47, -1, 31]
    q, kc, vc, err, q_ref, kr, vr, errs, k0, v0, cap = _append_case(5, positions, 64, interleaved, dtype)
    assert err == 1 and errs == [0, 1, 0, 1, 0]
    for b in (1, 3):
        assert not q[b].any()
        assert torch.equal(kc[b * cap : (b + 1) * cap], k0[b * cap : (b + 1) * cap])
        assert torch.equal(vc[b * cap : (b + 1) * cap], v0[b * cap : (b + 1) * cap])
    assert torch.equal(q, q_ref) and torch.equal(kc, kr) and torch.equal(vc, vr)
    assert q[0].any() and q[2].any() and q[4].any()


RANGES = [(0, 1), (100, 32), (50, 0), (200, 33), (300, 65)]  # per-sequence capacity 100; one empty segment


@pytest.mark.parametrize("D,dtype,Lq", [(64, torch.bfloat16, 1), (128, torch.bfloat16, 1), (64, torch.float16, 1),
                                        (128, torch.float16, 1), (64, torch.bfloat16, 2)])
def test_flash_decode_over_key_ranges(D, dtype, Lq):
    Hq, Hk, cap = 4, 2, 100
    nseg = len(RANGES)
    g = torch.Generator(device=DEV).manual_seed(0)
    k = torch.full((4 * cap, Hk, D), float("nan"), device=DEV, dtype=dtype)
    v = torch.full((4 * cap, Hk, D), float("nan"), device=DEV, dtype=dtype)
    for s0, n in RANGES:
        k[s0 : s0 + n] = torch.randn(n, Hk, D, device=DEV, dtype=dtype, generator=g)
        v[s0 : s0 + n] = torch.randn(n, Hk, D, device=DEV, dtype=dtype, generator=g)
    q = torch.randn(nseg * Lq, Hq, D, device=DEV, dtype=dtype, generator=g)
    cu_q = torch.arange(0, (nseg + 1) * Lq, Lq, device=DEV, dtype=torch.int32)
    kr = torch.tensor(RANGES, device=DEV, dtype=torch.int32)
    kc = torch.cat([k[s0 : s0 + n] for s0, n in RANGES])
    vc = torch.cat([v[s0 : s0 + n] for s0, n in RANGES])
    cu_k = torch.tensor([0] + [n for _, n in RANGES], device=DEV).cumsum(0).to(torch.int32)
    scale = 1 / math.sqrt(D)
    with torch.no_grad():
        o = attention.flash_attention(q, k, v, cu_q, None, Lq, cap, scale, True, key_ranges=kr)
        o2, _ = ext().fa_fwd(q, k, v, cu_q, cu_q, Lq, scale, True, -1, 0.0, 0, -1, cap, kr)
        packed, _ = ext().fa_fwd(q, kc, vc, cu_q, cu_k, Lq, scale, True, -1, 0.0, 0, -1, cap)
    assert torch.isfinite(o).all()
    # the split plan depends only on max_k, Hkv and nseg, so the ranged call walks the same tiles as the packed one
    assert torch.equal(o, packed) and torch.equal(o2, packed)
    ref = attention.attention_reference(q.float(), k.float(), v.float(), cu_q, None, scale, True, key_ranges=kr)
    torch.testing.assert_close(o.float(), ref, atol=2e-2, rtol=2e-2)


def test_key_ranges_need_the_decode_kernel():
    Hq, Hk, D, Lq = 4, 2, 64, 17  # 17 queries x 2 q heads per kv head = 34 packed rows > 32: the prefill kernel
    q = torch.randn(Lq, Hq, D, device=DEV, dtype=torch.bfloat16)
    k = torch.randn(64, Hk, D, device=DEV, dtype=torch.bfloat16)
    cu_q = torch.tensor([0, Lq], device=DEV, dtype=torch.int32)
    kr = torch.tensor([[0, 40]], device=DEV, dtype=torch.int32)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="decode kernel only"):
            ext().fa_fwd(q, k, k, cu_q, cu_q, Lq, 0.125, True, -1, 0.0, 0, -1, 64, kr)
        with pytest.raises(ValueError, match="decode kernel only"):
            attention.flash_attention(q, k, k, cu_q, None, Lq, 64, 0.125, True, key_ranges=kr)
        with pytest.raises(ValueError, match="dropout"):
            attention.flash_attention(q[:1], k, k, cu_q.clamp(max=1), None, 1, 64, 0.125, True, dropout_p=0.1,
                                      training=True, key_ranges=kr)


# ---------------------------------------------------------------------------------------------- graph == eager
def _sampler(sampled):
    from scaling_amd.transformer.inference import Sampler

    return {"sample_fn": Sampler(0.8, 40, 0.95, seed=1)} if sampled else {}


def _assert_same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.completion_tokens == y.completion_tokens, (x.completion_tokens, y.completion_tokens)
        torch.testing.assert_close(x.completion_logits.float().cpu(), y.completion_logits.float().cpu(),
                                   rtol=1e-2, atol=1e-2)


def _graph_equals_eager(m, B, sampled):
    kw = _sampler(sampled)
    prompts = PROMPTS[:B]
    eager = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=[], **kw)
    graph = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=[], use_cuda_graph=True, **kw)
    assert all(len(o.completion_tokens) == MAX_TOKENS for o in eager)
    _assert_same(graph, eager)
    again = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=[], use_cuda_graph=True, **kw)
    for x, y in zip(again, graph):
        assert x.completion_tokens == y.completion_tokens and torch.equal(x.completion_logits, y.completion_logits)
    # per-row stop tokens: one taken from each row's own text, at a different step per row
    stops = [o.completion_tokens[4 + 5 * b] for b, o in enumerate(eager)]
    eager_s = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=stops, **kw)
    graph_s = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=stops, use_cuda_graph=True, **kw)
    _assert_same(graph_s, eager_s)
    for o, full in zip(eager_s, eager):
        n = len(o.completion_tokens)
        assert o.completion_tokens == full.completion_tokens[:n] and n <= 4 + 5 * (B - 1) + 1
        assert o.completion_tokens[-1] in stops and not any(t in stops for t in o.completion_tokens[:-1])
        assert o.completion_logits.shape[0] == n
    again_s = m.generate_batch(MAX_TOKENS, input_tokens=prompts, stop_tokens=stops, use_cuda_graph=True, **kw)
    for x, y in zip(again_s, graph_s):
        assert x.completion_tokens == y.completion_tokens and torch.equal(x.completion_logits, y.completion_logits)


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_batch_graph_equals_eager(model, B, sampled):
    _graph_equals_eager(model, B, sampled)


def test_batch_graph_equals_eager_fp8(qmodel):
    _graph_equals_eager(qmodel, 3, False)
    _graph_equals_eager(qmodel, 3, True)


def test_graph_limit_is_four_rows(model):
    with pytest.raises(ValueError, match="at most 4"):
        model.generate_batch(4, input_tokens=PROMPTS[:5], stop_tokens=[], use_cuda_graph=True)


# ---------------------------------------------------------------------------------------------- batched follows single
@pytest.mark.parametrize("B,graph", [(4, True), (6, False)])
def test_batched_follows_single_teacher_forced(model, singles, B, graph):
    """Every row is fed the tokens of its own single-sequence greedy generation through the decoder's ``tok`` buffer;
    its logits must follow the single-sequence logits (which are teacher-forced on the same tokens by construction):
    step 0 bitwise (the same prefill, run alone), every later step within the bound the project uses for two kernel
    paths computing one function on this model (cached vs uncached, FP8 vs twin)."""
    want = singles[:B]
    assert all(len(s.completion_tokens) == MAX_TOKENS for s in want)
    dec = model.batch_decoder(MAX_TOKENS, PROMPTS[:B])
    if graph:
        dec.capture()
    for b, s in enumerate(want):
        assert torch.equal(dec.logits[0, b], s.completion_logits[0])
        assert int(dec.tokens[0, b]) == s.completion_tokens[0]
    for k in range(1, MAX_TOKENS):
        dec.tok.copy_(torch.tensor([[s.completion_tokens[k - 1]] for s in want], device=dec.tok.device))
        dec.step()
    dec.state.check()
    got = dec.logits[:MAX_TOKENS].float()  # [steps, B, V]
    ref = torch.stack([s.completion_logits.float() for s in want], dim=1)
    assert got.shape == ref.shape == (MAX_TOKENS, B, 256)
    diff = (got - ref).abs().amax(dim=2)
    print(f"B={B} graph={graph}: max |logit difference| per step (over rows):",
          [round(float(d), 4) for d in diff.amax(dim=1)])
    print("per row (over steps):", [round(float(d), 4) for d in diff.amax(dim=0)])
    torch.testing.assert_close(got, ref, rtol=5e-2, atol=5e-2)  # every step of every row, none left out


# ---------------------------------------------------------------------------------------------- kernels taken
W8 = ("gemv_w8", "gemv_w8_residual", "gemv_w8_swiglu", "gemv_w8_norm")
BF16 = ("gemv", "gemv_residual", "gemv_swiglu", "gemv_norm", "gemv_norm_rope")


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


@pytest.mark.parametrize("B", [2, 4])
def test_batched_step_takes_fused_kernels(model, monkeypatch, B):
    """Per captured layer step: the batched RoPE + K/V append once, gemv_norm twice (norm + q/k/v, norm + gate/up +
    SwiGLU), gemv_residual once (down + residual) -- each path declines silently when a layout check fails."""
    calls = _count(monkeypatch, ("rope_kv_append_batch", "rope_kv_append") + W8 + BF16)
    model.generate_batch(4, input_tokens=PROMPTS[:B], stop_tokens=[], use_cuda_graph=True)
    assert calls.get("rope_kv_append_batch", 0) >= LAYERS, calls
    assert calls.get("gemv_norm", 0) >= 2 * LAYERS and calls.get("gemv_residual", 0) >= LAYERS, calls
    assert calls.get("rope_kv_append", 0) == 0 and all(calls.get(k, 0) == 0 for k in W8), calls


@pytest.mark.parametrize("B", [2, 4])
def test_batched_step_takes_fp8_kernels(qmodel, monkeypatch, B):
    calls = _count(monkeypatch, ("rope_kv_append_batch",) + W8 + BF16)
    qmodel.generate_batch(4, input_tokens=PROMPTS[:B], stop_tokens=[], use_cuda_graph=True)
    assert calls.get("rope_kv_append_batch", 0) >= LAYERS, calls
    assert calls.get("gemv_w8_norm", 0) >= 2 * LAYERS and calls.get("gemv_w8_residual", 0) >= LAYERS, calls
    assert calls.get("gemv_w8", 0) >= LAYERS, calls
    # no bf16 GEMV inside the layers (ext().gemv still serves the tied, never-quantised head of this model)
    assert all(calls.get(k, 0) == 0 for k in ("gemv_norm", "gemv_residual", "gemv_swiglu", "gemv_norm_rope")), calls
