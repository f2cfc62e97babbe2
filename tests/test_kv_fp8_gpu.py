"""FP8 e4m3 KV cache on the GPU: the quantising RoPE + K/V append kernel against ``quantize_kv_rows`` of the rows the
bf16 kernel writes (bit for bit), flash-decoding over FP8 K/V against the bf16 kernel on the dequantised cache (bit for
bit) and the float reference, and ``generate`` / ``generate_batch`` with ``kv_cache="fp8_e4m3"``: graph versus eager,
teacher-forced logits against a bf16 cache holding the dequantised values, the kernels taken, the limits."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from batch_decode_common import MAX_TOKENS, PROMPTS, make_model  # noqa: E402
from scaling_amd.core.nn.attention import attention as attn_mod  # noqa: E402
from scaling_amd.core.nn.attention.attention import (BatchStaticKVCache, BatchStaticKVCacheFP8,  # noqa: E402
                                                     StaticKVCacheFP8)
from scaling_amd.ops import attention, quant  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402
from scaling_amd.transformer.inference import batch_decode  # noqa: E402

DEV = "cuda"
FP8 = "fp8_e4m3"
LAYERS = 2
BF = torch.bfloat16


# ---------------------------------------------------------------------------------------------- append kernel
def _rope_tables(rows, rd):
    half = rd // 2
    inv = 1.0 / (10000 ** (torch.arange(0, half, device=DEV, dtype=torch.float32) / half))
    ang = torch.arange(rows, device=DEV, dtype=torch.float32)[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


NQ, NKV, CAP = 4, 2, 48
SENT_CODE, SENT_SCALE = 0xA5, -7.0


def _append_both(qkv, positions, rd, interleaved, single=False):
    """The bf16 kernel and the FP8 kernel on the same projection rows.  Returns (q bf16 form, K, V bf16 caches, err),
    (q FP8 form, K codes, V codes, K scales, V scales, err)."""
    B, _, hd = qkv.shape
    cos, sin = _rope_tables(64, rd)
    pos = torch.tensor(positions, device=DEV, dtype=torch.long)
    kb = torch.zeros(B * CAP, NKV, hd, device=DEV, dtype=BF)
    vb = torch.zeros_like(kb)
    kc = torch.full((B * CAP, NKV, hd), SENT_CODE, device=DEV, dtype=torch.uint8)
    vc = kc.clone()
    ks = torch.full((NKV, B * CAP), SENT_SCALE, device=DEV, dtype=torch.float32)
    vs = ks.clone()
    e0, e1 = (torch.zeros(1, device=DEV, dtype=torch.int32) for _ in range(2))
    if single:
        assert B == 1
        q0 = ext().rope_kv_append(qkv, cos, sin, pos, NQ, NKV, rd, interleaved, kb, vb, e0)
        q1 = ext().rope_kv_append(qkv, cos, sin, pos, NQ, NKV, rd, interleaved, kc, vc, e1, ks, vs)
    else:
        q0 = ext().rope_kv_append_batch(qkv, cos, sin, pos, NQ, NKV, rd, interleaved, kb, vb, e0, CAP)
        q1 = ext().rope_kv_append_batch(qkv, cos, sin, pos, NQ, NKV, rd, interleaved, kc, vc, e1, CAP, ks, vs)
    assert q0 is not None and q1 is not None and q1.dtype == BF and tuple(q1.shape) == (B, NQ, hd)
    return (q0, kb, vb, int(e0.item())), (q1, kc, vc, ks, vs, int(e1.item()))


def _check_rows(bf, f8, rows):
    """The written rows are quantize_kv_rows of the bf16 kernel's rows; every other row keeps the sentinel."""
    (q0, kb, vb, _), (q1, kc, vc, ks, vs, _) = bf, f8
    assert torch.equal(q0, q1)
    idx = torch.tensor(rows, device=DEV, dtype=torch.long)
    for cache, codes, scale in ((kb, kc, ks), (vb, vc, vs)):
        want_q, want_s = quant.quantize_kv_rows(cache[idx])
        assert torch.equal(codes[idx], want_q), (codes[idx] != want_q).nonzero()[:8]
        assert torch.equal(scale[:, idx], want_s), (scale[:, idx], want_s)
        other = torch.ones(codes.shape[0], dtype=torch.bool, device=DEV)
        other[idx] = False
        assert bool((codes[other] == SENT_CODE).all()) and bool((scale[:, other] == SENT_SCALE).all())


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("hd,rd", [(32, 32), (64, 64), (64, 32), (128, 128), (128, 64)])
def test_append_equals_quantised_bf16_rows(hd, rd, interleaved):
    g = torch.Generator(device=DEV).manual_seed(hd + rd)
    for B, positions in ((1, [29]), (3, [0, 29, 47])):
        # rows of different magnitude, so the scales differ
        mag = torch.tensor([2.0 ** (3 * b - 2) for b in range(B)], device=DEV).view(B, 1, 1)
        qkv = (torch.randn(B, NQ + 2 * NKV, hd, device=DEV, generator=g) * mag).to(BF)
        bf, f8 = _append_both(qkv, positions, rd, interleaved)
        assert bf[3] == 0 and f8[5] == 0
        _check_rows(bf, f8, [b * CAP + p for b, p in enumerate(positions)])
        assert len(set(f8[3][:, [b * CAP + p for b, p in enumerate(positions)]].flatten().tolist())) >= B
    bf, f8 = _append_both(qkv[:1].contiguous(), [31], rd, interleaved, single=True)  # the one-sequence entry point
    assert f8[5] == 0
    _check_rows(bf, f8, [31])


@pytest.mark.parametrize("interleaved", [False, True])
def test_append_constructed_rows(interleaved):
    """Position 0 rotates by the identity, so k rows can be constructed like v rows: an all-zero head, amax exactly
    448 * 2^e and 224 * 2^e (the m == 0.5 case of quantize_rows_fp8), values on subnormal codes and on the ties between
    them, an amax below the scale clamp 448 * 2^-100 and a bf16-subnormal amax."""
    hd = 64
    sub = torch.tensor([2.0 ** -9 * t for t in (1, 1.5, 2, 2.5, 3, 3.5, 5, 6.5, 7, 7.5, 8, 0.5, 0.25, 0.75, -0.5, -1.5)])
    rows = []
    for e in (0, 5, -12):
        for top in (448.0, 224.0, 240.0, 232.0):
            r = torch.zeros(hd)
            r[3] = top * 2.0 ** e
            r[8:24] = sub * 2.0 ** e
            r[40] = -r[3] / 3
            rows.append(r)
    tiny = torch.zeros(hd)
    tiny[5], tiny[6] = 2.0 ** -110, -(2.0 ** -112)
    subn = torch.zeros(hd)
    subn[9] = 2.0 ** -130
    rows += [torch.zeros(hd), tiny, subn]
    rows = torch.stack(rows).to(BF)
    assert float(rows[-1].float().abs().max()) == 2.0 ** -130  # a bf16 subnormal survives the cast
    B = (rows.shape[0] + NKV - 1) // NKV
    qkv = torch.zeros(B, NQ + 2 * NKV, hd, dtype=BF)
    for i, r in enumerate(rows):  # the same constructed row as a k head and as a v head
        qkv[i // NKV, NQ + i % NKV] = r
        qkv[i // NKV, NQ + NKV + i % NKV] = r
    qkv = qkv.to(DEV)
    bf, f8 = _append_both(qkv, [0] * B, 64, interleaved)
    assert bf[3] == 0 and f8[5] == 0
    assert torch.equal(bf[1][[b * CAP for b in range(B)]].reshape(-1, hd)[: rows.shape[0]].cpu(), rows)  # identity rotation
    _check_rows(bf, f8, [b * CAP for b in range(B)])
    ks = f8[3][:, [b * CAP for b in range(B)]].t().reshape(-1)[: rows.shape[0]].cpu()
    assert ks[:4].tolist() == [1.0, 0.5, 1.0, 1.0] and float(ks[-3]) == 1.0 and float(ks[-2]) == float(ks[-1]) == 2.0 ** -100
    codes = f8[1][0, 0].cpu()  # first constructed row: 448 is code 0x7e, the subnormal codes are 1..7
    assert int(codes[3]) == 0x7E and 0 < int(codes[8]) < 8


@pytest.mark.parametrize("interleaved", [False, True])
def test_append_out_of_range_rows(interleaved):
    positions = [0, 48, 47, -1, 31]
    g = torch.Generator(device=DEV).manual_seed(7)
    qkv = torch.randn(5, NQ + 2 * NKV, 64, device=DEV, generator=g).to(BF)
    bf, f8 = _append_both(qkv, positions, 64, interleaved)
    assert bf[3] == 1 and f8[5] == 1
    q = f8[0]
    assert not q[1].any() and not q[3].any() and q[0].any() and q[2].any() and q[4].any()
    _check_rows(bf, f8, [0 * CAP + 0, 2 * CAP + 47, 4 * CAP + 31])  # includes: slabs 1 and 3 are all sentinel


def test_append_non_finite_values():
    g = torch.Generator(device=DEV).manual_seed(8)
    qkv = torch.randn(3, NQ + 2 * NKV, 64, device=DEV, generator=g).to(BF)
    clean = qkv.clone()
    qkv[1, NQ, 5] = float("nan")  # a k head of sequence 1
    qkv[1, NQ + NKV + 1, 9] = float("-inf")  # a v head of sequence 1
    bf, f8 = _append_both(qkv, [0, 0, 17], 64, True)
    q1, kc, vc, ks, vs, err = f8
    assert err == 2 and bf[3] == 0
    for codes in (kc, vc):
        written = codes[[0, CAP, 2 * CAP + 17]]
        assert not bool(((written & 0x7F) == 0x7F).any())
    assert torch.isfinite(ks[:, [0, CAP, 2 * CAP + 17]]).all() and torch.isfinite(vs[:, [0, CAP, 2 * CAP + 17]]).all()
    # -inf became -2^127 = -256 * 2^119: scale 2^119, the code of -256
    assert float(vs[1, CAP]) == 2.0 ** 119 and int(vc[CAP, 1, 9]) == 0xF8
    # the unfused torch append stores the same codes and scales
    xb, bad = quant.sanitize_kv(qkv[1:2, NQ + NKV :])
    tq, ts = quant.quantize_kv_rows(xb, check=False)
    assert bool(bad) and torch.equal(tq[0], vc[CAP]) and torch.equal(ts[:, 0], vs[:, CAP])
    # the clean sequences are what they are without the bad neighbour
    _, g8 = _append_both(clean, [0, 0, 17], 64, True)
    for a, b in ((kc, g8[1]), (vc, g8[2])):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2 * CAP + 17], b[2 * CAP + 17])
    assert torch.equal(q1[0], g8[0][0]) and torch.equal(q1[2], g8[0][2]) and g8[5] == 0


# ---------------------------------------------------------------------------------------------- decode attention
def _fp8_kv(rows, Hk, D, seed, wild=False):
    """Random codes (no NaN code) and power-of-two row scales [Hk, rows]; wild: every other key (phase by head) 2^-20
    smaller, so a scale taken from a neighbouring key or head changes the result.  K values reach ~448 * 2^-8."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    codes = torch.randint(0, 256, (rows, Hk, D), device=DEV, generator=g, dtype=torch.int32)
    codes = torch.where((codes & 0x7F) == 0x7F, codes & 0x80, codes).to(torch.uint8)
    e = torch.randint(-10, -7, (Hk, rows), device=DEV, generator=g)
    if wild:
        t = torch.arange(rows, device=DEV)[None, :] + torch.arange(Hk, device=DEV)[:, None]
        e = e - 20 * (t % 2)
    return codes, torch.ldexp(torch.ones(Hk, rows, device=DEV), e)


def _garbage_outside(codes, scale, spans):
    """Bytes 0x7f (the NaN code) and NaN scales in every row outside the key spans."""
    keep = torch.zeros(codes.shape[0], dtype=torch.bool, device=DEV)
    for s0, n in spans:
        keep[s0 : s0 + n] = True
    codes[~keep] = 0x7F
    scale[:, ~keep] = float("nan")


def _decode_both(q, kc, ks, vc, vs, cu_q, cu_k, max_q, max_k, kr=None, window=-1, local_heads=-1):
    """(o, lse) of the FP8 kernel, of the bf16 kernel on the dequantised cache, and the float reference of the latter."""
    scale = 1 / math.sqrt(q.shape[-1])
    kd, vd = quant.dequantize_kv_rows(kc, ks), quant.dequantize_kv_rows(vc, vs)
    if kr is not None:  # NaN rows outside the ranges would be multiplied by masked (zero) probabilities: keep them out
        keep = torch.zeros(kc.shape[0], dtype=torch.bool, device=DEV)
        for s0, n in kr.tolist():
            keep[s0 : s0 + n] = True
        kd[~keep], vd[~keep] = 0, 0
    with torch.no_grad():
        o8, l8 = ext().fa_fwd(q, kc, vc, cu_q, cu_k, max_q, scale, True, window, 0.0, 0, local_heads, max_k, kr, ks, vs)
        ob, lb = ext().fa_fwd(q, kd, vd, cu_q, cu_k, max_q, scale, True, window, 0.0, 0, local_heads, max_k, kr)
    assert torch.isfinite(o8).all()
    assert torch.equal(o8, ob), (o8.float() - ob.float()).abs().max()
    assert torch.equal(l8, lb), (l8 - lb).abs().max()
    ref = attention.attention_reference(q.float(), kd.float(), vd.float(), cu_q, cu_k, scale, True, window,
                                        local_heads=None if local_heads < 0 else local_heads, key_ranges=kr)
    torch.testing.assert_close(o8.float(), ref, atol=2e-2, rtol=2e-2)
    return o8, l8, kd, vd


KEYS = [1, 31, 32, 33, 95]


def _lse_reference(q, kd, cu_q, spans, scale):
    """log-sum-exp of the causal scores per (head, query), in float."""
    Hq, Hk = q.shape[1], kd.shape[1]
    out = torch.zeros(Hq, q.shape[0], device=DEV)
    cq = cu_q.tolist()
    for i, (s0, n) in enumerate(spans):
        qi = q[cq[i] : cq[i + 1]].float().transpose(0, 1)
        ki = kd[s0 : s0 + n].float().repeat_interleave(Hq // Hk, dim=1).transpose(0, 1)
        s = torch.matmul(qi, ki.transpose(1, 2)) * scale
        Lq = qi.shape[1]
        ok = torch.arange(n, device=DEV)[None, :] <= torch.arange(Lq, device=DEV)[:, None] + (n - Lq)
        out[:, cq[i] : cq[i + 1]] = torch.logsumexp(s.masked_fill(~ok, float("-inf")), dim=-1)
    return out


@pytest.mark.parametrize("form", ["cu_k", "k_range"])
@pytest.mark.parametrize("grp,Lq", [(1, 1), (4, 1), (8, 1), (8, 4), (1, 4)])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_decode_fp8_equals_bf16_on_dequantised_cache(D, grp, Lq, form):
    Hk = 2
    nseg = len(KEYS)
    keys = [max(n, Lq) for n in KEYS]  # at least one key per query
    g = torch.Generator(device=DEV).manual_seed(D + grp)
    q = torch.randn(nseg * Lq, Hk * grp, D, device=DEV, generator=g).to(BF)
    cu_q = torch.arange(0, (nseg + 1) * Lq, Lq, device=DEV, dtype=torch.int32)
    if form == "cu_k":
        starts = [sum(keys[:i]) for i in range(nseg)]
        rows = sum(keys) + 5  # a garbage tail
        cu_k = torch.tensor(starts + [sum(keys)], device=DEV, dtype=torch.int32)
        kr = None
    else:
        cap = 96
        starts = [i * cap for i in range(nseg)]
        rows = nseg * cap
        cu_k = cu_q
        kr = torch.tensor(list(zip(starts, keys)), device=DEV, dtype=torch.int32)
    spans = list(zip(starts, keys))
    kc, ks = _fp8_kv(rows, Hk, D, 1, wild=True)
    vc, vs = _fp8_kv(rows, Hk, D, 2, wild=True)
    _garbage_outside(kc, ks, spans)
    _garbage_outside(vc, vs, spans)
    if kr is None:
        o8, l8, kd, _ = _decode_packed(q, kc, ks, vc, vs, cu_q, cu_k, Lq, spans)
    else:
        o8, l8, kd, _ = _decode_both(q, kc, ks, vc, vs, cu_q, cu_k, Lq, 96, kr=kr)
    torch.testing.assert_close(l8, _lse_reference(q, kd, cu_q, spans, 1 / math.sqrt(D)), atol=2e-2, rtol=1e-3)


def _decode_packed(q, kc, ks, vc, vs, cu_q, cu_k, Lq, spans):
    """_decode_both for the cu_k form with garbage rows after the last segment: the bf16 twin holds zeros there."""
    kr = torch.tensor(spans, device=DEV, dtype=torch.int32)
    scale = 1 / math.sqrt(q.shape[-1])
    kd, vd = quant.dequantize_kv_rows(kc, ks), quant.dequantize_kv_rows(vc, vs)
    end = spans[-1][0] + spans[-1][1]
    kd[end:], vd[end:] = 0, 0
    with torch.no_grad():
        o8, l8 = ext().fa_fwd(q, kc, vc, cu_q, cu_k, Lq, scale, True, -1, 0.0, 0, -1, 96, None, ks, vs)
        ob, lb = ext().fa_fwd(q, kd, vd, cu_q, cu_k, Lq, scale, True, -1, 0.0, 0, -1, 96)
        pub = attention.flash_attention(q, kc, vc, cu_q, cu_k, Lq, 96, scale, True, kv_scales=(ks, vs))
    assert torch.isfinite(o8).all()
    assert torch.equal(o8, ob) and torch.equal(l8, lb) and torch.equal(pub, o8)
    ref = attention.attention_reference(q.float(), kd.float(), vd.float(), cu_q, None, scale, True, key_ranges=kr)
    torch.testing.assert_close(o8.float(), ref, atol=2e-2, rtol=2e-2)
    return o8, l8, kd, vd


def test_decode_fp8_two_tiles_per_split():
    """Hkv = 8, nseg = 16, cap = 320: 8 splits wanted, 10 tiles -> 64-key splits (two tiles each), 5 splits."""
    Hk, nseg, cap, D = 8, 16, 320, 64
    lengths = [320, 1, 64, 65, 129, 255, 300, 33, 32, 96, 191, 200, 7, 128, 319, 257]
    g = torch.Generator(device=DEV).manual_seed(11)
    q = torch.randn(nseg, Hk, D, device=DEV, generator=g).to(BF)
    cu_q = torch.arange(nseg + 1, device=DEV, dtype=torch.int32)
    spans = [(i * cap, n) for i, n in enumerate(lengths)]
    kr = torch.tensor(spans, device=DEV, dtype=torch.int32)
    kc, ks = _fp8_kv(nseg * cap, Hk, D, 3, wild=True)
    vc, vs = _fp8_kv(nseg * cap, Hk, D, 4)
    _garbage_outside(kc, ks, spans)
    _garbage_outside(vc, vs, spans)
    o8, l8, kd, _ = _decode_both(q, kc, ks, vc, vs, cu_q, cu_q, 1, cap, kr=kr)
    torch.testing.assert_close(l8, _lse_reference(q, kd, cu_q, spans, 1 / math.sqrt(D)), atol=2e-2, rtol=1e-3)
    with torch.no_grad():
        pub = attention.flash_attention(q, kc, vc, cu_q, None, 1, cap, None, True, key_ranges=kr, kv_scales=(ks, vs))
    assert torch.equal(pub, o8)


def test_decode_fp8_general_combine():
    """Hkv = 2, one segment, 640 keys: 20 one-tile splits, more than the combine kernel's unrolled 16."""
    Hk, grp, D, n = 2, 4, 128, 640
    g = torch.Generator(device=DEV).manual_seed(12)
    q = torch.randn(1, Hk * grp, D, device=DEV, generator=g).to(BF)
    cu_q = torch.tensor([0, 1], device=DEV, dtype=torch.int32)
    cu_k = torch.tensor([0, n], device=DEV, dtype=torch.int32)
    kc, ks = _fp8_kv(n, Hk, D, 5, wild=True)
    vc, vs = _fp8_kv(n, Hk, D, 6, wild=True)
    o8, l8, kd, _ = _decode_both(q, kc, ks, vc, vs, cu_q, cu_k, 1, n)
    torch.testing.assert_close(l8, _lse_reference(q, kd, cu_q, [(0, n)], 1 / math.sqrt(D)), atol=2e-2, rtol=1e-3)


def test_decode_fp8_windowed_local_heads():
    Hk, grp, D, n = 2, 2, 64, 95
    g = torch.Generator(device=DEV).manual_seed(13)
    q = torch.randn(2, Hk * grp, D, device=DEV, generator=g).to(BF)
    cu_q = torch.tensor([0, 1, 2], device=DEV, dtype=torch.int32)
    cu_k = torch.tensor([0, n, n + 40], device=DEV, dtype=torch.int32)
    kc, ks = _fp8_kv(n + 40, Hk, D, 7, wild=True)
    vc, vs = _fp8_kv(n + 40, Hk, D, 8)
    _decode_both(q, kc, ks, vc, vs, cu_q, cu_k, 1, n, window=16, local_heads=2)


def test_decode_fp8_rejections():
    Hq, Hk, D = 4, 2, 64
    q = torch.randn(1, Hq, D, device=DEV, dtype=BF)
    kc, ks = _fp8_kv(64, Hk, D, 9)
    cu_q = torch.tensor([0, 1], device=DEV, dtype=torch.int32)
    cu_k = torch.tensor([0, 40], device=DEV, dtype=torch.int32)
    args = (cu_q, cu_k, 1, 0.125, True, -1)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="bfloat16 queries"):
            ext().fa_fwd(q.half(), kc, kc, *args, 0.0, 0, -1, 64, None, ks, ks)
        with pytest.raises(ValueError, match="bfloat16 queries"):
            attention.flash_attention(q.half(), kc, kc, cu_q, cu_k, 1, 64, kv_scales=(ks, ks))
        q17 = torch.randn(17, Hq, D, device=DEV, dtype=BF)  # 17 queries x 2 heads per kv head = 34 rows > 32
        cu17 = torch.tensor([0, 17], device=DEV, dtype=torch.int32)
        with pytest.raises(RuntimeError, match="decode kernel only"):
            ext().fa_fwd(q17, kc, kc, cu17, cu_k, 17, 0.125, True, -1, 0.0, 0, -1, 64, None, ks, ks)
        with pytest.raises(ValueError, match="decode kernel only"):
            attention.flash_attention(q17, kc, kc, cu17, cu_k, 17, 64, kv_scales=(ks, ks))
        with pytest.raises(RuntimeError, match="decode kernel only"):
            ext().fa_fwd(q, kc, kc, *args, 0.1, 1, -1, 64, None, ks, ks)
        with pytest.raises(ValueError, match="dropout"):
            attention.flash_attention(q, kc, kc, cu_q, cu_k, 1, 64, dropout_p=0.1, training=True, kv_scales=(ks, ks))
        with pytest.raises(RuntimeError, match="kv heads, key rows"):
            ext().fa_fwd(q, kc, kc, *args, 0.0, 0, -1, 64, None, ks[:, :32].contiguous(), ks)
        with pytest.raises(RuntimeError, match="kv heads, key rows"):
            ext().fa_fwd(q, kc, kc, *args, 0.0, 0, -1, 64, None, ks.t().contiguous(), ks.t().contiguous())
        with pytest.raises(RuntimeError, match="come together"):
            ext().fa_fwd(q, kc, kc, *args, 0.0, 0, -1, 64, None, ks, None)
        with pytest.raises(ValueError, match="kv heads, key rows"):
            attention.flash_attention(q, kc, kc, cu_q, cu_k, 1, 64, kv_scales=(ks, ks[:1]))
        with pytest.raises(RuntimeError, match="codes"):
            ext().fa_fwd(q, kc.to(BF), kc.to(BF), *args, 0.0, 0, -1, 64, None, ks, ks)


# ---------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model():
    return make_model(0, "bfloat16")


@pytest.fixture(scope="module")
def qmodel():
    m = make_model(0, "bfloat16")
    m.quantize_weights()
    return m


def _sampler(sampled):
    from scaling_amd.transformer.inference import Sampler

    return {"sample_fn": Sampler(0.8, 40, 0.95, seed=1)} if sampled else {}


def _graph_equals_eager(m, B, sampled, **kw):
    kw.update(_sampler(sampled))
    eager = m.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:B], stop_tokens=[], kv_cache=FP8, **kw)
    graph = m.generate_batch(MAX_TOKENS, input_tokens=PROMPTS[:B], stop_tokens=[], kv_cache=FP8, use_cuda_graph=True, **kw)
    assert all(len(o.completion_tokens) == MAX_TOKENS for o in eager)
    for x, y in zip(graph, eager):
        assert x.completion_tokens == y.completion_tokens, (x.completion_tokens, y.completion_tokens)
        torch.testing.assert_close(x.completion_logits.float(), y.completion_logits.float(), rtol=1e-2, atol=1e-2)
    return eager


@pytest.mark.parametrize("sampled", [False, True])
def test_batch_graph_equals_eager(model, sampled):
    _graph_equals_eager(model, 3, sampled)


@pytest.mark.parametrize("sampled", [False, True])
def test_batch_graph_equals_eager_skinny(model, sampled):
    _graph_equals_eager(model, 5, sampled, skinny_gemm=True)


@pytest.mark.parametrize("sampled", [False, True])
def test_batch_graph_equals_eager_fp8_weights(qmodel, sampled):
    _graph_equals_eager(qmodel, 3, sampled)


@pytest.mark.parametrize("sampled", [False, True])
def test_single_graph_equals_eager(model, sampled):
    """``generate`` has no eager FP8-cache loop; its graph must give the eager batched decoder's B = 1 tokens (the same
    kernels: row b of the batched append and of the ranged decode equals the one-sequence call bit for bit)."""
    kw = _sampler(sampled)
    for p in (PROMPTS[0], PROMPTS[2]):
        graph = model.generate(MAX_TOKENS, input_tokens=p, stop_tokens=[], use_cuda_graph=True, kv_cache=FP8, **kw)
        eager = model.generate_batch(MAX_TOKENS, input_tokens=[p], stop_tokens=[], kv_cache=FP8, **kw)[0]
        assert graph.completion_tokens == eager.completion_tokens and len(graph.completion_tokens) == MAX_TOKENS
        torch.testing.assert_close(graph.completion_logits.float(), eager.completion_logits.float(), rtol=1e-2, atol=1e-2)


class _DequantisedBatchCache(BatchStaticKVCache):
    """The oracle's cache: plain bf16, holding what the FP8 cache encodes."""

    @staticmethod
    def _round(x):
        return quant.dequantize_kv_rows(*quant.quantize_kv_rows(x))

    @classmethod
    def from_caches(cls, kvs, state):
        for kv in kvs:
            kv.k[: kv.length] = cls._round(kv.k[: kv.length])
            kv.v[: kv.length] = cls._round(kv.v[: kv.length])
        c = BatchStaticKVCache.from_caches(kvs, state)
        return cls(c.k, c.v, state)

    def append(self, k, v):
        return super().append(self._round(k), self._round(v))


def _teacher_forced(dec, tokens):
    for k in range(1, MAX_TOKENS):
        dec.tok.copy_(tokens[k - 1].view(-1, 1))
        dec.step()
    dec.state.check()
    return dec.logits[:MAX_TOKENS].clone()


def test_logits_equal_the_dequantised_bf16_cache_run(model, monkeypatch):
    """B = 3, teacher-forced on the FP8 run's own greedy tokens.  The oracle is the same decoder over plain bf16 caches
    whose rows are dequantize(quantize(row)), written by the unfused RoPE + append path (documented bit-identical to
    the fused kernel): bitwise equal logits.  Beside it, the bf16-cache run on the same tokens: how far the format
    moves the logits (printed, not a pass mark).

    The unfused path is forced by making ``_decode_rope_append`` decline.  Switching the module flag ``_DECODE_FUSED``
    off instead also drops the RMSNorm-folding q/k/v GEMV (``decode_norm_project``), which keeps the normalised row in
    fp32 where the unfused norm rounds it to bf16: that changes the projection itself, FP8 cache or not -- the
    control below shows the plain bf16-cache run moving by as much under that flag -- so it is no oracle for the cache."""
    B = 3
    dec = model.batch_decoder(MAX_TOKENS, PROMPTS[:B], kv_cache=FP8)
    while dec.steps_done < MAX_TOKENS:
        dec.step()
    dec.state.check()
    tokens, got = dec.tokens[:MAX_TOKENS].clone(), dec.logits[:MAX_TOKENS].clone()
    kv0 = dec.attns[0].cache[0]
    assert isinstance(kv0, BatchStaticKVCacheFP8)

    plain = _teacher_forced(model.batch_decoder(MAX_TOKENS, PROMPTS[:B]), tokens)
    rel = float((got.float() - plain.float()).pow(2).mean().sqrt() / plain.float().pow(2).mean().sqrt())
    print(f"FP8 KV cache vs bf16 KV cache, teacher-forced logits, relative RMS difference: {rel:.4f}")
    assert math.isfinite(rel) and rel > 0
    assert torch.equal(got[0], plain[0])  # the prefill reads exact K/V

    with monkeypatch.context() as mp:  # control: the module flag moves the bf16-cache run too (see the docstring)
        mp.setattr(attn_mod, "_DECODE_FUSED", False)
        plain_off = _teacher_forced(model.batch_decoder(MAX_TOKENS, PROMPTS[:B]), tokens)
        mp.setattr(batch_decode, "BatchStaticKVCache", _DequantisedBatchCache)
        want_off = _teacher_forced(model.batch_decoder(MAX_TOKENS, PROMPTS[:B]), tokens)
    print("_DECODE_FUSED off: bf16-cache run, steps x rows with unequal logits:",
          int((plain_off != plain).any(dim=2).sum()), "max |difference|:",
          float((plain_off.float() - plain.float()).abs().max()), "; oracle built that way vs FP8 run:",
          int((want_off != got).any(dim=2).sum()), float((want_off.float() - got.float()).abs().max()))

    monkeypatch.setattr(batch_decode, "BatchStaticKVCache", _DequantisedBatchCache)
    monkeypatch.setattr(attn_mod.ParallelSelfAttention, "_decode_rope_append", lambda self, *a, **k: None)
    odec = model.batch_decoder(MAX_TOKENS, PROMPTS[:B])
    assert isinstance(odec.attns[0].cache[0], _DequantisedBatchCache)
    want = _teacher_forced(odec, tokens)
    bad = (got != want).any(dim=2)
    print("steps x rows with unequal logits:", int(bad.sum()), "max |difference|:", float((got.float() - want.float()).abs().max()))
    assert torch.equal(got, want)
    # and the oracle's caches hold what the FP8 caches encode
    dk, dv = kv0.dequantized()
    ok = odec.attns[0].cache[0]
    assert torch.equal(dk, ok.k) and torch.equal(dv, ok.v)


_V_SCALE_ARG = {"fa_fwd": 15, "rope_kv_append": 12, "rope_kv_append_batch": 13}  # position of v_scale


def _count(monkeypatch, names):
    calls: dict = {}
    mod = ext()
    for name in names:
        fn = getattr(mod, name)

        def wrapped(*a, _fn=fn, _name=name, **k):
            out = _fn(*a, **k)
            at = _V_SCALE_ARG.get(_name, 99)
            fp8 = (len(a) > at and a[at] is not None) or k.get("v_scale") is not None
            key = _name + ("+scales" if fp8 else "")
            calls[key] = calls.get(key, 0) + (out is not None)
            return out

        monkeypatch.setattr(mod, name, wrapped)
    return calls


def test_fp8_entry_points_are_taken(model, monkeypatch):
    calls = _count(monkeypatch, ("rope_kv_append_batch", "rope_kv_append", "fa_fwd", "gemv_norm_rope"))
    model.generate_batch(4, input_tokens=PROMPTS[:3], stop_tokens=[], use_cuda_graph=True, kv_cache=FP8)
    assert calls.get("rope_kv_append_batch+scales", 0) >= LAYERS and calls.get("rope_kv_append_batch", 0) == 0, calls
    assert calls.get("fa_fwd+scales", 0) >= LAYERS, calls
    # without scales only the prefills (over exact bf16 K/V): at most one call per prompt and layer, so no decode step
    # (warm-up, capture) went without the scales
    assert calls.get("fa_fwd", 0) <= 3 * LAYERS, calls
    calls.clear()
    model.generate(4, input_tokens=PROMPTS[0], stop_tokens=[], use_cuda_graph=True, kv_cache=FP8)
    assert calls.get("rope_kv_append+scales", 0) >= LAYERS and calls.get("rope_kv_append", 0) == 0, calls
    assert calls.get("fa_fwd+scales", 0) >= LAYERS and calls.get("fa_fwd", 0) <= LAYERS, calls
    assert calls.get("gemv_norm_rope", 0) == 0


def test_one_launch_rope_gemv_step_declines(model, monkeypatch):
    """SCALING_AMD_DECODE_ROPE_GEMV's one-launch step writes bf16 cache rows itself: with an FP8 cache it must step aside."""
    monkeypatch.setattr(attn_mod, "_DECODE_ROPE_GEMV", True)
    calls = _count(monkeypatch, ("gemv_norm_rope", "rope_kv_append"))
    want = model.generate_batch(8, input_tokens=[PROMPTS[0]], stop_tokens=[], kv_cache=FP8)[0]
    got = model.generate(8, input_tokens=PROMPTS[0], stop_tokens=[], use_cuda_graph=True, kv_cache=FP8)
    assert calls.get("gemv_norm_rope", 0) == 0 and calls.get("rope_kv_append+scales", 0) >= LAYERS, calls
    assert got.completion_tokens == want.completion_tokens


def test_cache_tensors_and_limits(model):
    dec = model.batch_decoder(4, PROMPTS[:3], kv_cache=FP8)
    cap = dec.capacity
    for a in dec.attns:
        c = a.cache[0]
        assert isinstance(c, BatchStaticKVCacheFP8)
        for t in (c.k, c.v):
            assert t.dtype == torch.uint8 and t.element_size() == 1 and tuple(t.shape) == (3 * cap, 2, 64)
        for s in (c.k_scale, c.v_scale):
            assert s.dtype == torch.float32 and tuple(s.shape) == (2, 3 * cap)
        assert c.bytes_per_token() == 2 * 2 * (64 + 4)
    from scaling_amd.transformer.inference.graph_decode import GraphDecoder

    out = model.forward(model._pre_process_input(input_tokens=PROMPTS[0]))
    first = out.activations.argmax(-1)[:, -1:]
    gd = GraphDecoder(model, len(PROMPTS[0]), 4, first, lambda a: a.argmax(-1)[:, -1:], out.activations[:, -1, :], kv_cache=FP8)
    c = gd.attns[0].cache[0]
    assert isinstance(c, StaticKVCacheFP8) and c.k.dtype == torch.uint8 and tuple(c.k_scale.shape) == (2, len(PROMPTS[0]) + 4)
    with pytest.raises(ValueError, match="unknown kv_cache scheme"):
        model.generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache="int8")
    with pytest.raises(ValueError, match="needs use_cuda_graph=True"):
        model.generate(4, input_tokens=PROMPTS[0], stop_tokens=[], kv_cache=FP8)
    with pytest.raises(ValueError, match="bfloat16 models only"):
        make_model(0, "float16").generate(4, input_tokens=PROMPTS[0], stop_tokens=[], use_cuda_graph=True, kv_cache=FP8)
    with pytest.raises(ValueError, match="key_query_norm is not supported"):
        make_model(0, "bfloat16", key_query_norm=True).generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache=FP8)
    with pytest.raises(ValueError, match="non-flash"):
        make_model(0, "bfloat16", masked_softmax={"kernel": "torch"}).generate_batch(
            4, input_tokens=PROMPTS[:2], stop_tokens=[], kv_cache=FP8)
    # tensor parallelism: a layer whose topology says model_parallel_size = 2 (as tests/test_quant_cpu.py does)
    tp = make_model(0, "bfloat16")
    attn = [m for m in tp.modules() if isinstance(m, attn_mod.ParallelSelfAttention)]
    attn[1].topology = SimpleNamespace(config=SimpleNamespace(model_parallel_size=2))
    with pytest.raises(ValueError, match="tensor parallelism"):
        tp.generate(4, input_tokens=PROMPTS[0], stop_tokens=[], use_cuda_graph=True, kv_cache=FP8)
    with pytest.raises(ValueError, match="tensor parallelism"):
        tp.generate_batch(4, input_tokens=PROMPTS[:2], stop_tokens=[], use_cuda_graph=True, kv_cache=FP8)
    assert not any(a.cache for a in attn)  # refused before anything was prefilled
