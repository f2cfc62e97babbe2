"""MXFP4-weight decode GEMV (the MXFP4 weight format of ``csrc/kernels/gemv.hip``) against float math on the DEQUANTISED
weights (GPU only).

The MXFP4 copy is an exact encoding of the bf16 values it was made from (``ops/quant.py``), so the tolerances are the
FP8 tests' (``test_gemv_fp8_gpu.py``): 2e-2 against float math, 3e-2 against the bf16 kernel on the same values, with
no quantisation term.  x is N(0,1), w is N(0,1)/sqrt(K) before quantisation.

Launch rules of the format (``w4_rules`` in gemv.hip): waves per row 4 for the plain / residual forms when N <= 8192
and K >= 2 N, else 1; rows per wave 4 when N x waves per row >= 8192, else 2, halved until they divide N.  Every shape
below names the rule it takes; ``test_every_candidate_rule`` runs every kernel the A/B switch can select.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import gemm, quant  # noqa: E402
from scaling_amd.ops import norm as norm_ops  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
TOL = dict(atol=2e-2, rtol=2e-2)
TOL_BF = dict(atol=3e-2, rtol=3e-2)
_cache: dict = {}


def _quantised(N, K, seed=0):
    """(codes, scales, dequantised bf16 weight) of a seeded N(0,1)/sqrt(K) matrix (computed once per shape)."""
    key = (N, K, seed)
    if key not in _cache:
        g = torch.Generator(device=DEV).manual_seed(seed)
        w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(BF)
        c, s = quant.quantize_rows_mxfp4(w)
        _cache[key] = (c, s, quant.dequantize_rows_mxfp4(c, s, BF))
    return _cache[key]


def _x(M, K, seed=1):
    return torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(BF)


def _ref(x, wd):
    return (x.double() @ wd.double().t()).float()


@pytest.mark.parametrize("M,N,K", [
    (1, 5, 32),          # 1 row / wave (odd N), 4 waves / row (K >= 2 N); one block: three K slices own no piece
    (3, 77, 64),         # 1 row / wave, 1 wave / row
    (2, 1003, 224),      # 1 row / wave, 1 wave / row; 7 blocks: a ragged trip
    (2, 264, 96),        # 2 rows / wave, 1 wave / row
    (1, 64, 4128),       # 2 rows / wave, 4 waves / row; one block past a full trip
    (2, 2064, 4128),     # 4 rows / wave (N x 4 >= 8192), 4 waves / row (K = 2 N)
    (4, 4100, 11008),    # 4 rows / wave, 4 waves / row, the down projection's K
    (4, 4128, 4096),     # 2 rows / wave, 1 wave / row at K = 4096: 128 pieces, two per lane
    (3, 8200, 64),       # 4 rows / wave, 1 wave / row
    (1, 8198, 64),       # 2 rows / wave (N % 4 != 0) where the rule asks for 4
])
@pytest.mark.parametrize("bias", [False, True])
def test_gemv_w4(M, N, K, bias, monkeypatch):
    """Plain (+ bias): ext().gemv_w4, and through ops.gemm.linear on a quantised parameter (which must route to it);
    a row-strided x; row slices of a shared buffer."""
    c, s, wd = _quantised(N, K)
    x = _x(M, K)
    b = _x(1, N, seed=2).view(N) if bias else None
    ref = _ref(x, wd) + (b.float() if bias else 0.0)
    assert ext().gemv_w4_ok(x, c, s)
    y = ext().gemv_w4(x, c, s, b)
    torch.testing.assert_close(y.float(), ref, **TOL)
    torch.testing.assert_close(y, ext().gemv(x, wd, b), **TOL_BF)
    assert torch.equal(ext().gemv_w4(x, c, s, b), y)  # deterministic
    if N > 2064:
        return
    # through linear() on a quantised parameter
    p = torch.nn.Parameter(wd.clone(), requires_grad=False)
    quant.quantize_parameters([p], "mxfp4")
    assert torch.equal(p.data, wd)
    calls = []
    real = ext().gemv_w4
    monkeypatch.setattr(ext(), "gemv_w4", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    yl = gemm.linear(x.view(M, 1, K), p, b)
    monkeypatch.undo()
    assert calls == [1] and torch.equal(yl.view(M, N), y)
    # a row-strided x
    xw = torch.zeros(M, K + 24, device=DEV, dtype=BF)
    xw[:, 8 : 8 + K] = x
    xs = xw[:, 8 : 8 + K]
    assert ext().gemv_w4_ok(xs, c, s) and torch.equal(ext().gemv_w4(xs, c, s, b), y)
    # a row slice of a larger group buffer (rows before and after it)
    n0 = 16
    big_c = torch.cat([torch.full((n0, K // 2), 0x77, device=DEV, dtype=torch.uint8), c, c[:3]])
    big_s = torch.cat([torch.full((n0, K // 32), 140, device=DEV, dtype=torch.uint8), s, s[:3]])
    cv, sv = big_c[n0 : n0 + N], big_s[n0 : n0 + N]
    assert ext().gemv_w4_ok(x, cv, sv) and torch.equal(ext().gemv_w4(x, cv, sv, b), y)


@pytest.mark.parametrize("M", [1, 3])
def test_gemv_w4_block_scales_zero_blocks_and_every_code(M):
    """Neighbouring blocks 2^+-20 apart in scale (x scaled the other way, so that every block contributes alike and a
    scale taken from the wrong block is a gross error), all-zero blocks, and a row of hand-placed codes with every one
    of the 16 code values, -0 included."""
    N, K = 12, 4128
    nb = K // 32
    g = torch.Generator(device=DEV).manual_seed(3)
    e = torch.tensor([0, 20, -20, 0, -20, 20, 3], device=DEV)[torch.arange(nb, device=DEV) % 7]
    bs = torch.ldexp(torch.ones((), device=DEV), e)  # [nb]
    w = torch.randn(N, K, device=DEV, generator=g).view(N, nb, 32) * bs[None, :, None]
    w[2, 5] = 0
    w[3] = 0
    w[4, ::2] = 0
    c, s = quant.quantize_rows_mxfp4(w.view(N, K).to(BF))
    assert int(s.max()) - int(s.min()) >= 40 and (s[3] == 127).all()
    # row 5: every code value in turn, with scales cycling through 2^-3..2^3
    allc = (torch.arange(K, device=DEV) % 16).to(torch.uint8)
    c[5] = allc[0::2] | (allc[1::2] << 4)
    s[5] = (124 + torch.arange(nb, device=DEV) % 7).to(torch.uint8)
    wd = quant.dequantize_rows_mxfp4(c, s, BF)
    assert (wd[5, 8::16] == 0).all()  # the -0 codes
    x = (_x(M, K).float().view(M, nb, 32) / bs[None, :, None]).view(M, K).to(BF)
    y = ext().gemv_w4(x, c, s)
    ref = _ref(x, wd)
    torch.testing.assert_close(y.float(), ref, **TOL)
    assert bool((y[:, 3] == 0).all())
    # rows on a common unit: the blocks' contributions are O(sqrt(32)) each by construction
    rest = [n for n in range(N) if n != 5]
    assert float(ref[:, rest].abs().max()) < 1e3 and float(ref[:, 0].abs().min()) > 0
    # row 5 against x that sees the codes' plain values
    x5 = _x(M, K, seed=9)
    unit = float(wd[5].float().norm())  # the row's own unit: the dot product with N(0,1) inputs has this deviation
    torch.testing.assert_close(ext().gemv_w4(x5, c, s)[:, 5].float() / unit, _ref(x5, wd)[:, 5] / unit, **TOL)


def _exact_case(M, N, K, seed):
    """Small integers in x, e2m1 grid values times 2^-2..2^2 in w: every product is a multiple of 2^-3 below 2^7 and
    every partial sum of K = 4128 of them stays below 2^19, i.e. needs 22 bits: exact in fp32 in any order."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    c = torch.randint(0, 256, (N, K // 2), device=DEV, generator=g, dtype=torch.uint8)  # every code, -0 included
    s = torch.randint(125, 130, (N, K // 32), device=DEV, generator=g, dtype=torch.uint8)
    x = torch.randint(-4, 5, (M, K), device=DEV, generator=g).to(BF)
    wd = quant.dequantize_rows_mxfp4(c, s, BF)
    return x, c, s, wd


@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("N", [40, 2064, 2073])  # 4 waves / row x 2 and x 4 rows / wave; 1 wave / row, 1 row / wave
def test_gemv_w4_exact(M, N):
    """Plain and residual forms equal the reference BITWISE where every fp32 sum is exact."""
    K = 4128
    x, c, s, wd = _exact_case(M, N, K, seed=M)
    ref64 = x.double() @ wd.double().t()
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    y = ext().gemv_w4(x, c, s)
    assert torch.equal(y, ref.to(BF))
    res = _x(M, N, seed=4)
    yr = ext().gemv_w4_residual(x, c, s, res)
    assert torch.equal(yr, (ref.to(BF).float() + res.float()).to(BF))


def test_every_candidate_rule():
    """The A/B switch of tools/gemv_bench.py: every (rows per wave, waves per row) kernel of every form, bitwise on
    the exact construction (plain, residual) and within tolerance of float math (SwiGLU, norm)."""
    K, N, M = 4128, 136, 3
    x, c, s, wd = _exact_case(M, N, K, seed=11)
    ref = (x.double() @ wd.double().t()).float()
    res = _x(M, N, seed=4)
    xr = _x(M, K)
    cq, sq, wq = _quantised(N, K)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    add = _x(M, K, seed=2)
    F = N // 2
    s_ref, _ = norm_ops.add_rms_norm(add, xr, gam, 1e-5)

    def rms(t):
        t = t.float()
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5) * gam.float()

    sw = torch.nn.functional.silu(xr.float() @ wq[:F].float().t()) * (xr.float() @ wq[F:].float().t())
    try:
        for rpw in (1, 2, 4):
            for ks in (1, 4):
                ext().gemv_w4_rule(rpw, ks)
                assert torch.equal(ext().gemv_w4(x, c, s), ref.to(BF)), (rpw, ks)
                assert torch.equal(ext().gemv_w4_residual(x, c, s, res), (ref.to(BF).float() + res.float()).to(BF)), (rpw, ks)
                torch.testing.assert_close(ext().gemv_w4_swiglu(xr, cq, sq).float(), sw, **TOL)
                so, y = ext().gemv_w4_norm(xr, add, gam, 1e-5, cq, sq, 0)
                assert torch.equal(so, s_ref), (rpw, ks)
                torch.testing.assert_close(y.float(), rms(s_ref) @ wq.float().t(), **TOL)
                _, y2 = ext().gemv_w4_norm(xr, None, gam, 1e-5, cq, sq, 2)
                torch.testing.assert_close(
                    y2.float(), torch.nn.functional.silu(rms(xr) @ wq[:F].float().t()) * (rms(xr) @ wq[F:].float().t()), **TOL)
    finally:
        ext().gemv_w4_rule(0, 0)


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_gemv_w4_epilogues(rows):
    """SwiGLU over [gate; up] (the halves 16x apart) and down + residual: against float math and against the bf16
    kernels on the dequantised weights.  The FP8 test's shapes with K = 528 rounded up to 544."""
    F, K = 136, 544
    g = torch.Generator(device=DEV).manual_seed(rows)
    w = torch.randn(2 * F, K, device=DEV, generator=g) / math.sqrt(K)
    w[F:] *= 16
    c, s = quant.quantize_rows_mxfp4(w.to(BF))
    wd = quant.dequantize_rows_mxfp4(c, s, BF)
    x = _x(rows, K)
    h = ext().gemv_w4_swiglu(x, c, s)  # 2 rows / wave, 1 wave / row
    hf = torch.nn.functional.silu(x.float() @ wd[:F].float().t()) * (x.float() @ wd[F:].float().t())
    torch.testing.assert_close(h.float(), hf, **TOL)
    torch.testing.assert_close(h, ext().gemv_swiglu(x, wd), **TOL_BF)
    assert torch.equal(ext().gemv_w4_swiglu(x, c, s), h)
    # odd F: one row per wave
    co, so_, wo_ = _quantised(2 * 135, K, seed=21)
    ho = ext().gemv_w4_swiglu(x, co, so_)
    torch.testing.assert_close(
        ho.float(), torch.nn.functional.silu(x.float() @ wo_[:135].float().t()) * (x.float() @ wo_[135:].float().t()), **TOL)
    # F = 8200: four output rows (eight weight rows) per wave
    cb, sb, wb = _quantised(2 * 8200, 64, seed=23)
    xb = _x(rows, 64)
    torch.testing.assert_close(
        ext().gemv_w4_swiglu(xb, cb, sb).float(),
        torch.nn.functional.silu(xb.float() @ wb[:8200].float().t()) * (xb.float() @ wb[8200:].float().t()), **TOL)
    # residual epilogue over K = 544: N = 136 takes the K-split form (K >= 2 N), N = 544 one wave per row, N = 135 odd
    for N in (F, K, 135):
        cr, sr, wo = _quantised(N, K, seed=7 + N)
        res = _x(rows, N, seed=4)
        y = ext().gemv_w4_residual(x, cr, sr, res)
        torch.testing.assert_close(y.float(), _ref(x, wo).to(BF).float() + res.float(), **TOL)
        torch.testing.assert_close(y, ext().gemv_residual(x, wo, res), **TOL_BF)
        assert torch.equal(ext().gemv_w4_residual(x, cr, sr, res), y)


@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("N,K", [(264, 544), (263, 544), (264, 4128), (263, 4128), (8200, 96)])
def test_gemv_w4_norm(rows, N, K):
    """RMSNorm prologue (with and without the residual add; two rows per wave for N = 264, one for odd N, four for
    N = 8200, plain and SwiGLU alike; always one wave per row): s is bit-identical to add_rms_norm's, y matches float
    math, plain and SwiGLU."""
    F = N // 2 if N == 264 else N  # SwiGLU over [2F, K]: F = 132 (two rows per wave), 263 (one), 8200 (four)
    x = _x(rows, K)
    add = _x(rows, K, seed=2)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    c, s, wd = _quantised(N, K)
    c2, s2, wd2 = _quantised(2 * F, K, seed=5)
    assert ext().gemv_w4_norm_ok(x, c, s, gam)

    def rms(t):
        t = t.float()
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5) * gam.float()

    def swiglu(n):
        return torch.nn.functional.silu(n @ wd2[:F].float().t()) * (n @ wd2[F:].float().t())

    so, y = ext().gemv_w4_norm(x, None, gam, 1e-5, c, s, 0)
    assert so.data_ptr() == x.data_ptr()
    torch.testing.assert_close(y.float(), rms(x) @ wd.float().t(), **TOL)
    torch.testing.assert_close(y, ext().gemv_norm(x, None, gam, 1e-5, wd, 0)[1], **TOL_BF)
    _, y2 = ext().gemv_w4_norm(x, None, gam, 1e-5, c2, s2, 2)
    torch.testing.assert_close(y2.float(), swiglu(rms(x)), **TOL)
    s_ref, _ = norm_ops.add_rms_norm(add, x, gam, 1e-5)
    sa, ya = ext().gemv_w4_norm(x, add, gam, 1e-5, c, s, 0)
    assert torch.equal(sa, s_ref)  # norm_sum is bitwise rnd(x + add)
    assert torch.equal(sa, (x.float() + add.float()).to(BF))
    torch.testing.assert_close(ya.float(), rms(s_ref) @ wd.float().t(), **TOL)
    sb, yb = ext().gemv_w4_norm(x, add, gam, 1e-5, c2, s2, 2)
    assert torch.equal(sb, s_ref)
    torch.testing.assert_close(yb.float(), swiglu(rms(s_ref)), **TOL)
    torch.testing.assert_close(yb, ext().gemv_norm(x, add, gam, 1e-5, wd2, 2)[1], **TOL_BF)
    for a, e, cc, ss, want in ((None, 0, c, s, y), (None, 2, c2, s2, y2), (add, 0, c, s, ya), (add, 2, c2, s2, yb)):
        assert torch.equal(ext().gemv_w4_norm(x, a, gam, 1e-5, cc, ss, e)[1], want)


def test_gemv_w4_rejects_unsupported():
    c, s, _ = _quantised(32, 64)
    x = _x(5, 64)
    ok = ext().gemv_w4_ok
    assert ok(x[:4], c, s) and ok(x[:1], c, s)
    assert not ok(x, c, s)  # 5 rows
    assert not ok(x[:1, :48], c[:, :24].contiguous(), s)  # K % 32
    assert not ok(_x(1, 48), torch.zeros(32, 24, device=DEV, dtype=torch.uint8),
                  torch.zeros(32, 1, device=DEV, dtype=torch.uint8))
    assert not ok(x[:1].half(), c, s) and not ok(x[:1].float(), c, s)  # bf16 activations only
    wide = torch.zeros(32, 64, device=DEV, dtype=torch.uint8)
    assert not ok(x[:1], wide[:, :32], s)  # code rows 64 bytes apart: not whole rows of the buffer
    assert not ok(x[:1], wide[:, 16:48], s)
    sw = torch.zeros(32, 4, device=DEV, dtype=torch.uint8)
    assert not ok(x[:1], c, sw[:, :2]) and not ok(x[:1], c, sw[:, ::2])  # non-contiguous scale rows
    assert not ok(x[:1], c, s[:31]) and not ok(x[:1], c, torch.cat([s, s]))  # scales of the wrong shape
    assert not ok(x[:1], c, s.view(-1)) and not ok(x[:1], c, s.float())
    assert not ok(x[:1], c.to(torch.int8), s) and not ok(x[:1], c.cpu(), s) and not ok(x[:1], c, s.cpu())
    odd = torch.zeros(33 * 32 + 8, device=DEV, dtype=torch.uint8)[8:].view(33, 32)
    assert not ok(x[:1], odd[:32], s)  # misaligned base (byte offset 8)
    with pytest.raises(RuntimeError):
        ext().gemv_w4(x, c, s)
    # the FP8 entry points keep rejecting MXFP4 operands (2-D scales), on both kernels
    assert not ext().gemv_w8_ok(x[:1], c, s) and not ext().skinny_w8_ok(x[:1], c, s)
    assert not ext().gemv_w8_norm_ok(x[:1], c, s, torch.ones(64, device=DEV, dtype=BF))
    with pytest.raises(RuntimeError):
        ext().gemv_w8(x[:1], c, s)
    with pytest.raises(RuntimeError):
        ext().skinny_w8_residual(x[:1], c, s, _x(1, 32))
    with pytest.raises(RuntimeError):
        ext().gemv_w4_swiglu(x[:1], c[:31], s[:31])  # an odd number of [gate; up] rows
    gam = torch.ones(64, device=DEV, dtype=BF)
    assert ext().gemv_w4_norm_ok(x[:2], c, s, gam)
    assert not ext().gemv_w4_norm_ok(x[:2], c, s, gam[:48]) and not ext().gemv_w4_norm_ok(x[:2], c, s, gam.float())
    # a rejected call falls through to the dense kernel on the bf16 parameter, which holds the same values
    p = torch.nn.Parameter(_quantised(32, 64)[2].clone(), requires_grad=False)
    quant.quantize_parameters([p], "mxfp4")
    xh = x[:2].half()
    y = gemm.linear(xh, p.data.half())
    torch.testing.assert_close(y.float(), xh.float() @ p.data.float().t(), **TOL)
