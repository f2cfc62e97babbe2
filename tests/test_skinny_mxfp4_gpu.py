"""MXFP4 weights on the skinny MFMA decode kernel (``csrc/kernels/skinny.hip``, ``ext().skinny_w4*``; GPU only).

The tolerances are those of ``test_skinny_gpu.py``: ``TOL`` 2e-2 against float math on the dequantised values (the
copy is an exact encoding of them, and the decode to bf16 inside the kernel is exact), ``TOL_BF`` 3e-2 against the
GEMV form where M <= 4.  The launch rules are the kernel's own (``skinny_rules``: from N and the form, never M);
``RULE_SHAPES`` takes each of them.
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
# K split + one tile per wave; K split + two tiles per wave; no K split (2049 tiles, N tail of 13)
RULE_SHAPES = [(136, 544), (8200, 64), (32781, 64)]
_CACHE: dict = {}


def _weights(N, K, seed=0, up_scale=None):
    """(codes, scales, dequantised bf16 weight) of a seeded N(0,1)/sqrt(K) matrix (rows N/2.. times up_scale)."""
    key = (N, K, seed, up_scale)
    if key not in _CACHE:
        g = torch.Generator(device=DEV).manual_seed(seed)
        w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
        if up_scale is not None:
            w[N // 2:] *= up_scale
        c, s = quant.quantize_rows_mxfp4(w.to(BF))
        _CACHE[key] = (c, s, quant.dequantize_rows_mxfp4(c, s, BF))
    return _CACHE[key]


def _x(M, K, seed=1):
    return torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(BF)


def _rms(s, gam):
    s = s.float()
    return s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + 1e-5) * gam.float()


def _swiglu_ref(n, wf):
    F = wf.shape[0] // 2
    return torch.nn.functional.silu(n @ wf[:F].t()) * (n @ wf[F:].t())


# (N, K): one block; N tail 77; 7 blocks (ragged against the 128-k step); one block past a trip; odd N;
# K = 96 against the 128-k step: the fourth k-group's piece is clamped and meets a zero x fragment
PLAIN_SHAPES = [(5, 32), (77, 64), (1003, 224), (64, 4128), (263, 544), (77, 96)]


@pytest.mark.parametrize("N,K", PLAIN_SHAPES + RULE_SHAPES[1:])
@pytest.mark.parametrize("M", [1, 3, 7, 16])
def test_skinny_w4_plain(M, N, K):
    c, s, wd = _weights(N, K)
    x = _x(M, K)
    for bias in (None, _x(1, N, seed=2).view(N)):
        ref = (x.double() @ wd.double().t()).float() + (bias.float() if bias is not None else 0.0)
        assert ext().skinny_w4_ok(x, c, s)
        y = ext().skinny_w4(x, c, s, bias)
        torch.testing.assert_close(y.float(), ref, **TOL)
        if M <= 4:
            torch.testing.assert_close(y, ext().gemv_w4(x, c, s, bias), **TOL_BF)
        assert torch.equal(ext().skinny_w4(x, c, s, bias), y)  # deterministic
    # a row-strided x
    xw = torch.zeros(M, K + 24, device=DEV, dtype=BF)
    xw[:, 8: 8 + K] = x
    xs = xw[:, 8: 8 + K]
    assert ext().skinny_w4_ok(xs, c, s) and torch.equal(ext().skinny_w4(xs, c, s, bias), y)


@pytest.mark.parametrize("M", [1, 3, 7, 16])
@pytest.mark.parametrize("N", [40, 8200])  # K split with one tile per wave, and with two
def test_skinny_w4_exact(M, N):
    """x small integers, w e2m1 grid values times 2^-2..2^2, K = 4128: every product is a multiple of 2^-3 below 2^7,
    every partial sum needs at most 22 bits, so the fp32 MFMA sums are exact in any order and the plain and residual
    forms equal the reference bitwise.  Every code value occurs, -0 included."""
    K = 4128
    g = torch.Generator(device=DEV).manual_seed(M)
    c = torch.randint(0, 256, (N, K // 2), device=DEV, generator=g, dtype=torch.uint8)
    s = torch.randint(125, 130, (N, K // 32), device=DEV, generator=g, dtype=torch.uint8)
    x = torch.randint(-4, 5, (M, K), device=DEV, generator=g).to(BF)
    wd = quant.dequantize_rows_mxfp4(c, s, BF)
    ref64 = x.double() @ wd.double().t()
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64)
    assert torch.equal(ext().skinny_w4(x, c, s), ref.to(BF))
    res = _x(M, N, seed=4)
    assert torch.equal(ext().skinny_w4_residual(x, c, s, res), (ref.to(BF).float() + res.float()).to(BF))


@pytest.mark.parametrize("M", [3, 12])
def test_skinny_w4_block_scales(M):
    """Neighbouring blocks 2^+-20 apart (x scaled the other way), zero blocks and a zero row."""
    N, K = 40, 4128
    nb = K // 32
    g = torch.Generator(device=DEV).manual_seed(3)
    e = torch.tensor([0, 20, -20, 0, -20, 20, 3], device=DEV)[torch.arange(nb, device=DEV) % 7]
    bs = torch.ldexp(torch.ones((), device=DEV), e)
    w = torch.randn(N, K, device=DEV, generator=g).view(N, nb, 32) * bs[None, :, None]
    w[2, 5] = 0
    w[3] = 0
    c, s = quant.quantize_rows_mxfp4(w.view(N, K).to(BF))
    wd = quant.dequantize_rows_mxfp4(c, s, BF)
    x = (_x(M, K).float().view(M, nb, 32) / bs[None, :, None]).view(M, K).to(BF)
    y = ext().skinny_w4(x, c, s)
    # (the B operand is bf16 x itself and the A operand the exact weight: only the fp32 sums' order differs)
    torch.testing.assert_close(y.float(), (x.double() @ wd.double().t()).float(), **TOL)
    assert bool((y[:, 3] == 0).all())


def _all_forms(x, add, res, gam, w, w2):
    """Every form's output on these operands: w [N, K] for plain / RES / NORM, w2 [2N, K] for the SwiGLU forms."""
    e = ext()
    s0, n0 = e.skinny_w4_norm(x, None, gam, 1e-5, w[0], w[1], 0)
    s1, n1 = e.skinny_w4_norm(x, add, gam, 1e-5, w[0], w[1], 0)
    s2, n2 = e.skinny_w4_norm(x, add, gam, 1e-5, w2[0], w2[1], 2)
    assert s0.data_ptr() == x.data_ptr()
    return {
        "plain": e.skinny_w4(x, w[0], w[1], None),
        "res": e.skinny_w4_residual(x, w[0], w[1], res),
        "swiglu": e.skinny_w4_swiglu(x, w2[0], w2[1]),
        "norm": n0, "add_norm": n1, "add_norm_s": s1, "add_norm_swiglu": n2, "add_norm_swiglu_s": s2,
        "norm_swiglu": e.skinny_w4_norm(x, None, gam, 1e-5, w2[0], w2[1], 2)[1],
    }


@pytest.mark.parametrize("N,K", RULE_SHAPES)
def test_skinny_w4_batch_invariance(N, K):
    """Row m of the M-row call is bitwise the 1-row call on x[m : m + 1], for M = 16 and M = 7, every form, every
    launch rule."""
    w, w2 = _weights(N, K), _weights(2 * N, K, seed=5)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    x, add, res = _x(16, K), _x(16, K, seed=2), _x(16, N, seed=4)
    single = [_all_forms(x[m: m + 1], add[m: m + 1], res[m: m + 1], gam, w, w2) for m in range(16)]
    for M in (16, 7):
        full = _all_forms(x[:M].clone(), add[:M].clone(), res[:M].clone(), gam, w, w2)
        for name, y in full.items():
            assert y.shape[0] == M
            for m in range(M):
                assert torch.equal(y[m: m + 1], single[m][name]), (name, M, m)
    x2, add2 = x.clone(), add.clone()
    x2[1:] = _x(15, K, seed=9) * 3
    add2[1:] = _x(15, K, seed=10)
    other = _all_forms(x2, add2, res, gam, w, w2)
    for name, y in other.items():
        assert torch.equal(y[:1], single[0][name]), name


@pytest.mark.parametrize("M", [1, 7, 15])
def test_skinny_w4_padding_rows_are_not_read(M):
    """x / add / res are the first M rows of 16-row buffers whose other rows are NaN: the outputs are finite and equal
    those of M-row operands."""
    N, K = 136, 544
    w, w2 = _weights(N, K), _weights(2 * N, K, seed=5)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    x, add, res = _x(M, K), _x(M, K, seed=2), _x(M, N, seed=4)
    want = _all_forms(x, add, res, gam, w, w2)

    def padded(t):
        buf = torch.full((16, t.shape[1]), float("nan"), device=DEV, dtype=t.dtype)
        buf[:M] = t
        return buf[:M]

    got = _all_forms(padded(x), padded(add), padded(res), gam, w, w2)
    for name in want:
        assert bool(torch.isfinite(got[name].float()).all()), name
        assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("rows", [1, 3, 7, 16])
def test_skinny_w4_epilogues(rows):
    """SwiGLU over [gate; up] with F = 136 and F = 263 (odd), the up half 16x larger; down + residual with N = 136,
    544 and 77 (an N tail), and K = 96 (the clamped-piece path)."""
    K = 544
    x = _x(rows, K)
    for F in (136, 263):
        w = _weights(2 * F, K, seed=rows, up_scale=16.0)
        h = ext().skinny_w4_swiglu(x, w[0], w[1])
        torch.testing.assert_close(h.float(), _swiglu_ref(x.float(), w[2].float()), **TOL)
        if rows <= 4:
            torch.testing.assert_close(h, ext().gemv_w4_swiglu(x, w[0], w[1]), **TOL_BF)
        assert torch.equal(ext().skinny_w4_swiglu(x, w[0], w[1]), h)
    for N, Kr in ((136, K), (544, K), (77, K), (77, 96)):
        wo = _weights(N, Kr, seed=7 + N)
        xr, res = _x(rows, Kr), _x(rows, N, seed=4)
        y = ext().skinny_w4_residual(xr, wo[0], wo[1], res)
        ref = (xr.double() @ wo[2].double().t()).float().to(BF).float() + res.float()
        torch.testing.assert_close(y.float(), ref, **TOL)
        if rows <= 4:
            torch.testing.assert_close(y, ext().gemv_w4_residual(xr, wo[0], wo[1], res), **TOL_BF)
    w96 = _weights(2 * 77, 96, seed=31)
    x96 = _x(rows, 96)
    torch.testing.assert_close(ext().skinny_w4_swiglu(x96, w96[0], w96[1]).float(),
                               _swiglu_ref(x96.float(), w96[2].float()), **TOL)


@pytest.mark.parametrize("rows", [1, 3, 7, 16])
@pytest.mark.parametrize("N", [264, 263])
@pytest.mark.parametrize("K", [544, 4128, 96])
def test_skinny_w4_norm(rows, N, K):
    """RMSNorm prologue with and without the residual add, plain and SwiGLU: s bit-identical to add_rms_norm's, y
    against float math (and against the GEMV form for M <= 4)."""
    x, add = _x(rows, K), _x(rows, K, seed=2)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    w, w2 = _weights(N, K), _weights(2 * N, K, seed=5)
    assert ext().skinny_w4_norm_ok(x, w[0], w[1], gam)
    s_ref, _ = norm_ops.add_rms_norm(add, x, gam, 1e-5)
    for a, ww, epi in ((None, w, 0), (None, w2, 2), (add, w, 0), (add, w2, 2)):
        so, y = ext().skinny_w4_norm(x, a, gam, 1e-5, ww[0], ww[1], epi)
        sin = x if a is None else s_ref
        assert torch.equal(so, sin)
        n = _rms(sin, gam)
        ref = n @ ww[2].float().t() if epi == 0 else _swiglu_ref(n, ww[2].float())
        torch.testing.assert_close(y.float(), ref, **TOL)
        if rows <= 4:
            torch.testing.assert_close(y, ext().gemv_w4_norm(x, a, gam, 1e-5, ww[0], ww[1], epi)[1], **TOL_BF)
        assert torch.equal(ext().skinny_w4_norm(x, a, gam, 1e-5, ww[0], ww[1], epi)[1], y)


def test_skinny_w4_rejects_and_dispatch(monkeypatch):
    c, s, wd = _weights(32, 64)
    x = _x(17, 64)
    ok = ext().skinny_w4_ok
    assert ok(x[:16], c, s) and ok(x[:1], c, s)
    assert not ok(x, c, s)  # 17 rows
    assert not ok(x[:1].half(), c, s) and not ok(x[:1].float(), c, s)
    wide = torch.zeros(32, 64, device=DEV, dtype=torch.uint8)
    assert not ok(x[:1], wide[:, :32], s)  # code rows not whole rows of the buffer
    sw = torch.zeros(32, 4, device=DEV, dtype=torch.uint8)
    assert not ok(x[:1], c, sw[:, :2])  # non-contiguous scale rows
    assert not ok(_x(1, 48), torch.zeros(32, 24, device=DEV, dtype=torch.uint8), torch.zeros(32, 1, device=DEV, dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        ext().skinny_w4(x, c, s)
    # ops.gemm.linear inside skinny_gemm(): 9 rows of a quantised parameter run skinny_w4
    p = torch.nn.Parameter(wd.clone(), requires_grad=False)
    quant.quantize_parameters([p], "mxfp4")
    calls = []
    real = ext().skinny_w4
    monkeypatch.setattr(ext(), "skinny_w4", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with gemm.skinny_gemm():
        y = gemm.linear(x[:9].view(9, 1, 64), p)
    monkeypatch.undo()
    assert calls == [1] and torch.equal(y.view(9, 32), ext().skinny_w4(x[:9], c, s))
