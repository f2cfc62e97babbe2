"""FP8-weight decode GEMV (the FP8 weight format of ``csrc/kernels/gemv.hip``) against float math on the DEQUANTISED weights (GPU only).

The FP8 copy is an exact encoding of the bf16 values it was made from (``ops/quant.py``), so the tolerances are the
bf16 GEMV's own -- 2e-2 against float math (``test_gemv``), 3e-2 against the bf16 kernel on the same values
(``test_gemv_norm_fused``) -- with no quantisation term.  x is N(0,1), w is N(0,1)/sqrt(K) before quantisation.
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
from tests.test_quant_cpu import make_weight  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
TOL = dict(atol=2e-2, rtol=2e-2)
TOL_BF = dict(atol=3e-2, rtol=3e-2)


def _quantised(N, K, seed=0):
    """(q, scale, dequantised bf16 weight) of a seeded N(0,1)/sqrt(K) matrix."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(BF)
    q, s = quant.quantize_rows_fp8(w)
    return q, s, quant.dequantize_rows_fp8(q, s, BF)


def _x(M, K, seed=1):
    return torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(BF)


@pytest.mark.parametrize("M,N,K", [(1, 5, 16), (3, 77, 64), (2, 1003, 208), (1, 64, 4112), (2, 2064, 4112),
                                   (4, 256, 1024)])
@pytest.mark.parametrize("bias", [False, True])
def test_gemv_w8(M, N, K, bias, monkeypatch):
    """Plain (+ bias): through ops.gemm.linear on a quantised parameter (which must route to the FP8 kernel) and
    through ext().gemv_w8; a row-strided code view and a row-strided x."""
    q, s, wd = _quantised(N, K)
    x = _x(M, K)
    b = _x(1, N, seed=2).view(N) if bias else None
    ref = x.float() @ wd.float().t() + (b.float() if bias else 0.0)
    assert ext().gemv_w8_ok(x, q, s)
    y = ext().gemv_w8(x, q, s, b)
    torch.testing.assert_close(y.float(), ref, **TOL)
    torch.testing.assert_close(y, ext().gemv(x, wd, b), **TOL_BF)
    assert torch.equal(ext().gemv_w8(x, q, s, b), y)  # deterministic
    # through linear() on a quantised parameter
    p = torch.nn.Parameter(wd.clone(), requires_grad=False)
    quant.quantize_parameters([p])
    assert torch.equal(p.data, wd)
    calls = []
    real = ext().gemv_w8
    monkeypatch.setattr(ext(), "gemv_w8", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    yl = gemm.linear(x.view(M, 1, K), p, b)
    monkeypatch.undo()
    assert calls == [1] and torch.equal(yl.view(M, N), y)
    # a row-strided view of a wider code buffer, starting at byte offset 32
    wide = torch.zeros(N, K + 64, device=DEV, dtype=torch.uint8)
    wide[:, 32 : 32 + K] = q.view(torch.uint8)
    qv = wide[:, 32 : 32 + K].view(torch.float8_e4m3fn)
    assert qv.stride(0) == K + 64 and ext().gemv_w8_ok(x, qv, s)
    assert torch.equal(ext().gemv_w8(x, qv, s, b), y)
    # a row-strided x
    xw = torch.zeros(M, K + 24, device=DEV, dtype=BF)
    xw[:, 8 : 8 + K] = x
    xs = xw[:, 8 : 8 + K]
    assert ext().gemv_w8_ok(xs, q, s) and torch.equal(ext().gemv_w8(xs, q, s, b), y)


@pytest.mark.parametrize("K", [64, 4096])
@pytest.mark.parametrize("M", [1, 3])
def test_gemv_w8_row_scales_and_subnormals(K, M):
    """The CPU test's matrix: rows scaled by 2^(i % 12 - 6), a zero row, outlier rows whose other codes are small,
    subnormal (exponent 0) or zero.  A kernel that ignores or mis-indexes scale, or mis-decodes exponent-0 codes, fails."""
    w = make_weight(K).to(DEV)
    q, s = quant.quantize_rows_fp8(w)
    wd = quant.dequantize_rows_fp8(q, s, BF)
    assert len(set(s.tolist())) >= 12
    x = _x(M, K)
    y = ext().gemv_w8(x, q, s)
    torch.testing.assert_close(y.float(), x.float() @ wd.float().t(), **TOL)
    assert bool((y[:, 1] == 0).all())
    # the subnormal codes alone (the outlier column removed from the dot product): absolute values ~2^-14 of the
    # outlier's, so they are compared in the row's own units
    col = K // 5
    xz = x.clone()
    xz[:, col] = 0
    got = ext().gemv_w8(xz, q, s)[:, 4].float() / s[4]
    want = (xz.float() @ wd[4].float()) / s[4]
    torch.testing.assert_close(got, want, **TOL)
    assert float(want.abs().max()) > 0


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
def test_gemv_w8_epilogues(rows):
    """SwiGLU over [gate; up] (the halves on different scales) and down + residual: against float math and against
    the bf16 kernels on the dequantised weights."""
    F, K = 136, 528
    g = torch.Generator(device=DEV).manual_seed(rows)
    w = torch.randn(2 * F, K, device=DEV, generator=g) / math.sqrt(K)
    w[F:] *= 16  # the up half on its own scales: taking the gate row's scale for the up row is off by 4x or more
    q, s = quant.quantize_rows_fp8(w.to(BF))
    assert float(s[F:].min()) >= 4 * float(s[:F].max())
    wd = quant.dequantize_rows_fp8(q, s, BF)
    x = _x(rows, K)
    h = ext().gemv_w8_swiglu(x, q, s)
    hf = torch.nn.functional.silu(x.float() @ wd[:F].float().t()) * (x.float() @ wd[F:].float().t())
    torch.testing.assert_close(h.float(), hf, **TOL)
    torch.testing.assert_close(h, ext().gemv_swiglu(x, wd), **TOL_BF)
    assert torch.equal(ext().gemv_w8_swiglu(x, q, s), h)
    # residual epilogue over K = 528: N = 136 takes the K-split form (N <= 8192 and K >= 2 N), N = 528 one wave per row
    for N in (F, K):
        qo, so, wo = _quantised(N, K, seed=7 + N)
        res = _x(rows, N, seed=4)
        y = ext().gemv_w8_residual(x, qo, so, res)
        torch.testing.assert_close(y.float(), (x.float() @ wo.float().t()).to(BF).float() + res.float(), **TOL)
        torch.testing.assert_close(y, ext().gemv_residual(x, wo, res), **TOL_BF)
        assert torch.equal(ext().gemv_w8_residual(x, qo, so, res), y)


@pytest.mark.parametrize("rows", [1, 2, 4])
@pytest.mark.parametrize("N", [264, 263])
@pytest.mark.parametrize("K", [528, 4112])
def test_gemv_w8_norm(rows, N, K):
    """RMSNorm prologue (with and without the residual add; two rows per wave for even N, one for odd): s is
    bit-identical to add_rms_norm's, y matches float math, plain and SwiGLU."""
    F = N // 2 if N % 2 == 0 else N  # SwiGLU over [2F, K]: F = 132 (two rows per wave) or 263 (one)
    x = _x(rows, K)
    add = _x(rows, K, seed=2)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    q, s, wd = _quantised(N, K)
    q2, s2, wd2 = _quantised(2 * F, K, seed=5)
    assert ext().gemv_w8_norm_ok(x, q, s, gam)

    def rms(t):
        t = t.float()
        return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5) * gam.float()

    def swiglu(n):
        return torch.nn.functional.silu(n @ wd2[:F].float().t()) * (n @ wd2[F:].float().t())

    so, y = ext().gemv_w8_norm(x, None, gam, 1e-5, q, s, 0)
    assert so.data_ptr() == x.data_ptr()
    torch.testing.assert_close(y.float(), rms(x) @ wd.float().t(), **TOL)
    torch.testing.assert_close(y, ext().gemv_norm(x, None, gam, 1e-5, wd, 0)[1], **TOL_BF)
    _, y2 = ext().gemv_w8_norm(x, None, gam, 1e-5, q2, s2, 2)
    torch.testing.assert_close(y2.float(), swiglu(rms(x)), **TOL)
    s_ref, _ = norm_ops.add_rms_norm(add, x, gam, 1e-5)  # the layer's order: residual + attention output
    sa, ya = ext().gemv_w8_norm(x, add, gam, 1e-5, q, s, 0)
    assert torch.equal(sa, s_ref)
    torch.testing.assert_close(ya.float(), rms(s_ref) @ wd.float().t(), **TOL)
    sb, yb = ext().gemv_w8_norm(x, add, gam, 1e-5, q2, s2, 2)
    assert torch.equal(sb, s_ref)
    torch.testing.assert_close(yb.float(), swiglu(rms(s_ref)), **TOL)
    torch.testing.assert_close(yb, ext().gemv_norm(x, add, gam, 1e-5, wd2, 2)[1], **TOL_BF)
    # deterministic
    for a, e, qq, ss, want in ((None, 0, q, s, y), (None, 2, q2, s2, y2), (add, 0, q, s, ya), (add, 2, q2, s2, yb)):
        assert torch.equal(ext().gemv_w8_norm(x, a, gam, 1e-5, qq, ss, e)[1], want)


def test_gemv_w8_rejects_unsupported():
    q, s, _ = _quantised(32, 64)
    x = _x(5, 64)
    ok = ext().gemv_w8_ok
    assert ok(x[:4], q, s) and ok(x[:1], q.view(torch.uint8), s)
    assert not ok(x, q, s)  # 5 rows
    assert not ok(x[:1, :56], q[:, :56], s)  # K % 16 (56 = 3.5 pieces), though the bf16 GEMV takes K % 8
    q136, s136, _ = _quantised(32, 136)
    assert not ok(_x(1, 136), q136, s136)  # (a 136-wide down projection stays on the bf16 kernel)
    wide = torch.zeros(32, 64 + 16, device=DEV, dtype=torch.uint8).view(torch.float8_e4m3fn)
    assert not ok(x[:1], wide[:, 8:72], s)  # misaligned base (byte offset 8)
    odd = torch.zeros(32, 64 + 8, device=DEV, dtype=torch.uint8).view(torch.float8_e4m3fn)
    assert not ok(x[:1], odd[:, :64], s)  # row stride 72 bytes
    assert not ok(x[:1], q, s[:31]) and not ok(x[:1], q, torch.cat([s, s]))  # scale of the wrong length
    assert not ok(x[:1], q, s.double()) and not ok(x[:1], q, s.to(BF))  # ... or dtype
    assert not ok(x[:1], q, torch.stack([s, s], dim=1)[:, 0])  # ... or strided
    assert not ok(x[:1].half(), q, s) and not ok(x[:1], q.view(torch.uint8).to(torch.int8), s)
    assert not ok(x[:1], q.cpu(), s) and not ok(x[:1], q, s.cpu())
    with pytest.raises(RuntimeError):
        ext().gemv_w8(x, q, s)
    with pytest.raises(RuntimeError):
        ext().gemv_w8_swiglu(x[:1], q[:31], s[:31])  # an odd number of [gate; up] rows
    gam = torch.ones(64, device=DEV, dtype=BF)
    assert ext().gemv_w8_norm_ok(x[:2], q, s, gam)
    assert not ext().gemv_w8_norm_ok(x[:2], q, s, gam[:48]) and not ext().gemv_w8_norm_ok(x[:2], q, s, gam.float())
