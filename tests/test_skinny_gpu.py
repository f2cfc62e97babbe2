"""The MFMA weight-streaming decode kernel for 1 <= M <= 16 rows (``csrc/kernels/skinny.hip``, ``ext().skinny*``) (GPU only).

Inputs and tolerances are those of ``tests/test_gemv_fp8_gpu.py``: x is N(0,1), w is N(0,1)/sqrt(K) (for FP8: before
quantisation, and the dense kernels run on the dequantised values), ``TOL`` 2e-2 against float math on the bf16 / fp16 /
dequantised values, ``TOL_BF`` 3e-2 against the GEMV kernel where M <= 4.

Launch rules (``skinny_rules``): the workgroup's four waves split K while the layer has at most 2048 weight tiles of 16
rows, one output tile per wave below 512 tiles and two from there; above 2048 weight tiles a wave owns its tiles' whole
K.  ``RULE_SHAPES`` has one (N, K) per rule.
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
FORMATS = ["bf16", "fp16", "fp8"]
# K split + one tile per wave; K split + two tiles per wave; no K split (2049 tiles, N tail of 13)
RULE_SHAPES = [(136, 528), (8200, 64), (32781, 64)]


def _quantised(N, K, seed=0, up_scale=None):
    """(q, scale, dequantised bf16 weight) of a seeded N(0,1)/sqrt(K) matrix (rows N/2.. times up_scale)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)
    if up_scale is not None:
        w[N // 2:] *= up_scale
    q, s = quant.quantize_rows_fp8(w.to(BF))
    return q, s, quant.dequantize_rows_fp8(q, s, BF)


def _x(M, K, seed=1):
    return torch.randn(M, K, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(BF)


def _t(fmt, t):
    """An activation-typed tensor in the format's activation type."""
    return None if t is None else (t.half() if fmt == "fp16" else t)


def _w(fmt, w):
    """The weight arguments of a call: (W,) dense, (q, scale) FP8."""
    q, s, wd = w
    return (q, s) if fmt == "fp8" else (wd.half(),) if fmt == "fp16" else (wd,)


def _wf(fmt, w):
    """The weight's values as float."""
    return (w[2].half() if fmt == "fp16" else w[2]).float()


def _fn(fmt, suffix, gemv=False):
    return getattr(ext(), ("gemv" if gemv else "skinny") + ("_w8" if fmt == "fp8" else "") + suffix)


def _norm(fmt, x, add, gam, w, epi, gemv=False):
    return _fn(fmt, "_norm", gemv)(_t(fmt, x), _t(fmt, add), _t(fmt, gam), 1e-5, *_w(fmt, w), epi)


def _rms(s, gam):
    s = s.float()
    return s * torch.rsqrt(s.pow(2).mean(-1, keepdim=True) + 1e-5) * gam.float()


def _swiglu_ref(n, wf):
    F = wf.shape[0] // 2
    return torch.nn.functional.silu(n @ wf[:F].t()) * (n @ wf[F:].t())


_CACHE = {}


def _weights(N, K, seed=0, up_scale=None):
    key = (N, K, seed, up_scale)
    if key not in _CACHE:
        _CACHE[key] = _quantised(N, K, seed, up_scale)
    return _CACHE[key]


PLAIN_SHAPES = [(5, 16), (77, 64), (1003, 208), (64, 4112), (263, 528)]


@pytest.mark.parametrize("fmt,N,K", [(f, n, k) for f in FORMATS for n, k in PLAIN_SHAPES]
                         + [(f, 77, k) for f in FORMATS[:2] for k in (8, 24)])  # (FP8 pieces are 16 codes)
@pytest.mark.parametrize("M", [1, 2, 5, 15, 16])
def test_skinny_plain(fmt, M, N, K):
    """Plain (+ bias): the N tail, the K tails of 8 / 16 / 24 and a single partial k-step; a row-strided x and a
    row-strided weight / code view at byte offset 32; every call twice."""
    if fmt == "fp8":
        w = _weights(N, K)
    else:  # (quantize_rows_fp8 wants K % 16; the dense K = 8 / 24 cases take plain bf16 values)
        g = torch.Generator(device=DEV).manual_seed(0)
        w = (None, None, (torch.randn(N, K, device=DEV, generator=g) / math.sqrt(K)).to(BF))
    x = _t(fmt, _x(M, K))
    fn, ok = _fn(fmt, ""), _fn(fmt, "_ok")
    for bias in (None, _t(fmt, _x(1, N, seed=2).view(N))):
        ref = x.float() @ _wf(fmt, w).t() + (bias.float() if bias is not None else 0.0)
        assert ok(x, *_w(fmt, w))
        y = fn(x, *_w(fmt, w), bias)
        assert y.shape == (M, N) and y.dtype == x.dtype
        torch.testing.assert_close(y.float(), ref, **TOL)
        assert torch.equal(fn(x, *_w(fmt, w), bias), y)  # deterministic
        if M <= 4:
            torch.testing.assert_close(y, _fn(fmt, "", gemv=True)(x, *_w(fmt, w), bias), **TOL_BF)
        # a row-strided view of a wider weight / code buffer, starting at byte offset 32
        wa = _w(fmt, w)
        pad = 32 // wa[0].element_size()
        wide = torch.zeros(N, K + 2 * pad, device=DEV, dtype=torch.uint8 if fmt == "fp8" else wa[0].dtype)
        wide[:, pad: pad + K] = wa[0].view(wide.dtype)
        wv = wide[:, pad: pad + K].view(wa[0].dtype)
        assert wv.stride(0) == K + 2 * pad and ok(x, wv, *wa[1:])
        assert torch.equal(fn(x, wv, *wa[1:], bias), y)
        # a row-strided x
        xw = torch.zeros(M, K + 24, device=DEV, dtype=x.dtype)
        xw[:, 8: 8 + K] = x
        xs = xw[:, 8: 8 + K]
        assert ok(xs, *wa) and torch.equal(fn(xs, *wa, bias), y)


def _all_forms(fmt, x, add, res, gam, w, w2):
    """Every form's output on these operands: w [N, K] for plain / RES / NORM, w2 [2N, K] for the SwiGLU forms."""
    xa = _t(fmt, x)
    s0, n0 = _norm(fmt, x, None, gam, w, 0)
    s1, n1 = _norm(fmt, x, add, gam, w, 0)
    s2, n2 = _norm(fmt, x, add, gam, w2, 2)
    assert s0.data_ptr() == xa.data_ptr() or torch.equal(s0, xa)
    return {
        "plain": _fn(fmt, "")(xa, *_w(fmt, w), None),
        "res": _fn(fmt, "_residual")(xa, *_w(fmt, w), _t(fmt, res)),
        "swiglu": _fn(fmt, "_swiglu")(xa, *_w(fmt, w2)),
        "norm": n0, "add_norm": n1, "add_norm_s": s1, "add_norm_swiglu": n2, "add_norm_swiglu_s": s2,
        "norm_swiglu": _norm(fmt, x, None, gam, w2, 2)[1],
    }


@pytest.mark.parametrize("N,K", RULE_SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_skinny_batch_invariance(fmt, N, K):
    """Row m of the M-row call is bitwise the 1-row call on x[m : m + 1], for M = 16 and M = 7, every form, every
    launch rule: the rules do not depend on M and no row's arithmetic depends on another row."""
    w, w2 = _weights(N, K), _weights(2 * N, K, seed=5)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    x, add, res = _x(16, K), _x(16, K, seed=2), _x(16, N, seed=4)
    single = [_all_forms(fmt, x[m: m + 1], add[m: m + 1], res[m: m + 1], gam, w, w2) for m in range(16)]
    for M in (16, 7):
        # (contiguous copies of exactly M rows: nothing behind them belongs to the call)
        full = _all_forms(fmt, x[:M].clone(), add[:M].clone(), res[:M].clone(), gam, w, w2)
        for name, y in full.items():
            assert y.shape[0] == M
            for m in range(M):
                assert torch.equal(y[m: m + 1], single[m][name]), (name, M, m)
    # ... and whatever the other rows hold
    x2, add2 = x.clone(), add.clone()
    x2[1:] = _x(15, K, seed=9) * 3
    add2[1:] = _x(15, K, seed=10)
    other = _all_forms(fmt, x2, add2, res, gam, w, w2)
    for name, y in other.items():
        assert torch.equal(y[:1], single[0][name]), name


@pytest.mark.parametrize("M", [1, 7, 15])
@pytest.mark.parametrize("fmt", FORMATS)
def test_skinny_padding_rows_are_not_read(fmt, M):
    """x / add / res are the first M rows of 16-row buffers whose other rows are NaN: the outputs are finite and equal
    those of M-row operands.  (Allocated memory only: a kernel that did read them would turn rows non-finite.)"""
    N, K = 136, 528
    w, w2 = _weights(N, K), _weights(2 * N, K, seed=5)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    x, add, res = _t(fmt, _x(M, K)), _t(fmt, _x(M, K, seed=2)), _t(fmt, _x(M, N, seed=4))  # (_t is idempotent)
    want = _all_forms(fmt, x, add, res, gam, w, w2)

    def padded(t):
        buf = torch.full((16, t.shape[1]), float("nan"), device=DEV, dtype=t.dtype)
        buf[:M] = t
        return buf[:M]

    got = _all_forms(fmt, padded(x), padded(add), padded(res), gam, w, w2)
    for name in want:
        assert bool(torch.isfinite(got[name].float()).all()), name
        assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("rows", [2, 9, 16])
@pytest.mark.parametrize("fmt", FORMATS)
def test_skinny_epilogues(fmt, rows):
    """SwiGLU over [gate; up] with F = 136 and F = 263 (odd), the up half on 16x larger scales; down + residual with
    N = 136 and N = 528, and with the other two launch rules."""
    K = 528
    x = _t(fmt, _x(rows, K))
    for F in (136, 263):
        w = _weights(2 * F, K, seed=rows, up_scale=16.0)
        assert float(w[1][F:].min()) >= 4 * float(w[1][:F].max())
        h = _fn(fmt, "_swiglu")(x, *_w(fmt, w))
        assert h.shape == (rows, F)
        torch.testing.assert_close(h.float(), _swiglu_ref(x.float(), _wf(fmt, w)), **TOL)
        assert torch.equal(_fn(fmt, "_swiglu")(x, *_w(fmt, w)), h)
        if rows <= 4:
            torch.testing.assert_close(h, _fn(fmt, "_swiglu", gemv=True)(x, *_w(fmt, w)), **TOL_BF)
    for N, Kr in [(136, K), (528, K)] + RULE_SHAPES[1:]:
        xr = _t(fmt, _x(rows, Kr))
        wo = _weights(N, Kr, seed=7 + N)
        res = _t(fmt, _x(rows, N, seed=4))
        y = _fn(fmt, "_residual")(xr, *_w(fmt, wo), res)
        ref = (xr.float() @ _wf(fmt, wo).t()).to(xr.dtype).float() + res.float()
        torch.testing.assert_close(y.float(), ref, **TOL)
        assert torch.equal(_fn(fmt, "_residual")(xr, *_w(fmt, wo), res), y)
        if rows <= 4:
            torch.testing.assert_close(y, _fn(fmt, "_residual", gemv=True)(xr, *_w(fmt, wo), res), **TOL_BF)


@pytest.mark.parametrize("rows", [2, 9, 16])
@pytest.mark.parametrize("N", [264, 263])
@pytest.mark.parametrize("K", [528, 4112])
@pytest.mark.parametrize("fmt", FORMATS)
def test_skinny_norm(fmt, rows, N, K):
    """RMSNorm prologue with and without the residual add, epilogue 0 and 2: s is bit-identical to add_rms_norm's (x
    itself without add), y matches float math and, at rows <= 4, gemv_norm."""
    F = N // 2 if N % 2 == 0 else N
    x, add = _x(rows, K), _x(rows, K, seed=2)
    gam = (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K)
    w, w2 = _weights(N, K), _weights(2 * F, K, seed=5)
    xa, ga = _t(fmt, x), _t(fmt, gam)
    assert _fn(fmt, "_norm_ok")(xa, *_w(fmt, w), ga)
    wf, wf2 = _wf(fmt, w), _wf(fmt, w2)
    s_ref, _ = norm_ops.add_rms_norm(_t(fmt, add), xa, ga, 1e-5)  # the layer's order: residual + attention output
    for a, s_want in ((None, xa), (add, s_ref)):
        for epi, ww, ref in ((0, w, _rms(s_want, ga) @ wf.t()), (2, w2, _swiglu_ref(_rms(s_want, ga), wf2))):
            s, y = _norm(fmt, xa, a, gam, ww, epi)  # (_t leaves the converted xa as it is)
            if a is None:
                assert s.data_ptr() == xa.data_ptr()
            assert torch.equal(s, s_want)
            torch.testing.assert_close(y.float(), ref, **TOL)
            assert torch.equal(_norm(fmt, x, a, gam, ww, epi)[1], y)  # deterministic
            if rows <= 4:
                torch.testing.assert_close(y, _norm(fmt, x, a, gam, ww, epi, gemv=True)[1], **TOL_BF)


@pytest.mark.parametrize("K", [64, 4096])
@pytest.mark.parametrize("M", [3, 12])
def test_skinny_w8_row_scales_and_subnormals(K, M):
    """The CPU test's matrix: rows scaled by 2^(i % 12 - 6), a zero row, outlier rows whose other codes are small,
    subnormal (exponent 0) or zero."""
    w = make_weight(K).to(DEV)
    q, s = quant.quantize_rows_fp8(w)
    wd = quant.dequantize_rows_fp8(q, s, BF)
    assert len(set(s.tolist())) >= 12
    x = _x(M, K)
    y = ext().skinny_w8(x, q, s)
    torch.testing.assert_close(y.float(), x.float() @ wd.float().t(), **TOL)
    assert bool((y[:, 1] == 0).all())
    # the subnormal codes alone (the outlier column removed from the dot product), in the row's own units
    col = K // 5
    xz = x.clone()
    xz[:, col] = 0
    got = ext().skinny_w8(xz, q, s)[:, 4].float() / s[4]
    want = (xz.float() @ wd[4].float()) / s[4]
    torch.testing.assert_close(got, want, **TOL)
    assert float(want.abs().max()) > 0


def test_skinny_rejects_unsupported():
    q, s, wd = _quantised(32, 64)
    x = _x(17, 64)
    ok, ok8 = ext().skinny_ok, ext().skinny_w8_ok
    assert ok(x[:16], wd) and ok8(x[:16], q, s) and ok(x[:1].half(), wd.half()) and ok8(x[:1], q.view(torch.uint8), s)
    gam = torch.ones(64, device=DEV, dtype=BF)
    assert ext().skinny_norm_ok(x[:9], wd, gam) and ext().skinny_w8_norm_ok(x[:9], q, s, gam)
    bad = [
        (x[:0], wd), (x, wd),  # M = 0, M = 17
        (x[:2, :12], wd[:, :12]),  # K % 8
        (x[:2].float(), wd.float()), (x[:2].half(), wd), (x[:2], wd.half()),  # dtypes
    ]
    xw = torch.zeros(2, 64 + 8, device=DEV, dtype=BF)
    bad.append((xw[:, 4:68], wd))  # misaligned base (byte offset 8)
    for a, b in bad:
        assert not ok(a, b)
        with pytest.raises(RuntimeError):
            ext().skinny(a, b)
        with pytest.raises(RuntimeError):
            ext().skinny_residual(a, b, torch.zeros(a.shape[0], b.shape[0], device=DEV, dtype=a.dtype))
    wide = torch.zeros(32, 64 + 16, device=DEV, dtype=torch.uint8).view(torch.float8_e4m3fn)
    bad8 = [
        (x[:0], q, s), (x, q, s),  # M = 0, M = 17
        (x[:2, :56], q[:, :56], s),  # K % 16
        (x[:2], wide[:, 8:72], s),  # misaligned base (byte offset 8)
        (x[:2].half(), q, s), (x[:2], q.view(torch.uint8).to(torch.int8), s), (x[:2], q, s.double()),  # dtypes
        (x[:2], q, s[:31]),
    ]
    for a, b, c in bad8:
        assert not ok8(a, b, c)
        with pytest.raises(RuntimeError):
            ext().skinny_w8(a, b, c)
    with pytest.raises(RuntimeError):
        ext().skinny_swiglu(x[:2], wd[:31])  # an odd number of [gate; up] rows
    assert not ext().skinny_norm_ok(x[:2], wd, gam[:48]) and not ext().skinny_norm_ok(x, wd, gam)
    assert not ext().skinny_w8_norm_ok(x[:2], q, s, gam.float()) and not ext().skinny_w8_norm_ok(x, q, s, gam)
    with pytest.raises(RuntimeError):
        ext().skinny_norm(x, None, gam, 1e-5, wd, 0)
    with pytest.raises(RuntimeError):
        ext().skinny_w8_norm(x[:2], None, gam[:48], 1e-5, q, s, 0)


@pytest.mark.parametrize("fp8", [False, True])
def test_linear_dispatch(fp8, monkeypatch):
    """Inside ops.gemm.skinny_gemm() linear() on 9 rows calls skinny (skinny_w8 on a quantised parameter) exactly once
    and returns the direct call's result; outside the context the same call does not."""
    N, K = 77, 64
    q, s, wd = _weights(N, K)
    x = _x(9, K)
    p = torch.nn.Parameter(wd.clone(), requires_grad=False)
    if fp8:
        quant.quantize_parameters([p])
    name = "skinny_w8" if fp8 else "skinny"
    want = ext().skinny_w8(x, q, s) if fp8 else ext().skinny(x, wd)
    calls = []
    real = getattr(ext(), name)
    monkeypatch.setattr(ext(), name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert gemm.decode_rows_limit() == 4
    y_out = gemm.linear(x.view(9, 1, K), p)
    assert calls == []
    with gemm.skinny_gemm():
        assert gemm.decode_rows_limit() == 16
        y_in = gemm.linear(x.view(9, 1, K), p)
        assert calls == [1]
        gemm.linear(_x(17, K).view(17, 1, K), p)  # above 16 rows: the library path
        small = gemm.linear(x[:1].view(1, 1, K), p)  # below SKINNY_MIN_ROWS: the GEMV
        assert calls == [1]
    monkeypatch.undo()
    assert gemm.decode_rows_limit() == 4
    assert y_in.shape == (9, 1, N) and torch.equal(y_in.view(9, N), want)
    torch.testing.assert_close(y_out.view(9, N), want, **TOL_BF)
    gv = ext().gemv_w8(x[:1], q, s) if fp8 else ext().gemv(x[:1], wd)
    assert gemm.SKINNY_MIN_ROWS > 1 and torch.equal(small.view(1, N), gv)
