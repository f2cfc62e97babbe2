"""The wide MFMA decode kernel for 1 <= M <= 64 rows (``csrc/kernels/wide.hip``, ``ext().wide*``) (GPU only).

Inputs and tolerances are those of ``tests/test_skinny_gpu.py`` (``TOL`` 2e-2 against float math, ``TOL_BF`` 3e-2 kernel
against kernel).  Launch rules (``wide_rules``): at most 2048 weight tiles: one tile per wave and K split across workgroups into slices of
whole chunks, merged by a second launch (136 x 528: three slices, an N tail, a K tail) -- or not split when K is one
chunk (77 x 64); above 2048 weight tiles two weight tiles per wave and no split (32781 x 288: N tail of 13, K tail).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import gemm, quant  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402
import test_skinny_gpu as sk  # noqa: E402
import test_skinny_mxfp4_gpu as sk4  # noqa: E402
from test_skinny_gpu import BF, DEV, TOL, TOL_BF, _rms, _swiglu_ref, _t, _x  # noqa: E402

FORMATS = ["bf16", "fp16", "fp8", "mxfp4"]
SUFFIX = {"bf16": "", "fp16": "", "fp8": "_w8", "mxfp4": "_w4"}
WIDE_RULE_SHAPES = [(136, 528), (77, 64), (32781, 288)]


def _shape(fmt, N, K):
    return N, (544 if K == 528 and fmt == "mxfp4" else K)  # (MXFP4 needs K % 32)


def _weights(fmt, N, K, seed=0):
    """(weight arguments of a call, the weight's values as float)."""
    w = (sk4 if fmt == "mxfp4" else sk)._weights(N, K, seed)
    wd = w[2].half() if fmt == "fp16" else w[2]
    return ((wd,) if fmt in ("bf16", "fp16") else (w[0], w[1])), wd.float()


def _fn(fmt, suffix, kern="wide"):
    return getattr(ext(), kern + SUFFIX[fmt] + suffix)


def _operands(fmt, M, N, K):
    gam = _t(fmt, (1 + 0.1 * _x(1, K, seed=3).float()).to(BF).view(K))
    return _t(fmt, _x(M, K)), _t(fmt, _x(M, K, seed=2)), _t(fmt, _x(M, N, seed=4)), gam


def _all_forms(fmt, x, add, res, gam, w, w2, kern="wide", bias=None):
    """Every form's output: w [N, K] for plain / RES / NORM, w2 [2N, K] for the SwiGLU forms."""
    norm = _fn(fmt, "_norm", kern)
    s0, n0 = norm(x, None, gam, 1e-5, *w, 0)
    s1, n1 = norm(x, add, gam, 1e-5, *w, 0)
    s2, n2 = norm(x, add, gam, 1e-5, *w2, 2)
    assert s0.data_ptr() == x.data_ptr()
    return {"plain": _fn(fmt, "", kern)(x, *w, None), "bias": _fn(fmt, "", kern)(x, *w, bias),
            "res": _fn(fmt, "_residual", kern)(x, *w, res), "swiglu": _fn(fmt, "_swiglu", kern)(x, *w2),
            "norm": n0, "add_norm": n1, "add_norm_s": s1, "add_norm_swiglu": n2, "add_norm_swiglu_s": s2,
            "norm_swiglu": norm(x, None, gam, 1e-5, *w2, 2)[1]}


@pytest.mark.parametrize("N,K", WIDE_RULE_SHAPES)
@pytest.mark.parametrize("M", [1, 17, 32, 49, 64])
@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_forms_against_float_math(fmt, M, N, K):
    N, K = _shape(fmt, N, K)
    (w, wf), (w2, wf2) = _weights(fmt, N, K), _weights(fmt, 2 * N, K, seed=5)
    x, add, res, gam = _operands(fmt, M, N, K)
    bias = _t(fmt, _x(1, N, seed=6).view(N))
    assert _fn(fmt, "_ok")(x, *w) and _fn(fmt, "_norm_ok")(x, *w, gam)
    got = _all_forms(fmt, x, add, res, gam, w, w2, bias=bias)
    again = _all_forms(fmt, x, add, res, gam, w, w2, bias=bias)
    s = (x.float() + add.float()).to(x.dtype)  # rnd(x + add)
    xf, n0, n1 = x.float(), _rms(x, gam), _rms(s, gam)
    want = {"plain": xf @ wf.t(), "bias": xf @ wf.t() + bias.float(),
            "res": (xf @ wf.t()).to(x.dtype).float() + res.float(), "swiglu": _swiglu_ref(xf, wf2),
            "norm": n0 @ wf.t(), "add_norm": n1 @ wf.t(), "add_norm_swiglu": _swiglu_ref(n1, wf2),
            "norm_swiglu": _swiglu_ref(n0, wf2)}
    for name, y in got.items():
        assert torch.equal(y, again[name]), name  # deterministic
        if name.endswith("_s"):
            assert torch.equal(y, s), name
        else:
            assert y.shape == (M, N) and y.dtype == x.dtype
            torch.testing.assert_close(y.float(), want[name], **TOL, msg=lambda m, name=name: f"{name}: {m}")


@pytest.mark.parametrize("N,K", WIDE_RULE_SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_batch_invariance(fmt, N, K):
    """Row m of the M-row call (M = 64, 37) is bitwise the 1-row call on it; row 0 does not change when the others do."""
    N, K = _shape(fmt, N, K)
    w, w2 = _weights(fmt, N, K)[0], _weights(fmt, 2 * N, K, seed=5)[0]
    x, add, res, gam = _operands(fmt, 64, N, K)
    single = [_all_forms(fmt, x[m: m + 1], add[m: m + 1], res[m: m + 1], gam, w, w2) for m in range(64)]
    for M in (64, 37):
        full = _all_forms(fmt, x[:M].clone(), add[:M].clone(), res[:M].clone(), gam, w, w2)
        for name, y in full.items():
            assert y.shape[0] == M
            for m in range(M):
                assert torch.equal(y[m: m + 1], single[m][name]), (name, M, m)
    x2, add2 = x.clone(), add.clone()
    x2[1:] = _t(fmt, _x(63, K, seed=9) * 3)
    add2[1:] = _t(fmt, _x(63, K, seed=10))
    for name, y in _all_forms(fmt, x2, add2, res, gam, w, w2).items():
        assert torch.equal(y[:1], single[0][name]), name


@pytest.mark.parametrize("M", [17, 33, 63])
@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_padding_rows_are_not_read(fmt, M):
    """x / add / res are the first M rows of 64-row buffers whose other rows are NaN."""
    N, K = _shape(fmt, 136, 528)
    w, w2 = _weights(fmt, N, K)[0], _weights(fmt, 2 * N, K, seed=5)[0]
    x, add, res, gam = _operands(fmt, M, N, K)
    want = _all_forms(fmt, x, add, res, gam, w, w2)

    def padded(t):
        buf = torch.full((64, t.shape[1]), float("nan"), device=DEV, dtype=t.dtype)
        buf[:M] = t
        return buf[:M]

    got = _all_forms(fmt, padded(x), padded(add), padded(res), gam, w, w2)
    for name in want:
        assert bool(torch.isfinite(got[name].float()).all()), name
        assert torch.equal(got[name], want[name]), name


@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_continues_skinny(fmt):
    N, K = _shape(fmt, 136, 528)
    w, w2 = _weights(fmt, N, K)[0], _weights(fmt, 2 * N, K, seed=5)[0]
    ops = _operands(fmt, 16, N, K)
    wide, skinny = _all_forms(fmt, *ops, w, w2), _all_forms(fmt, *ops, w, w2, kern="skinny")
    for name in wide:
        torch.testing.assert_close(wide[name], skinny[name], **TOL_BF)


@pytest.mark.parametrize("fmt", ["bf16", "fp8", "mxfp4"])
def test_wide_rejections_and_dispatch(fmt, monkeypatch):
    N, K = 77, 64
    w = _weights(fmt, N, K)[0]
    x = _x(65, K)
    assert _fn(fmt, "_ok")(x[:64], *w) and not _fn(fmt, "_ok")(x[:0], *w) and not _fn(fmt, "_ok")(x, *w)
    for bad in (x[:0], x):  # M = 0, M = 65
        with pytest.raises(RuntimeError):
            _fn(fmt, "")(bad, *w)
    p = torch.nn.Parameter(sk._weights(N, K)[2].clone() if fmt != "mxfp4" else sk4._weights(N, K)[2].clone(),
                           requires_grad=False)
    if fmt != "bf16":
        quant.quantize_parameters([p], "mxfp4" if fmt == "mxfp4" else "fp8_e4m3")
    calls = []
    for kern in ("wide", "skinny"):
        real = _fn(fmt, "", kern)
        monkeypatch.setattr(ext(), kern + SUFFIX[fmt], lambda *a, _r=real, _k=kern, **k: (calls.append(_k), _r(*a, **k))[1])
    with gemm.skinny_gemm(wide=True):
        assert gemm.decode_rows_limit() == 64
        for rows in (17, 64, 16, 65):
            y = gemm.linear(x[:rows].view(rows, 1, K), p)
            if rows != 65:
                assert torch.equal(y.view(rows, N), _fn(fmt, "", "wide" if rows > 16 else "skinny")(x[:rows], *w))
        assert calls == ["wide", "wide", "wide", "wide", "skinny", "skinny"]  # (each once by linear, once above)
    calls.clear()
    with gemm.skinny_gemm():
        gemm.linear(x[:17].view(17, 1, K), p)  # the library path, as before
    assert calls == [] and gemm.decode_rows_limit() == 4
