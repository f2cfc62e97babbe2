"""The quantised-weight prefill GEMM (``ext().qgemm_w8`` / ``qgemm_w4``, ``csrc/kernels/qgemm.hip``) against float64
math on the dequantised weights: every tile edge (M 1 / 64 / 65 / 129 / 200: both tile variants and their row tails;
N 40 / 128 / 136; K 32 / 64 / 96 / 352: below a chunk, a chunk, a chunk tail, chunks and a tail), bitwise on inputs whose
sums are exact, and the operand bounds.  ``TOL`` is ``tests/test_skinny_gpu.py``'s bound against float math."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import quant  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

TOL = dict(atol=2e-2, rtol=2e-2)
SHAPES = [(1, 40, 32), (64, 128, 64), (65, 136, 96), (129, 40, 352), (200, 136, 352), (129, 128, 64), (200, 128, 32),
          (64, 136, 352)]


def _copy(fmt, w):
    """(codes, scales, dequantised fp64) of the Gaussian matrix ``w``, on the CPU."""
    if fmt == "w8":
        q, s = quant.quantize_rows_fp8(w)
        return q.view(torch.uint8), s, quant.dequantize_rows_fp8(q, s, torch.float32).double()
    c, s = quant.quantize_rows_mxfp4(w)
    return c, s, quant.dequantize_rows_mxfp4(c, s, torch.float32).double()


def _run(fmt, x, c, s, bias=None, out=None):
    assert getattr(ext(), f"qgemm_{fmt}_ok")(x, c, s)
    return getattr(ext(), f"qgemm_{fmt}")(x, c, s, bias, out)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("fmt", ["w8", "w4"])
def test_against_float_math(fmt, M, N, K, bias):
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=g).bfloat16()
    c, s, deq = _copy(fmt, torch.randn(N, K, generator=g))
    b = torch.randn(N, generator=g).bfloat16() if bias else None
    ref = x.double() @ deq.t() + (b.double() if bias else 0)
    y = _run(fmt, x.cuda(), c.cuda(), s.cuda(), b.cuda() if bias else None)
    assert y.shape == (M, N) and y.dtype == torch.bfloat16
    torch.testing.assert_close(y.float().cpu(), ref.float(), **TOL)


@pytest.mark.parametrize("M,N,K", [(65, 136, 96), (40, 40, 352), (200, 128, 64)])
@pytest.mark.parametrize("fmt", ["w8", "w4"])
def test_bitwise_where_every_sum_is_exact(fmt, M, N, K):
    """x in -2..2, weights on the code grid: every partial sum is a whole number of the row's smallest code step (the
    e4m3 subnormal 2^-9, the e2m1 step 1/2, times the row's smallest scale) below 2^24 of them, so fp32 adds nothing
    and the result is the float64 product rounded once.  Scales run from the smallest the quantisers make (2^-100) to
    the largest (2^120 per row, 2^118 per block; those rows keep small codes so the sums stay finite in bf16)."""
    g = torch.Generator().manual_seed(K)
    x = torch.randint(-2, 3, (M, K), generator=g).bfloat16()
    exps = torch.tensor([-100, 0, 3, -7, 118])[torch.arange(N) % 5]
    if fmt == "w8":
        exps = torch.where(exps == 118, 120, exps)
        v = torch.randint(-8, 9, (N, K), generator=g).float()
        v[0, :4] = torch.tensor([2.0 ** -9, -3 * 2.0 ** -9, 2.0 ** -7, 1.0])  # subnormal codes
        v = torch.where((exps == 120)[:, None], v * 2.0 ** -6, v)
        c, s = v.to(torch.float8_e4m3fn).view(torch.uint8), torch.ldexp(torch.ones(N), exps)
        assert torch.equal(c.view(torch.float8_e4m3fn).float(), v)
        deq, step = quant.dequantize_rows_fp8(c, s, torch.float32).double(), s.double() * 2.0 ** -9
    else:
        nib = torch.randint(0, 16, (N, K), generator=g)
        nib = torch.where((exps == 118)[:, None], nib & 0b1011, nib)  # |code| <= 1.5
        nib = torch.where(nib == 8, 0, nib)  # (-0 is never produced)
        c = (nib[:, 0::2] | (nib[:, 1::2] << 4)).to(torch.uint8)
        be = torch.where(exps == 118, 116, exps)[:, None] + torch.arange(K // 32)[None, :] % 3
        s = (be + 127).to(torch.uint8)
        deq, step = quant.dequantize_rows_mxfp4(c, s, torch.float32).double(), torch.ldexp(torch.ones(N), be[:, 0]).double() / 2
    b = torch.randint(-3, 4, (N,), generator=g).bfloat16() * step.bfloat16() * 4
    ref = x.double() @ deq.t() + b.double()
    # the exactness condition, on the reference alone: sums of magnitudes (bias included) stay below 2^24 steps
    assert float(((x.abs().double() @ deq.abs().t() + b.abs().double()) / step).max()) < 2 ** 24 and torch.isfinite(ref.bfloat16()).all()
    y = _run(fmt, x.cuda(), c.cuda(), s.cuda(), b.cuda())
    assert torch.equal(y.cpu().view(torch.int16), ref.bfloat16().view(torch.int16))


@pytest.mark.parametrize("fmt", ["w8", "w4"])
def test_nothing_outside_the_operands_is_touched(fmt):
    M, N, K, LD = 70, 136, 96, 128
    g = torch.Generator().manual_seed(7)
    buf = torch.full((M + 5, LD), float("nan")).bfloat16().cuda()
    x = buf[3: 3 + M, :K]  # M rows at a row offset, stride 128 > K, NaN all around and behind the last row
    x.copy_(torch.randn(M, K, generator=g))
    c, s, deq = _copy(fmt, torch.randn(N, K, generator=g))
    c, s = c.cuda(), s.cuda()
    ref = x.double().cpu() @ deq.t()
    out = torch.full((M + 1, N), -7.0).bfloat16().cuda()  # the last row: the guard
    y = _run(fmt, x, c, s, None, out[:M])
    assert y.data_ptr() == out.data_ptr()
    torch.testing.assert_close(out[:M].float().cpu(), ref.float(), **TOL)
    assert bool((out[M] == -7.0).all())
    assert torch.equal(_run(fmt, x, c, s), out[:M])
