"""``chunk_attention(..., key_bias=)`` (the KB form of csrc/kernels/flash_chunk.hip) against a dense fp32 softmax that
adds the bias, ``o`` and ``lse``.  k / v / key_bias rows outside the segments' ranges hold NaN.  Every query row keeps a
finite unmasked key: ``-inf`` on a first key only where each row sees a later one (Lk > Lq), a ``-inf`` tile only behind
64 finite keys."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops.attention import chunk_attention  # noqa: E402

TOL = dict(atol=2e-2, rtol=2e-2)  # tests/test_chunk_attn_gpu.py's bound for the unbiased kernel against its reference
INF = float("-inf")
BIAS = {"zeros": (slice(0), 0.0), "log03": (slice(None, None, 3), math.log(0.3)), "m10000": (slice(1), -10000.0),
        "inf_first": (slice(1), INF), "inf_tile": (slice(64, 128), INF)}


def run(segs, grp, D, dtype, start=0, bias=True, check=True, window=-1, local_heads=None, **kw):
    """Segments [(Lq, Lk, bias kind)], keys back to back from buffer row ``start``; returns the kernel's (o, lse)."""
    g = torch.Generator().manual_seed(len(segs) + D)
    rows, H = start + sum(s[1] for s in segs) + 3, 2 * grp
    q = torch.randn(sum(s[0] for s in segs), H, D, generator=g).to(dtype).cuda()
    k, v = (torch.full((rows, 2, D), float("nan"), dtype=dtype).cuda() for _ in range(2))
    kb, kr, cu, o, lse = torch.full((rows,), float("nan")).cuda(), [], [0], torch.zeros_like(q, dtype=torch.float), []
    for lq, lk, kind in segs:
        q0, k0 = cu[-1], start + sum(r[1] for r in kr)
        k[k0 : k0 + lk], v[k0 : k0 + lk] = (torch.randn(lk, 2, D, generator=g).to(dtype).cuda() for _ in range(2))
        kb[k0 : k0 + lk] = 0.0
        kb[k0 : k0 + lk][BIAS[kind][0]] = BIAS[kind][1]
        kr.append([k0, lk])
        cu.append(q0 + lq)
        s = torch.einsum("qhd,khd->hqk", q[q0 : q0 + lq].float(), k[k0 : k0 + lk].float().repeat_interleave(grp, 1))
        s = s / math.sqrt(D) + kb[k0 : k0 + lk]
        qp, kp = torch.arange(lq).cuda()[:, None] + lk - lq, torch.arange(lk).cuda()[None, :]
        ok = torch.stack([(kp <= qp) & ((kp >= qp - window) | (window < 0) | (h >= (local_heads or H))) for h in range(H)])
        s = s.masked_fill(~ok, INF)
        lse.append(torch.logsumexp(s, -1))
        o[q0 : q0 + lq] = torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), v[k0 : k0 + lk].float().repeat_interleave(grp, 1))
    lse = torch.cat(lse, 1)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all(), "the case leaves a row without a finite key"
    got = chunk_attention(q, k, v, torch.tensor(cu, dtype=torch.int32).cuda(), torch.tensor(kr, dtype=torch.int32).cuda(),
                          max(s[0] for s in segs), max(s[1] for s in segs), return_lse=True, window=None if window < 0 else window,
                          local_heads=local_heads, **{"key_bias": kb if bias is True else bias, **kw})
    if check:
        print(f"{segs} {kw}: max abs diff o {(got[0].float() - o).abs().max():.3e} lse {(got[1] - lse).abs().max():.3e}")
        torch.testing.assert_close(got[0].float(), o, **TOL)
        torch.testing.assert_close(got[1], lse, **TOL)
    return got, kb


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("grp", [1, 4])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_prompt_lengths_around_the_key_tile(D, grp, dtype):
    for L in (1, 63, 64, 65, 129):
        for kind in ("zeros", "log03", "m10000") + (("inf_tile",) if L > 128 else ()):
            got, _ = run([(L, L, kind)], grp, D, dtype)
            if kind == "zeros":  # seeded with 0: the unbiased kernel's bits
                plain, _ = run([(L, L, kind)], grp, D, dtype, bias=None, check=False)
                assert torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1])
        run([(L, L + 1, "inf_first")], grp, D, dtype)


@pytest.mark.parametrize("splits", [0, 1, 2, 5])
def test_context_from_a_nonzero_start_segments_and_forced_splits(splits):
    run([(40, 200, "inf_first"), (0, 7, "zeros"), (130, 225, "inf_tile"), (33, 33, "m10000")], 4, 64, torch.float16, start=37, splits=splits)
    run([(40, 200, "log03")], 4, 128, torch.bfloat16, start=37, splits=splits)


def test_window_on_local_heads_and_refusals():
    run([(130, 225, "log03"), (65, 65, "m10000")], 4, 128, torch.bfloat16, window=40, local_heads=6)  # heads 6, 7 global
    _, kb = run([(40, 71, "log03")], 2, 64, torch.bfloat16)
    for match, kw in (("key_bias with block_table", dict(block_table=torch.zeros(1, 3, dtype=torch.int32).cuda(), page_size=32)),
                      ("key_bias with kv_scales", dict(kv_scales=(kb, kb))), ("key_bias must be", dict(bias=kb.double())),
                      ("key_bias must be", dict(bias=kb[:-1])), ("key_bias must be", dict(bias=kb.repeat_interleave(2)[::2]))):
        with pytest.raises(ValueError, match=match):
            run([(40, 71, "log03")], 2, 64, torch.bfloat16, check=False, **kw)
