"""``ops.attention.chunk_attention`` (csrc/kernels/flash_chunk.hip) against ``attention_reference`` in fp32, paged = slab
and FP8 = bf16 bitwise, both write paths, and the refusals.  Every pool is poisoned: NaN in unowned pages and page
tails, table entries -1 / 2**30 past the used pages."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import attention, quant  # noqa: E402

DEV = torch.device("cuda", 0)
TOL = dict(atol=2e-2, rtol=2e-2)  # tests/test_batch_decode_gpu.py's bound for the decode kernel against this reference
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp8": torch.bfloat16}


class Case:
    """Segments [(ctx, Lq), ...] over a poisoned pool, page ids shuffled and interleaved; slab form: 5 junk rows first."""

    def __init__(self, segs, Hk, grp, D, kind, page, seed=0, poison=True):
        g = torch.Generator(device="cpu").manual_seed(seed)
        dt = DTYPES[kind]
        self.kind, self.page, self.fp8 = kind, page, kind == "fp8"
        self.lq = [s[1] for s in segs]
        self.lk = [s[0] + s[1] for s in segs]
        need = [-(-n // page) for n in self.lk]
        ids = list(range(sum(need) + 3))
        random.Random(seed).shuffle(ids)
        owned = [[] for _ in segs]
        for j in range(max(need)):  # dealt round-robin: the segments' pages interleave in the pool
            for i, n in enumerate(need):
                if j < n:
                    owned[i].append(ids.pop())
        ids = range(sum(need) + 3)
        width = max(need) + 2
        tab = [o + [(-1, 2**30)[j % 2] for j in range(width - len(o))] for o in owned]
        self.table = torch.tensor(tab, dtype=torch.int32, device=DEV)
        self.k_range = torch.tensor([[0, n] for n in self.lk], dtype=torch.int32, device=DEV)
        self.cu_q = torch.tensor([sum(self.lq[:i]) for i in range(len(segs) + 1)], dtype=torch.int32, device=DEV)
        self.q = torch.randn(sum(self.lq), Hk * grp, D, generator=g).to(dt).to(DEV)
        rows = len(ids) * page
        dense = [torch.randn(2, n, Hk, D, generator=g).to(dt).to(DEV) for n in self.lk]
        bad = float("nan") if poison else 0.0
        if self.fp8:
            self.k = torch.full((rows, Hk, D), 0x7F if poison else 0, dtype=torch.uint8, device=DEV)
            self.v = self.k.clone()
            self.scales = (torch.full((Hk, rows), bad if poison else 1.0, device=DEV),
                           torch.full((Hk, rows), bad if poison else 1.0, device=DEV))
        else:
            self.k = torch.full((rows, Hk, D), bad, dtype=dt, device=DEV)
            self.v = self.k.clone()
            self.scales = None
        self.rows, ranges = attention.gather_pages(self.table, page, self.lk)
        self.slab_range = ranges + torch.tensor([5, 0], dtype=torch.int32, device=DEV)
        for i, d in enumerate(dense):
            at = self.rows[int(ranges[i, 0]) : int(ranges[i, 0]) + self.lk[i]]
            for buf, sc, x in ((self.k, 0, d[0]), (self.v, 1, d[1])):
                if self.fp8:
                    c, s = quant.quantize_kv_rows(x)
                    buf[at] = c
                    self.scales[sc][:, at] = s
                else:
                    buf[at] = x

    def dequantised(self):
        if not self.fp8:
            return self.k, self.v
        return (quant.dequantize_kv_rows(self.k, self.scales[0]), quant.dequantize_kv_rows(self.v, self.scales[1]))

    def call(self, form="paged", k=None, v=None, scales="own", **kw):
        k, v = (self.k, self.v) if k is None else (k, v)
        scales = self.scales if scales == "own" else scales
        args = dict(softmax_scale=1.0 / math.sqrt(self.q.shape[-1]), return_lse=True, kv_scales=scales)
        args.update(kw)
        if form == "paged":
            return attention.chunk_attention(self.q, k, v, self.cu_q, self.k_range, max(self.lq), max(self.lk),
                                             block_table=self.table, page_size=self.page, **args)
        pad = lambda t, dim: torch.cat([t.narrow(dim, 0, 5), t.index_select(dim, self.rows)], dim)  # noqa: E731
        if scales is not None:
            args["kv_scales"] = (pad(scales[0], 1), pad(scales[1], 1))
        return attention.chunk_attention(self.q, pad(k, 0), pad(v, 0), self.cu_q, self.slab_range, max(self.lq),
                                         max(self.lk), **args)

    def reference(self, causal=True, window=-1, local_heads=None):
        kd, vd = (t.index_select(0, self.rows).float() for t in self.dequantised())
        _, ranges = attention.gather_pages(self.table, self.page, self.lk)
        q, scale = self.q.float(), 1.0 / math.sqrt(self.q.shape[-1])
        o = attention.attention_reference(q, kd, vd, self.cu_q, None, scale, causal, window, local_heads=local_heads,
                                          key_ranges=ranges)
        # attention_reference returns no lse: log-sum-exp of the same fp32 scores over the keys its mask keeps
        lse = torch.full((q.shape[1], q.shape[0]), float("nan"), device=DEV)
        grp = q.shape[1] // kd.shape[1]
        for i, (lq, lk) in enumerate(zip(self.lq, self.lk)):
            q0, k0 = int(self.cu_q[i]), int(ranges[i, 0])
            s = torch.einsum("qhd,khd->hqk", q[q0 : q0 + lq], kd[k0 : k0 + lk].repeat_interleave(grp, 1)) * scale
            qp = torch.arange(lq, device=DEV)[:, None] + lk - lq
            kp = torch.arange(lk, device=DEV)[None, :]
            ok = (kp <= qp) if causal else torch.ones(lq, lk, dtype=torch.bool, device=DEV)
            okw = ok & (kp >= qp - window) & ((kp <= qp + window) | causal) if window >= 0 else ok
            nl = q.shape[1] if local_heads is None else local_heads
            mask = torch.stack([okw if h < nl else ok for h in range(q.shape[1])])
            lse[:, q0 : q0 + lq] = torch.logsumexp(s.masked_fill(~mask, float("-inf")), -1)
        return o, lse


def _close(got, ref, what):
    for name, a, b in (("o", got[0], ref[0]), ("lse", got[1], ref[1])):
        print(f"{what} {name}: max abs diff {(a.float() - b).abs().max().item():.3e}")
        torch.testing.assert_close(a.float(), b, **TOL, msg=lambda m: f"{what} {name}: {m}")


def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (what, (a[0].float() - b[0].float()).abs().max().item())


def _check(c, splits=0, **mask):
    """The paged call: close to the reference, bitwise the slab call and (FP8) the bf16 call on the dequantised pool."""
    got = c.call("paged", splits=splits, **mask)
    _close(got, c.reference(**mask), f"{c.kind} splits={splits} {mask}")
    _same(got, c.call("slab", splits=splits, **mask), "paged vs slab")
    if c.fp8:
        _same(got, c.call("paged", *c.dequantised(), scales=None, splits=splits, **mask), "fp8 vs bf16 on dequantised")
    return got


# (D, group, kind, ctx, Lq, page): packed rows cross 32 / 128 / 129, keys cross 32-, 64- and page boundaries
CASES = [(128, 4, "bf16", 0, 33, 32), (128, 4, "fp8", 0, 128, 64), (64, 1, "fp16", 1, 129, 32),
         (32, 3, "bf16", 31, 40, 64), (64, 8, "fp8", 64, 64, 32), (128, 1, "fp16", 95, 130, 64),
         (64, 3, "bf16", 200, 300, 32), (32, 8, "fp16", 200, 300, 64), (128, 8, "bf16", 95, 130, 32),
         (32, 1, "fp8", 1, 129, 64), (64, 4, "fp16", 31, 40, 32), (32, 4, "bf16", 0, 128, 32),
         (128, 3, "fp8", 200, 300, 64), (64, 1, "bf16", 64, 64, 64)]


@pytest.mark.parametrize("D,grp,kind,ctx,Lq,page", CASES)
def test_one_segment(D, grp, kind, ctx, Lq, page):
    _check(Case([(ctx, Lq)], 2, grp, D, kind, page, seed=1))


@pytest.mark.parametrize("splits", [0, 1, 2, 5])
@pytest.mark.parametrize("kind", ["bf16", "fp8"])
@pytest.mark.parametrize("ctx,Lq", [(200, 300), (95, 130)])
def test_split_plans_and_determinism(ctx, Lq, kind, splits):
    c = Case([(ctx, Lq)], 2, 4, 128, kind, 32, seed=2)
    _same(_check(c, splits), c.call("paged", splits=splits), "two identical calls")


@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8"])
def test_three_segments_one_empty(kind):
    c = Case([(31, 40), (7, 0), (95, 130)], 2, 4, 64, kind, 32, seed=3)
    _check(c)
    _check(c, splits=3)


@pytest.mark.parametrize("kind", ["bf16", "fp8"])
def test_window_on_some_heads_of_a_kv_group(kind):
    c = Case([(95, 130)], 2, 4, 128, kind, 64, seed=4)  # 8 q heads; heads 4, 5 windowed and 6, 7 global share kv head 1
    _check(c, window=40, local_heads=6)
    _check(c, window=40)


def test_not_causal():
    _check(Case([(31, 40)], 2, 3, 64, "bf16", 32, seed=5), causal=False)


@pytest.mark.parametrize("kind", ["bf16", "fp16", "fp8"])
def test_unowned_memory_is_not_read(kind):
    dirty, clean = (Case([(95, 130), (1, 33)], 2, 4, 128, kind, 64, seed=6, poison=p) for p in (True, False))
    for splits in (0, 2):
        got = dirty.call("paged", splits=splits)
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
        _same(got, clean.call("paged", splits=splits), f"poisoned vs clean pool, splits={splits}")


def test_rejections():
    c = Case([(31, 40)], 2, 2, 64, "fp8", 32, seed=7)
    kw = dict(kv_scales=c.scales, block_table=c.table, page_size=32)
    for err, change in (("multiple of 32", dict(page_size=48)), ("block_table", dict(block_table=c.table.repeat(2, 1)))):
        with pytest.raises(ValueError, match=err):
            attention.chunk_attention(c.q, c.k, c.v, c.cu_q, c.k_range, 40, 71, **{**kw, **change})
    with pytest.raises(ValueError, match="bfloat16"):
        attention.chunk_attention(c.q.half(), c.k, c.v, c.cu_q, c.k_range, 40, 71, **kw)
    with torch.enable_grad(), pytest.raises(ValueError, match="forward only"):
        attention.chunk_attention(c.q.clone().requires_grad_(), c.k, c.v, c.cu_q, c.k_range, 40, 71, **kw)
