"""Paged KV cache kernels on the GPU: the paged RoPE + K/V append against ``rope_kv_append_batch`` on slabs holding the
same data, and paged flash-decoding against the ``key_ranges`` call on the gathered contiguous buffer -- bit for bit in
bf16, fp16 and FP8, with the pages handed out in a shuffled order interleaved between the rows, and with every page and
table entry a call must not read poisoned (NaN pages, entries -1 and 2^30)."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a GPU", allow_module_level=True)

from scaling_amd.ops import attention  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

DEV = "cuda"
BF, FP16 = torch.bfloat16, torch.float16
KINDS = ["bf16", "fp16", "fp8"]
NQ, NKV = 4, 2


def _hand_out(needs, spare, seed):
    """Page ids for rows needing ``needs[i]`` pages out of a pool with ``spare`` pages left over, in a shuffled order and
    interleaved between the rows (row 0's first page, row 1's first page, ..., row 0's second page, ...)."""
    num_pages = sum(needs) + spare
    order = list(range(num_pages))
    random.Random(seed).shuffle(order)
    pages = [[] for _ in needs]
    for j in range(max(needs)):
        for i, n in enumerate(needs):
            if j < n:
                pages[i].append(order.pop())
    return pages, num_pages


def _table(pages, max_pages, poison=True):
    """int32 [B, max_pages]; the entries past a row's pages alternate between -1 and 2^30."""
    rows = []
    for i, pg in enumerate(pages):
        fill = [(-1 if (i + j) % 2 == 0 else 2**30) if poison else -1 for j in range(max_pages - len(pg))]
        rows.append(list(pg) + fill)
    return torch.tensor(rows, device=DEV, dtype=torch.int32)


def _pool_rows(pages, page, n):
    return torch.tensor([pages[j // page] * page + j % page for j in range(n)], device=DEV, dtype=torch.long)


# ---------------------------------------------------------------------------------------------- append
def _rope_tables(rows, rd):
    half = rd // 2
    inv = 1.0 / (10000 ** (torch.arange(0, half, device=DEV, dtype=torch.float32) / half))
    ang = torch.arange(rows, device=DEV, dtype=torch.float32)[:, None] * inv[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def _patterned(rows, hd, kind, seed):
    """(k, v[, k scales, v scales]) buffers of ``rows`` rows filled with a pattern no append writes by accident."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if kind == "fp8":
        k = torch.randint(0, 256, (rows, NKV, hd), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
        v = torch.randint(0, 256, (rows, NKV, hd), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
        ks = torch.rand(NKV, rows, device=DEV, generator=g) - 7.0
        vs = torch.rand(NKV, rows, device=DEV, generator=g) - 9.0
        return [k, v, ks, vs]
    dt = BF if kind == "bf16" else FP16
    return [torch.randn(rows, NKV, hd, device=DEV, generator=g).to(dt) for _ in range(2)]


def _slabs_like(bufs, rows):
    """Zeroed slab buffers of ``rows`` rows in the formats of the pool buffers (k, v[, scales [nkv, rows]])."""
    return [t.new_zeros((rows,) + tuple(t.shape[1:])) if t.dim() == 3 else t.new_zeros(t.shape[0], rows) for t in bufs]


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _append_paged(qkv, pos, rd, interleaved, bufs, table, page):
    cos, sin = _rope_tables(256, rd)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    q = ext().rope_kv_append_paged(qkv, cos, sin, pos, NQ, NKV, rd, interleaved, bufs[0], bufs[1], err, table, page,
                                   *bufs[2:])
    assert q is not None
    return q, int(err.item())


def _append_slab(qkv, pos, rd, interleaved, bufs, cap):
    cos, sin = _rope_tables(256, rd)
    err = torch.zeros(1, device=DEV, dtype=torch.int32)
    q = ext().rope_kv_append_batch(qkv, cos, sin, pos, NQ, NKV, rd, interleaved, bufs[0], bufs[1], err, cap, *bufs[2:])
    assert q is not None
    return q, int(err.item())


@pytest.mark.parametrize("page", [32, 64])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("hd,rd", [(64, 64), (64, 32)])
@pytest.mark.parametrize("kind", KINDS)
def test_append_equals_slab_append(kind, hd, rd, interleaved, page):
    max_pages = 3
    cap = max_pages * page
    dt = FP16 if kind == "fp16" else BF
    for B, positions in ((1, [2 * page + 5]), (3, [0, page - 1, page]), (5, [0, page - 1, page, 2 * page + 5, 7])):
        g = torch.Generator(device=DEV).manual_seed(hd + rd + B + page)
        mag = torch.tensor([2.0 ** (2 * b - 2) for b in range(B)], device=DEV).view(B, 1, 1)
        qkv = (torch.randn(B, NQ + 2 * NKV, hd, device=DEV, generator=g) * mag).to(dt)
        pos = torch.tensor(positions, device=DEV, dtype=torch.long)
        pages, num_pages = _hand_out([p // page + 1 for p in positions], 2, seed=B)
        table = _table(pages, max_pages)
        pool = _patterned(num_pages * page, hd, kind, 1)
        before = [t.clone() for t in pool]
        slab = _slabs_like(pool, B * cap)
        qp, ep = _append_paged(qkv, pos, rd, interleaved, pool, table, page)
        qs, es = _append_slab(qkv, pos, rd, interleaved, slab, cap)
        assert ep == 0 and es == 0
        assert torch.equal(qp, qs)
        prow = torch.tensor([pages[b][p // page] * page + p % page for b, p in enumerate(positions)], device=DEV)
        srow = torch.tensor([b * cap + p for b, p in enumerate(positions)], device=DEV)
        assert len(set(prow.tolist())) == B
        for t, s, b0 in zip(pool, slab, before):
            if t.dim() == 3:  # k / v rows (values or codes)
                assert torch.equal(t[prow], s[srow])
                t[prow] = b0[prow]
            else:  # FP8 scales [nkv, rows]
                assert torch.equal(t[:, prow], s[:, srow])
                t[:, prow] = b0[:, prow]
            assert torch.equal(_bytes(t), _bytes(b0)), "a byte outside the written rows changed"


@pytest.mark.parametrize("kind", KINDS)
def test_append_error_rows_write_nothing(kind):
    """Position = max_pages * page, a negative position, a table entry of -1 and one of num_pages: bit 0 of the error word,
    zero q rows, and not one pool byte changed.  All buffers are in bounds; the kernel must not follow the entries."""
    page, max_pages, hd = 32, 3, 64
    dt = FP16 if kind == "fp16" else BF
    g = torch.Generator(device=DEV).manual_seed(3)
    qkv = torch.randn(4, NQ + 2 * NKV, hd, device=DEV, generator=g).to(dt)
    num_pages = 6
    table = torch.tensor([[0, 1, 2], [3, -1, -1], [4, -1, 5], [5, num_pages, 2]], device=DEV, dtype=torch.int32)
    pos = torch.tensor([max_pages * page, -1, page + 3, page], device=DEV, dtype=torch.long)
    pool = _patterned(num_pages * page, hd, kind, 2)
    before = [t.clone() for t in pool]
    q, err = _append_paged(qkv, pos, 64, True, pool, table, page)
    assert err == 1
    assert not q.any()
    for t, b0 in zip(pool, before):
        assert torch.equal(_bytes(t), _bytes(b0))
    # a bad row beside good ones: the good rows are written and rotated as if alone
    pos2 = torch.tensor([5, -1, page + 3, 2 * page], device=DEV, dtype=torch.long)
    table2 = torch.tensor([[0, 1, 2], [3, -1, -1], [4, 1, 5], [5, 3, 2]], device=DEV, dtype=torch.int32)
    q2, err2 = _append_paged(qkv, pos2, 64, True, pool, table2, page)
    slab = _slabs_like(pool, 4 * 96)
    qs, _ = _append_slab(qkv, pos2.clamp(min=0), 64, True, slab, 96)
    assert err2 == 1 and not q2[1].any()
    for b in (0, 2, 3):
        assert torch.equal(q2[b], qs[b])
    assert torch.equal(pool[0][0 * page + 5], slab[0][5]) and torch.equal(pool[1][1 * page + 3], slab[1][2 * 96 + page + 3])
    assert torch.equal(pool[0][2 * page], slab[0][3 * 96 + 2 * page])
    assert torch.equal(pool[0][3 * page : 4 * page], before[0][3 * page : 4 * page])  # the bad row's page is untouched


# ---------------------------------------------------------------------------------------------- decode attention
def _paged_case(lengths, page, max_pages, Hk, D, kind, seed, spare=3):
    """Random K/V of the given lengths as (a) a pool with shuffled, interleaved pages, NaN in every unallocated page and in
    the tail of each last page, poisoned table entries past the used pages, and (b) one slab of max_pages * page rows per
    segment holding the same rows in logical order.  Returns dicts with k, v, scales (FP8), ranges, table."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    cap = max_pages * page
    nseg = len(lengths)
    pages, num_pages = _hand_out([-(-n // page) for n in lengths], spare, seed)
    rows = num_pages * page
    fp8 = kind == "fp8"
    dt = FP16 if kind == "fp16" else BF
    if fp8:
        def data(n):
            c = torch.randint(0, 256, (n, Hk, D), device=DEV, generator=g, dtype=torch.int32)
            c = torch.where((c & 0x7F) == 0x7F, c & 0x80, c).to(torch.uint8)
            e = torch.randint(-10, -7, (Hk, n), device=DEV, generator=g)
            e = e - 20 * ((torch.arange(n, device=DEV)[None, :] + torch.arange(Hk, device=DEV)[:, None]) % 2)
            return c, torch.ldexp(torch.ones(Hk, n, device=DEV), e)
        pool = {"k": torch.full((rows, Hk, D), 0x7F, device=DEV, dtype=torch.uint8),
                "ks": torch.full((Hk, rows), float("nan"), device=DEV)}
        pool["v"], pool["vs"] = pool["k"].clone(), pool["ks"].clone()
        slab = {"k": torch.zeros(nseg * cap, Hk, D, device=DEV, dtype=torch.uint8), "ks": torch.ones(Hk, nseg * cap, device=DEV)}
        slab["v"], slab["vs"] = slab["k"].clone(), slab["ks"].clone()
    else:
        def data(n):
            return torch.randn(n, Hk, D, device=DEV, generator=g).to(dt), None
        pool = {"k": torch.full((rows, Hk, D), float("nan"), device=DEV, dtype=dt), "ks": None, "vs": None}
        pool["v"] = pool["k"].clone()
        slab = {"k": torch.zeros(nseg * cap, Hk, D, device=DEV, dtype=dt), "ks": None, "vs": None}
        slab["v"] = slab["k"].clone()
    for i, n in enumerate(lengths):
        idx = _pool_rows(pages[i], page, n)
        for name in ("k", "v"):
            x, s = data(n)
            pool[name][idx] = x
            slab[name][i * cap : i * cap + n] = x
            if fp8:
                pool[name + "s"][:, idx] = s
                slab[name + "s"][:, i * cap : i * cap + n] = s
    pool["kr"] = torch.tensor([(0, n) for n in lengths], device=DEV, dtype=torch.int32)
    slab["kr"] = torch.tensor([(i * cap, n) for i, n in enumerate(lengths)], device=DEV, dtype=torch.int32)
    pool["table"] = _table(pages, max_pages)
    return pool, slab


def _both(q, pool, slab, page, max_k, window=-1, local_heads=-1, Lq=1):
    nseg = q.shape[0] // Lq
    cu_q = torch.arange(0, (nseg + 1) * Lq, Lq, device=DEV, dtype=torch.int32)
    scale = 1 / math.sqrt(q.shape[-1])
    with torch.no_grad():
        op, lp = ext().fa_fwd(q, pool["k"], pool["v"], cu_q, cu_q, Lq, scale, True, window, 0.0, 0, local_heads, max_k,
                              pool["kr"], pool["ks"], pool["vs"], pool["table"], page)
        os_, ls = ext().fa_fwd(q, slab["k"], slab["v"], cu_q, cu_q, Lq, scale, True, window, 0.0, 0, local_heads, max_k,
                               slab["kr"], slab["ks"], slab["vs"])
        scales = None if pool["ks"] is None else (pool["ks"], pool["vs"])
        pub = attention.flash_attention(q, pool["k"], pool["v"], cu_q, None, Lq, max_k, scale, True,
                                        window=None if window < 0 else window,
                                        local_heads=None if local_heads < 0 else local_heads, key_ranges=pool["kr"],
                                        kv_scales=scales, block_table=pool["table"], page_size=page)
    assert torch.isfinite(op.float()).all() and torch.isfinite(lp).all()
    assert torch.equal(op, os_), (op.float() - os_.float()).abs().max()
    assert torch.equal(lp, ls), (lp - ls).abs().max()
    assert torch.equal(pub, op)
    return op, lp


def _queries(n, H, D, kind, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(n, H, D, device=DEV, generator=g).to(FP16 if kind == "fp16" else BF)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("grp", [1, 2, 4])
@pytest.mark.parametrize("D", [32, 64, 128])
def test_paged_decode_equals_key_ranges(D, grp, kind):
    Hk = 2
    lengths = [1, 31, 32, 33, 64, 65, 95]
    pool, slab = _paged_case(lengths, 32, 3, Hk, D, kind, seed=D + grp)
    _both(_queries(len(lengths), Hk * grp, D, kind, 5), pool, slab, 32, 96)
    lengths = [129, 64, 1, 191]
    pool, slab = _paged_case(lengths, 64, 3, Hk, D, kind, seed=D + grp + 1)
    _both(_queries(len(lengths), Hk * grp, D, kind, 6), pool, slab, 64, 192)


@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_two_tiles_per_split(kind):
    """Hkv = 8, nseg = 16, max_seqlen_k = 320: 64-key splits of two tiles, which at page 32 come from two pages."""
    Hk, D = 8, 64
    lengths = [320, 1, 64, 65, 129, 255, 300, 33, 32, 96, 191, 200, 7, 128, 319, 257]
    pool, slab = _paged_case(lengths, 32, 10, Hk, D, kind, seed=11)
    _both(_queries(16, Hk, D, kind, 7), pool, slab, 32, 320)
    pool, slab = _paged_case([max(n, 2) for n in lengths], 32, 10, Hk, D, kind, seed=12)
    _both(_queries(16 * 2, Hk, D, kind, 8), pool, slab, 32, 320, Lq=2)  # two queries per segment, causal


@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_many_splits(kind):
    """One segment, Hkv = 2, max_seqlen_k = 640: 20 one-tile splits, more than the combine kernel's unrolled 16."""
    lengths = [640 - 13]
    pool, slab = _paged_case(lengths, 64, 10, 2, 128, kind, seed=12)
    _both(_queries(1, 8, 128, kind, 9), pool, slab, 64, 640)


@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_sliding_window_on_local_heads(kind):
    lengths = [95, 40, 64, 17]
    pool, slab = _paged_case(lengths, 32, 3, 2, 64, kind, seed=13)
    _both(_queries(4, 4, 64, kind, 10), pool, slab, 32, 96, window=16, local_heads=2)


@pytest.mark.parametrize("kind", KINDS)
def test_paged_decode_is_deterministic(kind):
    lengths = [95, 40, 64, 17]
    pool, slab = _paged_case(lengths, 32, 3, 2, 64, kind, seed=14)
    q = _queries(4, 8, 64, kind, 11)
    a = _both(q, pool, slab, 32, 96)
    b = _both(q, pool, slab, 32, 96)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_an_entry_outside_the_pool_masks_its_keys():
    """A table entry outside [0, num_pages) inside a row's length: its 32 keys count as masked, nothing is dereferenced."""
    pool, slab = _paged_case([96], 32, 3, 2, 64, "bf16", seed=15)
    q = _queries(1, 4, 64, "bf16", 12)
    cu = torch.tensor([0, 1], device=DEV, dtype=torch.int32)
    tab = pool["table"].clone()
    tab[0, 1] = 2**30
    o, _ = ext().fa_fwd(q, pool["k"], pool["v"], cu, cu, 1, 0.125, False, -1, 0.0, 0, -1, 96, pool["kr"], None, None, tab, 32)
    k, v = slab["k"][:96].clone(), slab["v"][:96].clone()
    keep = torch.cat([torch.arange(0, 32), torch.arange(64, 96)]).to(DEV)
    ref = attention.attention_reference(q.float(), k[keep].float(), v[keep].float(), cu, cu * 64, 0.125, False)
    assert torch.isfinite(o.float()).all()
    torch.testing.assert_close(o.float(), ref, atol=2e-2, rtol=2e-2)


def test_rejections():
    pool, _ = _paged_case([40, 7], 32, 2, 2, 64, "bf16", seed=16)
    q = _queries(2, 4, 64, "bf16", 13)
    cu = torch.arange(3, device=DEV, dtype=torch.int32)
    base = dict(cu_seqlens_q=cu, max_seqlen_q=1, max_seqlen_k=64, key_ranges=pool["kr"], block_table=pool["table"],
                page_size=32)

    def call(**kw):
        args = dict(base)
        args.update(kw)
        return attention.flash_attention(q, pool["k"], pool["v"], **args)

    with torch.no_grad():
        call()
        for bad in (48, 16, 0, -32):
            with pytest.raises(ValueError, match="multiple of 32"):
                call(page_size=bad)
        with pytest.raises(ValueError, match="int32"):
            call(block_table=pool["table"].long())
        with pytest.raises(ValueError, match="int32"):
            call(block_table=pool["table"][:1])
        with pytest.raises(ValueError, match="int32"):
            call(block_table=pool["table"].view(-1))
        with pytest.raises(ValueError, match="is on"):
            call(block_table=pool["table"].cpu())
        with pytest.raises(ValueError, match="key_ranges"):
            call(key_ranges=None, cu_seqlens_k=cu)
        with pytest.raises(ValueError, match="come together"):
            call(page_size=None)
        with pytest.raises(ValueError, match="dropout"):
            call(dropout_p=0.1, training=True)
    with pytest.raises(ValueError, match="forward only"):
        attention.flash_attention(q.clone().requires_grad_(), pool["k"], pool["v"], **base)
