"""Decode attention micro-benchmark on one GPU: the flash-decoding call of one layer alone (``ext().fa_fwd`` over key
ranges, one query token per sequence) at the 7B head shape (32 q heads, 8 kv heads, head dim 128), over a bf16 cache
and over the FP8 e4m3 cache that encodes the same values, alternating in one process.

    python tools/decode_attn_bench.py            # B in {1, 16} x context in {128, 1024, 4096, 16384}, PASSES=2

Protocol of ``tools/gemv_bench.py``: the timed loop (calls captured as one graph) cycles through cache copies of more
than 1 GiB in total (bf16; the FP8 copies are the same count), and runs at least ``REPS`` calls and as many as it takes
for the FP8 calls of one replay to read 512 MiB of distinct copies -- twice the 256 MiB last-level cache, so no pass
finds what the one before left there, however small the shape.  Prints us per call and bytes streamed / time (codes
plus scales for FP8).

``slab`` is the rows between two sequences' first rows: ``ctx`` (every slab starts at a multiple of four rows, so the
four scales of a register group sit at a 16-byte aligned address) and, for B = 16, ``ctx + 1`` -- what the batched
decoder's capacity (longest prompt + max_tokens) is in general: slabs start at arbitrary rows and most groups are at
dword-aligned addresses only.

``paged`` (the ``slab = ctx`` lines): the same buffers read as a pool of ``PAGE``-row pages (default 64) through a block
table that names the pages in a shuffled order -- the paged form of the same call, alternating with the slab call in the
same pass.  Both read the same bytes; the difference is the table lookup per 32-key tile and the page order."""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HQ, HKV, D = 32, 8, 128


def timeit(fn, reps: int) -> float:
    for i in range(5):
        fn(reps + i)  # warm-up on copies the timed loop reaches last (or never)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(reps):
            fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps


def make_copies(n: int, rows: int, dev: str):
    """n cache copies: (K codes, K scales, V codes, V scales) and the bf16 (K, V) they encode."""
    from scaling_amd.ops.quant import dequantize_kv_rows

    g = torch.Generator(device=dev).manual_seed(0)
    f8, bf = [], []
    for _ in range(n):
        one = []
        for _ in range(2):
            codes = torch.randint(0, 256, (rows, HKV, D), device=dev, generator=g, dtype=torch.int32)
            codes = torch.where((codes & 0x7F) == 0x7F, codes & 0x80, codes).to(torch.uint8)
            scale = torch.ldexp(torch.ones(HKV, rows, device=dev), torch.randint(-10, -7, (HKV, rows), device=dev, generator=g))
            one += [codes, scale]
        f8.append(tuple(one))
        bf.append((dequantize_kv_rows(one[0], one[1]), dequantize_kv_rows(one[2], one[3])))
    return f8, bf


def main() -> None:
    from scaling_amd.ops._ext import ext

    dev = "cuda"
    passes = int(os.environ.get("PASSES", "2"))
    reps = int(os.environ.get("REPS", "100"))
    scale = D ** -0.5
    print(f"decode attention, {HQ} q heads, {HKV} kv heads, head dim {D}; cold (cache copies cycled through > 1 GiB)", flush=True)
    for B in (1, 16):
        for ctx in (128, 1024, 4096, 16384):
            for slab in ((ctx, ctx + 1) if B > 1 else (ctx,)):
                bench(ext, B, ctx, slab, passes, reps, scale, dev)


def bench(ext, B: int, ctx: int, slab: int, passes: int, reps: int, scale: float, dev: str) -> None:
    rows = B * slab
    nb16 = B * ctx * HKV * D * 2 * 2
    nb8 = B * ctx * HKV * (D + 4) * 2
    n = max(2, -(-(1 << 30) // nb16))
    reps = max(reps, min(n, -(-(1 << 29) // nb8)))
    f8, bf = make_copies(n, rows, dev)
    q = torch.randn(B, HQ, D, device=dev, dtype=torch.bfloat16)
    cu_q = torch.arange(B + 1, device=dev, dtype=torch.int32)
    kr = torch.tensor([[b * slab, ctx] for b in range(B)], device=dev, dtype=torch.int32)

    def run16(i):
        k, v = bf[i % n]
        return ext().fa_fwd(q, k, v, cu_q, cu_q, 1, scale, True, -1, 0.0, 0, -1, slab, kr)

    def run8(i):
        kc, ks, vc, vs = f8[i % n]
        return ext().fa_fwd(q, kc, vc, cu_q, cu_q, 1, scale, True, -1, 0.0, 0, -1, slab, kr, ks, vs)

    page = int(os.environ.get("PAGE", "64"))
    paged = slab == ctx and ctx % page == 0
    if paged:  # the same buffers as a pool of pages, handed out in a shuffled order
        gp = torch.Generator().manual_seed(1)
        table = torch.randperm(rows // page, generator=gp).to(torch.int32).view(B, ctx // page).to(dev)
        kr0 = torch.tensor([[0, ctx]] * B, device=dev, dtype=torch.int32)

        def run16p(i):
            k, v = bf[i % n]
            return ext().fa_fwd(q, k, v, cu_q, cu_q, 1, scale, True, -1, 0.0, 0, -1, slab, kr0, None, None, table, page)

        def run8p(i):
            kc, ks, vc, vs = f8[i % n]
            return ext().fa_fwd(q, kc, vc, cu_q, cu_q, 1, scale, True, -1, 0.0, 0, -1, slab, kr0, ks, vs, table, page)

        # the paged call against the slab call on the rows gathered in logical order
        idx = (table.long().view(-1, 1) * page + torch.arange(page, device=dev).view(1, -1)).view(-1)
        k0, v0 = bf[0]
        ref = ext().fa_fwd(q, k0[idx], v0[idx], cu_q, cu_q, 1, scale, True, -1, 0.0, 0, -1, slab, kr)[0]
        same_p = torch.equal(run16p(0)[0], ref) and torch.equal(run8p(0)[0], ref)
        del idx, ref
    same = torch.equal(run16(0)[0], run8(0)[0])
    for p in range(passes):
        us16 = timeit(run16, reps)
        us16p = timeit(run16p, reps) if paged else 0.0
        us8 = timeit(run8, reps)
        us8p = timeit(run8p, reps) if paged else 0.0
        line = (f"B={B:2d} ctx={ctx:5d} slab={slab:5d} reps={reps:4d} pass {p}  bf16 {us16:8.2f} us {nb16 / us16 / 1e6:5.2f} TB/s   "
                f"fp8 {us8:8.2f} us {nb8 / us8 / 1e6:5.2f} TB/s   bf16/fp8 time {us16 / us8:4.2f}  "
                f"outputs equal {same}")
        if paged:
            line += (f"   paged({page}) bf16 {us16p:8.2f} us x{us16p / us16:5.3f}   fp8 {us8p:8.2f} us x{us8p / us8:5.3f}  "
                     f"paged equal gathered slab {same_p}")
        print(line, flush=True)
    del f8, bf
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
