"""RoPE + paged K/V write micro-benchmark on one GPU: one layer's ``ext().rope_kv_write_chunk`` call for a chunk of
``T`` tokens of one sequence at the 7B head shape (32 q heads, 8 kv heads, head dim 128, interleaved rotation), into a
bf16 pool and into an FP8 e4m3 pool with shuffled pages -- against the composition it replaces: two ``apply_rope`` calls
(q and k) and ``write_rows``' two ``index_copy_`` (FP8: ``sanitize_kv`` + ``quantize_kv_rows`` on top).  All alternate in
one process.

    python tools/rope_chunk_bench.py             # T in {512, 2048}, page 64, PASSES=2

Protocol of ``tools/decode_attn_bench.py``: the timed loop (calls captured as one graph) cycles through copies of the
projection and of the pools of more than 1 GiB in total, so no call finds its operands in the last-level cache.  Prints
us per call and bytes moved / time (x read once; q, k and v written once)."""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from decode_attn_bench import D, HKV, HQ, timeit  # noqa: E402


def bench(ext, T: int, passes: int, page: int, dev: str) -> None:
    from scaling_amd.ops.quant import quantize_kv_rows, sanitize_kv
    from scaling_amd.ops.rope import apply_rope, rope_tables

    nh, rows = HQ + 2 * HKV, -(-T // page) * page
    n = max(2, -(-(1 << 30) // (T * nh * D * 2)))
    reps = max(20, min(n, 200))
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.randn(T, nh, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(n)]
    p16 = [(torch.zeros(rows, HKV, D, device=dev, dtype=torch.bfloat16), torch.zeros(rows, HKV, D, device=dev, dtype=torch.bfloat16))
           for _ in range(n)]
    p8 = [(torch.zeros(rows, HKV, D, device=dev, dtype=torch.uint8), torch.zeros(rows, HKV, D, device=dev, dtype=torch.uint8),
           torch.ones(HKV, rows, device=dev), torch.ones(HKV, rows, device=dev)) for _ in range(n)]
    cos, sin = rope_tables(D, rows, 10000.0, True, torch.bfloat16, dev)
    table = torch.randperm(rows // page, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(1, -1).to(dev)
    idx = (table.long().view(-1, 1) * page + torch.arange(page, device=dev).view(1, -1)).view(-1)[:T]
    cu_q = torch.tensor([0, T], device=dev, dtype=torch.int32)
    start = torch.zeros(1, device=dev, dtype=torch.long)
    pos = torch.arange(T, device=dev)
    err = torch.zeros(1, device=dev, dtype=torch.int32)

    def fused16(i):
        k, v = p16[i % n]
        return ext().rope_kv_write_chunk(xs[i % n], cos, sin, cu_q, start, HQ, HKV, D, True, k, v, err, table, page)

    def fused8(i):
        k, v, ks, vs = p8[i % n]
        return ext().rope_kv_write_chunk(xs[i % n], cos, sin, cu_q, start, HQ, HKV, D, True, k, v, err, table, page, ks, vs)

    def rotated(i):
        x = xs[i % n]
        return apply_rope(x[:, :HQ], cos, sin, pos, D, T, True), apply_rope(x[:, HQ : HQ + HKV], cos, sin, pos, D, T, True)

    def unfused16(i):
        q, kr = rotated(i)
        k, v = p16[i % n]
        k.index_copy_(0, idx, kr)
        v.index_copy_(0, idx, xs[i % n][:, HQ + HKV :])
        return q

    def unfused8(i):
        q, kr = rotated(i)
        k, v, ks, vs = p8[i % n]
        for codes, scale, val in ((k, ks, kr), (v, vs, xs[i % n][:, HQ + HKV :])):
            xb, nonfinite = sanitize_kv(val)
            c, s = quantize_kv_rows(xb, check=False)
            codes.index_copy_(0, idx, c)
            scale.index_copy_(1, idx, s)
            err.bitwise_or_(nonfinite.to(torch.int32) * 2)
        return q

    same = torch.equal(fused16(0), unfused16(0))
    b16 = T * D * 2 * (nh + HQ + 2 * HKV)
    b8 = T * D * (2 * nh + 2 * HQ + 2 * HKV) + 2 * T * HKV * 4
    with torch.no_grad():
        for p in range(passes):
            tf, tu, tf8, tu8 = timeit(fused16, reps), timeit(unfused16, reps), timeit(fused8, reps), timeit(unfused8, reps)
            print(f"T={T:5d} copies={n:4d} reps={reps:3d} pass {p}  bf16 pool: fused {tf:8.2f} us {b16 / tf / 1e6:5.2f} TB/s, "
                  f"unfused {tu:8.2f} us, ratio {tf / tu:5.3f}   fp8 pool: fused {tf8:8.2f} us {b8 / tf8 / 1e6:5.2f} TB/s, "
                  f"unfused {tu8:8.2f} us, ratio {tf8 / tu8:5.3f}   q equals unfused {same}", flush=True)
    del xs, p16, p8
    torch.cuda.empty_cache()


def main() -> None:
    from scaling_amd.ops._ext import ext

    passes, page = int(os.environ.get("PASSES", "2")), int(os.environ.get("PAGE", "64"))
    print(f"RoPE + paged K/V write, {HQ} q heads, {HKV} kv heads, head dim {D}, page {page} (shuffled); cold (copies "
          "cycled through > 1 GiB)", flush=True)
    for T in (512, 2048):
        bench(ext, T, passes, page, "cuda")


if __name__ == "__main__":
    main()
