"""Chunk attention micro-benchmark on one GPU: one layer's ``ext().fa_chunk`` call (a chunk of ``Lq`` queries after
``ctx`` cached tokens, over a paged pool with shuffled pages) at the 7B head shape (32 q heads, 8 kv heads, head dim
128), over bf16 pages and over the FP8 e4m3 pages that encode the same values -- against what admission costs without
it at the same ``(Lq, Lk)``: ``ext().fa_fwd`` over contiguous bf16 keys in ``cu_k`` form plus the ``load_row`` copy of
the ``Lk`` rows into the pool.  All alternate in one process.

    python tools/chunk_attn_bench.py             # chunk in {128, 512, 2048} x ctx in {0, 2048, 8192}, PASSES=2
    KEYBIAS=1 python tools/chunk_attn_bench.py   # key_bias form vs plain vs dense torch, Lq = Lk in {512, 2048, 4096}

Protocol of ``tools/decode_attn_bench.py``: the timed loop (calls captured as one graph) cycles through pool copies of
more than 1 GiB in total (at most ``MAXCOPIES``, default 256), so no call finds its keys in the last-level cache.  Prints
us per call, the achieved MFMA rate of the chunk call (4 Lq Lk' D Hq flops, Lk' the causal average of visible keys) and
the ratios."""
from __future__ import annotations

import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from decode_attn_bench import D, HKV, HQ, make_copies, timeit  # noqa: E402


def bench(ext, Lq: int, ctx: int, passes: int, page: int, dev: str) -> None:
    Lk = ctx + Lq
    rows = -(-Lk // page) * page
    nb16 = rows * HKV * D * 2 * 2
    n = max(2, min(int(os.environ.get("MAXCOPIES", "256")), -(-(1 << 30) // nb16)))
    reps = max(20, min(n, 200))
    f8, bf = make_copies(n, rows, dev)
    scale = D ** -0.5
    q = torch.randn(Lq, HQ, D, device=dev, dtype=torch.bfloat16)
    cu_q = torch.tensor([0, Lq], device=dev, dtype=torch.int32)
    cu_k = torch.tensor([0, Lk], device=dev, dtype=torch.int32)
    kr = torch.tensor([[0, Lk]], device=dev, dtype=torch.int32)
    table = torch.randperm(rows // page, generator=torch.Generator().manual_seed(1)).to(torch.int32).view(1, -1).to(dev)
    idx = (table.long().view(-1, 1) * page + torch.arange(page, device=dev).view(1, -1)).view(-1)[:Lk]
    dst_k, dst_v = torch.empty_like(bf[0][0]), torch.empty_like(bf[0][1])

    def chunk16(i):
        k, v = bf[i % n]
        return ext().fa_chunk(q, k, v, cu_q, Lq, scale, True, -1, -1, Lk, kr, None, None, table, page)

    def chunk8(i):
        kc, ks, vc, vs = f8[i % n]
        return ext().fa_chunk(q, kc, vc, cu_q, Lq, scale, True, -1, -1, Lk, kr, ks, vs, table, page)

    def fwd(i):  # today's admission: the prefill kernel over contiguous keys ...
        k, v = bf[i % n]
        return ext().fa_fwd(q, k[:Lk], v[:Lk], cu_q, cu_k, Lq, scale, True, -1, 0.0, 0, -1, Lk)

    def copy(i):  # ... and load_row's copy of the prompt's rows into its pages
        k, v = bf[i % n]
        dst_k.index_copy_(0, idx, k[:Lk])
        dst_v.index_copy_(0, idx, v[:Lk])

    k0, v0 = bf[0]
    ref = ext().fa_fwd(q, k0[idx], v0[idx], cu_q, cu_k, Lq, scale, True, -1, 0.0, 0, -1, Lk)[0]
    o16, o8 = chunk16(0)[0], chunk8(0)[0]
    err = (o16.float() - ref.float()).abs().max().item()
    flops = 4.0 * Lq * (ctx + (Lq + 1) / 2) * D * HQ
    for p in range(passes):
        t16, tf, tc, t8 = timeit(chunk16, reps), timeit(fwd, reps), timeit(copy, reps), timeit(chunk8, reps)
        print(f"chunk={Lq:5d} ctx={ctx:5d} copies={n:4d} reps={reps:3d} pass {p}  fa_chunk bf16 {t16:9.2f} us "
              f"{flops / t16 / 1e6:6.1f} TF   fp8 {t8:9.2f} us {flops / t8 / 1e6:6.1f} TF   fa_fwd {tf:9.2f} us + copy "
              f"{tc:8.2f} us   chunk/(fwd+copy) bf16 {t16 / (tf + tc):5.3f} fp8 {t8 / (tf + tc):5.3f}   chunk/fwd "
              f"{t16 / tf:5.3f}   fp8 equals bf16 {torch.equal(o16, o8)}  max |chunk - fa_fwd| {err:.2e}", flush=True)
    del f8, bf
    torch.cuda.empty_cache()


def bench_key_bias(ext, L: int, passes: int, dev: str) -> None:
    """A manipulated prompt pass (Lq = Lk = L, slab keys): ``fa_chunk`` without and with ``key_bias`` (log 0.3 on every
    7th key, -10000 on one), alternating over the cold copies, and beside them the dense torch branch
    (``multi_head_attention``, [1, heads, L, L] scores) on the same inputs, timed eagerly (its mask builder reads back)."""
    from scaling_amd.core.nn.attention.attention import multi_head_attention
    from scaling_amd.core.nn.masked_softmax import MaskedSoftmax, MaskedSoftmaxConfig

    n = max(2, min(int(os.environ.get("MAXCOPIES", "256")), -(-(1 << 30) // (L * HKV * D * 2 * 2))))
    reps = max(20, min(n, 200))
    g = torch.Generator(device=dev).manual_seed(0)
    kv = [tuple(torch.randn(L, HKV, D, device=dev, generator=g).to(torch.bfloat16) for _ in range(2)) for _ in range(n)]
    q = torch.randn(L, HQ, D, device=dev, generator=g).to(torch.bfloat16)
    scale = D ** -0.5
    cu = torch.tensor([0, L], device=dev, dtype=torch.int32)
    kr = torch.tensor([[0, L]], device=dev, dtype=torch.int32)
    bias = torch.zeros(L, device=dev)
    bias[::7] = math.log(0.3)
    bias[L // 3] = -10000.0

    def plain(i):
        return ext().fa_chunk(q, *kv[i % n], cu, L, scale, True, -1, -1, L, kr)

    def biased(i):
        return ext().fa_chunk(q, *kv[i % n], cu, L, scale, True, -1, -1, L, kr, None, None, None, 0, 0, bias)

    softmax = MaskedSoftmax(MaskedSoftmaxConfig(kernel="torch"))
    manip = bias.to(torch.bfloat16).view(1, 1, 1, L).expand(1, 1, L, L)

    def dense(i):
        k, v = (t.repeat_interleave(HQ // HKV, 1).view(1, L, HQ, D) for t in kv[i % n])
        return multi_head_attention(q.view(1, L, HQ, D), k, v, cu, True, scale, softmax,
                                    attention_scores_manipulation=manip)

    ref = dense(0).view(L, HQ, D).float()
    err = (biased(0)[0].float() - ref).abs().max().item()
    flops = 4.0 * L * ((L + 1) / 2) * D * HQ
    for p in range(passes):
        t0, t1 = timeit(plain, reps), timeit(biased, reps)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(5):
            dense(i)
        e1.record()
        torch.cuda.synchronize()
        td = 1000.0 * e0.elapsed_time(e1) / 5
        print(f"key bias  Lq=Lk={L:5d} copies={n:4d} reps={reps:3d} pass {p}  fa_chunk {t0:9.2f} us {flops / t0 / 1e6:6.1f} TF"
              f"   with key_bias {t1:9.2f} us {flops / t1 / 1e6:6.1f} TF   biased/plain {t1 / t0:5.3f}   torch dense "
              f"{td:10.2f} us (x{td / t1:6.1f})   max |fa_chunk - dense| {err:.2e}", flush=True)
    del kv
    torch.cuda.empty_cache()


def main() -> None:
    from scaling_amd.ops._ext import ext

    if os.environ.get("KEYBIAS", "0") == "1":  # the key-bias form against the unbiased call and the dense torch branch
        print(f"chunk attention with key_bias, {HQ} q heads, {HKV} kv heads, head dim {D}, slab keys; cold (K/V copies "
              "cycled through > 1 GiB)", flush=True)
        for L in (512, 2048, 4096):
            bench_key_bias(ext, L, int(os.environ.get("PASSES", "2")), "cuda")
        return
    passes, page = int(os.environ.get("PASSES", "2")), int(os.environ.get("PAGE", "64"))
    print(f"chunk attention, {HQ} q heads, {HKV} kv heads, head dim {D}, page {page} (shuffled); cold (pool copies "
          "cycled through > 1 GiB)", flush=True)
    for Lq in (128, 512, 2048):
        for ctx in (0, 2048, 8192):
            bench(ext, Lq, ctx, passes, page, "cuda")


if __name__ == "__main__":
    main()
