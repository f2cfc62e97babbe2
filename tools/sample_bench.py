"""Isolated time of one batch-1 sampling step on one GPU: the fused kernel (``ops.sample.sample_logits``) against
``torch.argmax`` (the launch it replaces in greedy decoding) and against the torch composition
``sample_temperature(top_p_transform(top_k_transform(x, k), p), T)``.

    python tools/sample_bench.py [--vocab 32000 128000] [--iters 2000] [--sampler 0.8,40,0.95]

warm: the same row every call (L2-resident); cold: every call reads another row of a buffer larger than the
256 MiB Infinity Cache.  Device-event time over ``iters`` back-to-back calls (the composition syncs with the host in
its mask indexing, which is part of what it costs).  Prints one JSON line per vocabulary size.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="+", default=[32000, 128000])
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--sampler", default="0.8,40,0.95")
    ap.add_argument("--dtype", default="bfloat16")
    a = ap.parse_args()
    from scaling_amd.ops.sample import sample_logits
    from scaling_amd.transformer.inference import sample_temperature, top_k_transform, top_p_transform

    temp, top_k, top_p = (lambda s: (float(s[0]), int(s[1]), float(s[2])))(a.sampler.split(","))
    dtype = getattr(torch, a.dtype)
    dev = torch.device("cuda", 0)
    step = torch.zeros(1, dtype=torch.long, device=dev)

    def fused(x):
        return sample_logits(x, step, 0, temp, top_k, top_p)

    def fused_plain(x):
        return sample_logits(x, step, 0, 1.0, 0, 1.0)

    def argmax(x):
        return torch.argmax(x, dim=-1)

    def composed(x):
        return sample_temperature(top_p_transform(top_k_transform(x[0], top_k), top_p)[None, None], temp)

    def timed(fn, rows, iters):
        n = rows.shape[0]
        for i in range(min(iters, 20)):
            fn(rows[i % n][None])
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(iters):
            fn(rows[i % n][None])
        e1.record()
        torch.cuda.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / iters  # microseconds per call

    for V in a.vocab:
        torch.manual_seed(V)
        n_cold = (640 << 20) // (V * torch.finfo(dtype).bits // 8) + 1
        rows = (torch.randn(n_cold, V, device=dev) * 3.0).to(dtype)
        res = {"metric": "batch-1 sampling step, microseconds per call", "vocab": V, "dtype": a.dtype,
               "sampler": a.sampler, "iters": a.iters, "cold_rows": n_cold}
        for name, fn, it in (("fused", fused, a.iters), ("fused_no_filter", fused_plain, a.iters),
                             ("argmax", argmax, a.iters), ("torch_composition", composed, max(a.iters // 10, 50))):
            res[f"{name}_warm_us"] = round(timed(fn, rows[:1], it), 2)
            res[f"{name}_cold_us"] = round(timed(fn, rows, it), 2)
        print(json.dumps(res), flush=True)
        del rows


if __name__ == "__main__":
    main()
