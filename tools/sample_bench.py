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


def rows_mode(a, dtype, dev, temp, top_k, top_p) -> None:
    """``--rows``: ``sample_rows`` (no penalties; repetition + presence penalty over a full ``--history``-token
    history) against ``sample_logits`` on the same logits, B rows per call, warm and cold, the three alternating in one
    process for ``--rounds`` rounds; one JSON line per (vocabulary, B) with every round's figures (their spread is the
    run-to-run noise)."""
    from scaling_amd.ops.sample import sample_logits, sample_rows
    from scaling_amd.transformer.inference import RequestSampler, SamplingParams

    step = torch.zeros(1, dtype=torch.long, device=dev)
    for V in a.vocab:
        for B in a.batch:
            torch.manual_seed(V)
            n_cold = (640 << 20) // (B * V * torch.finfo(dtype).bits // 8) + 1
            x = (torch.randn(n_cold, B, V, device=dev) * 3.0).to(dtype)
            samplers = {}
            for name, pen in (("rows", False), ("rows_history", True)):
                rs = RequestSampler(B, a.history, dev)  # a full history: every call sees the same tokens
                for b in range(B):
                    rs.set_row(b, SamplingParams(temp, top_k, top_p, seed=b, repetition_penalty=1.3 if pen else 1.0,
                                                 presence_penalty=0.5 if pen else 0.0),
                               torch.randint(0, V, (a.history,)).tolist())
                samplers[name] = rs
            fns = {"scalar": lambda t: sample_logits(t, step, 0, temp, top_k, top_p),
                   "rows": lambda t: sample_rows(t, samplers["rows"].table),
                   "rows_history": lambda t: sample_rows(t, samplers["rows_history"].table)}
            res = {"metric": "sampling step, microseconds per call", "vocab": V, "rows": B, "dtype": a.dtype,
                   "sampler": a.sampler, "history": a.history, "iters": a.iters}
            for name in fns:
                res[f"{name}_warm_us"], res[f"{name}_cold_us"] = [], []
            for _ in range(a.rounds):
                for name, fn in fns.items():
                    for kind, data in (("warm", x[:1]), ("cold", x)):
                        n = data.shape[0]
                        for i in range(20):
                            fn(data[i % n])
                        torch.cuda.synchronize()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for i in range(a.iters):
                            fn(data[i % n])
                        e1.record()
                        torch.cuda.synchronize()
                        res[f"{name}_{kind}_us"].append(round(1000.0 * e0.elapsed_time(e1) / a.iters, 2))
            print(json.dumps(res), flush=True)
            del x


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, nargs="+", default=[32000, 128000])
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--sampler", default="0.8,40,0.95")
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--rows", action="store_true", help="the row-table form (sample_rows) against sample_logits")
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--history", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
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

    if a.rows:
        rows_mode(a, dtype, dev, temp, top_k, top_p)
        return
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
