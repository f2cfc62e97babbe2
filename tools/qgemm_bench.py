"""Prefill GEMM over quantised weights (``ext().qgemm_w8`` / ``qgemm_w4``, ``csrc/kernels/qgemm.hip``) against the
library GEMM on the dequantised bf16 weights (``ext().lt_linear``: cached hipBLASLt plans) at the 7B layer shapes, M =
128, 512, 2048 and 4096.  Same process, cold cache (every call takes the next of several weight copies, > 1 GiB of bf16
in total per shape), the two kernels alternating, ``PASSES`` (default 2) passes.  ``REPS`` calls per timing (default 20),
timed with events around the eager loop (a hipBLASLt plan cannot be made inside a graph capture).

    python tools/qgemm_bench.py | tee profiles/qgemm_bench.log
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, reps: int) -> float:
    for i in range(3):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps


def main() -> None:
    from scaling_amd.ops import quant
    from scaling_amd.ops._ext import ext

    dev = torch.device("cuda")
    H, F, V = 4096, 11008, 32000
    layers = [("qkv", 3 * H, H), ("o", H, H), ("gate/up", 2 * F, H), ("down", H, F), ("head", V, H)]
    reps, passes = int(os.environ.get("REPS", "20")), int(os.environ.get("PASSES", "2"))
    print(f"qgemm vs lt_linear, cold (weights cycled through > 1 GiB of bf16), {reps} calls per timing", flush=True)
    for name, N, K in layers:
        n = max(2, -(-(1 << 30) // (N * K * 2)))
        w = torch.randn(N, K, device=dev, dtype=torch.bfloat16) / 64
        q8, s8 = quant.quantize_rows_fp8(w)
        c4, s4 = quant.quantize_rows_mxfp4(w)
        del w
        # (the timing does not depend on the values: the further copies are clones)
        fmts = {
            "w8": ([(q8.clone(), s8.clone()) for _ in range(n)], [quant.dequantize_rows_fp8(q8, s8) for _ in range(n)]),
            "w4": ([(c4.clone(), s4.clone()) for _ in range(n)], [quant.dequantize_rows_mxfp4(c4, s4) for _ in range(n)]),
        }
        for fmt, (qs, ds) in fmts.items():
            fn_q = getattr(ext(), "qgemm_" + fmt)
            for M in (128, 512, 2048, 4096):
                xs = [torch.randn(M, K, device=dev, dtype=torch.bfloat16) for _ in range(4)]
                y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
                if ext().lt_linear(xs[0], ds[0], None, y) is not None:
                    lib = lambda i: ext().lt_linear(xs[i % 4], ds[i % n], None, y)  # noqa: E731
                else:  # no cached plan for this product: the same library through torch
                    lib = lambda i: torch.matmul(xs[i % 4], ds[i % n].t(), out=y)  # noqa: E731
                for p in range(passes):
                    us_l = timeit(lib, reps)
                    us_q = timeit(lambda i: fn_q(xs[i % 4], *qs[i % n], None, y), reps)
                    tf = 2.0 * M * N * K / 1e6
                    print(f"{name:8s} {fmt} M {M:5d} pass {p}  lt_linear {us_l:9.1f} us {tf / us_l:7.1f} TF/s   "
                          f"qgemm {us_q:9.1f} us {tf / us_q:7.1f} TF/s   ratio {us_q / us_l:5.2f}", flush=True)
        del fmts


if __name__ == "__main__":
    main()
