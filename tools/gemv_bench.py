"""Decode GEMV micro-benchmark on one GPU: the 7B decode projections (q/k/v, o, gate/up, down, head) at batch 1
through the plain, epilogue-fused and norm-prologue GEMV kernels; prints us per call and the weight-stream rate.

``FP8=1``: the FP8-weight kernels (``csrc/kernels/gemv.hip``) of the decode step, each right after its bf16
counterpart, in the same process, on the same shapes and under the same cold-cache protocol (``PASSES`` alternating
passes over the list, default 2 with FP8); the rate counts the bytes each kernel streams (codes + row scales).
``MXFP4=1`` (implies ``FP8=1``): the MXFP4-weight kernels follow their FP8 counterparts in the same way; their rate
counts codes plus block-scale bytes (0.53125 bytes per weight).

``W4_RULES=1``: the A/B behind the MXFP4 GEMV's launch rules -- the five decode forms at batch 1 under every candidate
(rows per wave, waves per row), forced through ``ext().gemv_w4_rule``, ``PASSES`` (default 2) alternating passes.

``SKINNY=1``: the MFMA weight-streaming kernel (``csrc/kernels/skinny.hip``) at M = 1, 2, 3, 4, 8, 16 rows on the five 7B
shapes in the forms the decode step runs them, each right beside its counterpart -- the GEMV at M <= 4, ``F.linear``
(the library GEMM alone, without the norm / SwiGLU / residual the fused forms include) at M = 8 and 16 -- bf16 and
FP8 (``SKINNY_FORMATS=bf16`` for one of them; ``SKINNY_FORMATS=bf16,fp8,mxfp4`` adds the MXFP4 forms, ``SKINNY_ROWS``
such as ``1,4,16`` picks the row counts), same process, same cold-cache protocol, ``PASSES`` (default 2) alternating
passes."""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, reps: int = 200) -> float:
    for _ in range(10):
        fn(0)
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


def copies(shape, dev, dt, cold: bool):
    """Weight copies cycled through by the timed loop: > 1 GiB in total when cold, so every call streams its weight
    from HBM (the 256 MiB last-level cache holds a single 7B projection otherwise)."""
    nb = shape[0] * shape[1] * 2
    n = max(2, -(-(1 << 30) // nb)) if cold else 1
    return [torch.randn(*shape, device=dev, dtype=dt) / 64 for _ in range(n)]


def copies8(shape, dev, cold: bool):
    """FP8 copies ``(q, scale)`` under the same protocol: > 1 GiB of codes in total when cold."""
    from scaling_amd.ops.quant import quantize_rows_fp8

    n = max(2, -(-(1 << 30) // (shape[0] * shape[1]))) if cold else 1
    return [quantize_rows_fp8(torch.randn(*shape, device=dev, dtype=torch.bfloat16) / 64) for _ in range(n)]


def copies4(shape, dev, cold: bool):
    """MXFP4 copies ``(codes, scales)`` under the same protocol: > 1 GiB of codes in total when cold."""
    from scaling_amd.ops.quant import quantize_rows_mxfp4

    n = max(2, -(-(1 << 30) // (shape[0] * shape[1] // 2))) if cold else 1
    first = quantize_rows_mxfp4(torch.randn(*shape, device=dev, dtype=torch.bfloat16) / 64)
    # (the timing does not depend on the values: the further copies are permuted clones, which spares the quantiser)
    return [first] + [(first[0].roll(i + 1, 0), first[1].roll(i + 1, 0)) for i in range(n - 1)]


def w4_rules_main() -> None:
    from scaling_amd.ops._ext import ext

    torch.manual_seed(0)
    dev, dt = "cuda", torch.bfloat16
    H, F, V = 4096, 11008, 32000
    g = torch.ones(H, device=dev, dtype=dt)
    x, add = torch.randn(1, H, device=dev, dtype=dt), torch.randn(1, H, device=dev, dtype=dt)
    a = torch.randn(1, F, device=dev, dtype=dt)
    W = lambda ws, i: ws[i % len(ws)]  # noqa: E731
    layers = [("qkv norm", (3 * H, H)), ("o residual", (H, H)), ("gate/up norm swiglu", (2 * F, H)),
              ("down residual", (H, F)), ("head", (V, H))]
    rules = [(0, 0), (1, 1), (2, 1), (4, 1), (1, 4), (2, 4), (4, 4)]
    print("MXFP4 GEMV launch rules A/B, batch 1, cold; rule (0, 0) = the kernel's own", flush=True)
    for name, shape in layers:
        ws = copies4(shape, dev, True)
        nb = sum(t.numel() for t in ws[0])
        fn = {"qkv norm": lambda i: ext().gemv_w4_norm(x, None, g, 1e-5, *W(ws, i), 0),
              "o residual": lambda i: ext().gemv_w4_residual(x, *W(ws, i), add),
              "gate/up norm swiglu": lambda i: ext().gemv_w4_norm(x, add, g, 1e-5, *W(ws, i), 2),
              "down residual": lambda i: ext().gemv_w4_residual(a, *W(ws, i), add),
              "head": lambda i: ext().gemv_w4(x, *W(ws, i), None)}[name]
        for p in range(int(os.environ.get("PASSES", "2"))):
            for rpw, ks in rules:
                ext().gemv_w4_rule(rpw, ks)
                us = timeit(fn)
                print(f"{name:20s} pass {p} rows/wave {rpw} waves/row {ks}  {us:8.2f} us  {nb / us / 1e6:6.2f} TB/s", flush=True)
        ext().gemv_w4_rule(0, 0)
        del ws
        torch.cuda.empty_cache()


def main() -> None:
    from scaling_amd.ops._ext import ext
    from scaling_amd.ops import norm as norm_ops

    torch.manual_seed(0)
    dev, dt = "cuda", torch.bfloat16
    H, F, M = 4096, 11008, int(os.environ.get("ROWS", "1"))
    x = torch.randn(M, H, device=dev, dtype=dt)
    add = torch.randn(M, H, device=dev, dtype=dt)
    g = torch.ones(H, device=dev, dtype=dt)
    cold = os.environ.get("COLD", "1") != "0"
    wqkv = copies((3 * H, H), dev, dt, cold)
    wo = copies((H, H), dev, dt, cold)
    wgu = copies((2 * F, H), dev, dt, cold)
    wd = copies((H, F), dev, dt, cold)
    a = torch.randn(M, F, device=dev, dtype=dt)
    V = 32000
    wh = copies((V, H), dev, dt, cold)
    W = lambda ws, i: ws[i % len(ws)]  # noqa: E731
    cases = [
        ("norm_row (rmsnorm, 1 launch)", lambda i: norm_ops.add_rms_norm(x, add, g, 1e-5), None),
        ("qkv gemv", lambda i: ext().gemv(x, W(wqkv, i), None), wqkv),
        ("qkv gemv_norm", lambda i: ext().gemv_norm(x, None, g, 1e-5, W(wqkv, i), 0), wqkv),
        ("o gemv_residual", lambda i: ext().gemv_residual(x, W(wo, i), add), wo),
        ("gate/up gemv (plain, 2F rows)", lambda i: ext().gemv(x, W(wgu, i), None), wgu),
        ("gate/up gemv_swiglu", lambda i: ext().gemv_swiglu(x, W(wgu, i)), wgu),
        ("gate/up gemv_norm swiglu", lambda i: ext().gemv_norm(x, add, g, 1e-5, W(wgu, i), 2), wgu),
        ("down gemv_residual", lambda i: ext().gemv_residual(a, W(wd, i), add), wd),
        ("head gemv", lambda i: ext().gemv(x, W(wh, i), None), wh),
    ]
    mx = os.environ.get("MXFP4", "0") != "0"
    fp8 = os.environ.get("FP8", "0") != "0" or mx
    if fp8:
        q_qkv, q_o, q_gu = copies8((3 * H, H), dev, cold), copies8((H, H), dev, cold), copies8((2 * F, H), dev, cold)
        q_d, q_h = copies8((H, F), dev, cold), copies8((V, H), dev, cold)
        after = {
            "qkv gemv_norm": ("qkv gemv_w8_norm", lambda i: ext().gemv_w8_norm(x, None, g, 1e-5, *W(q_qkv, i), 0), q_qkv),
            "o gemv_residual": ("o gemv_w8_residual", lambda i: ext().gemv_w8_residual(x, *W(q_o, i), add), q_o),
            "gate/up gemv_norm swiglu": ("gate/up gemv_w8_norm swiglu",
                                         lambda i: ext().gemv_w8_norm(x, add, g, 1e-5, *W(q_gu, i), 2), q_gu),
            "down gemv_residual": ("down gemv_w8_residual", lambda i: ext().gemv_w8_residual(a, *W(q_d, i), add), q_d),
            "head gemv": ("head gemv_w8", lambda i: ext().gemv_w8(x, *W(q_h, i), None), q_h),
        }
        after4 = {}
        if mx:
            c_qkv, c_o, c_gu = copies4((3 * H, H), dev, cold), copies4((H, H), dev, cold), copies4((2 * F, H), dev, cold)
            c_d, c_h = copies4((H, F), dev, cold), copies4((V, H), dev, cold)
            after4 = {
                "qkv gemv_norm": ("qkv gemv_w4_norm", lambda i: ext().gemv_w4_norm(x, None, g, 1e-5, *W(c_qkv, i), 0), c_qkv),
                "o gemv_residual": ("o gemv_w4_residual", lambda i: ext().gemv_w4_residual(x, *W(c_o, i), add), c_o),
                "gate/up gemv_norm swiglu": ("gate/up gemv_w4_norm swiglu",
                                             lambda i: ext().gemv_w4_norm(x, add, g, 1e-5, *W(c_gu, i), 2), c_gu),
                "down gemv_residual": ("down gemv_w4_residual", lambda i: ext().gemv_w4_residual(a, *W(c_d, i), add), c_d),
                "head gemv": ("head gemv_w4", lambda i: ext().gemv_w4(x, *W(c_h, i), None), c_h),
            }
        cases = [c for case in cases
                 for c in ([case, after[case[0]]] + ([after4[case[0]]] if mx else []) if case[0] in after else [case])]
    print(f"rows {M}, {'cold (weights cycled through > 1 GiB)' if cold else 'warm (one weight copy)'}", flush=True)
    for p in range(int(os.environ.get("PASSES", "2" if fp8 else "1"))):
        if fp8:
            print(f"pass {p}", flush=True)
        for name, fn, w in cases:
            us = timeit(fn)
            w0 = w[0] if w is not None else None
            nb = sum(t.numel() * t.element_size() for t in (w0 if isinstance(w0, tuple) else (w0,))) if w0 is not None else 0
            print(f"{name:34s} {us:8.2f} us  {nb / us / 1e6 if nb else 0:6.2f} TB/s", flush=True)


def skinny_main() -> None:
    from scaling_amd.ops._ext import ext

    torch.manual_seed(0)
    dev, dt = "cuda", torch.bfloat16
    H, F, V = 4096, 11008, 32000
    cold = os.environ.get("COLD", "1") != "0"
    g = torch.ones(H, device=dev, dtype=dt)
    W = lambda ws, i: ws[i % len(ws)]  # noqa: E731
    # (name, weight shape, K, form); forms: n0 = norm + plain, n2 = add + norm + SwiGLU, res = + residual, plain
    layers = [("qkv norm", (3 * H, H), "n0"), ("o residual", (H, H), "res"), ("gate/up norm swiglu", (2 * F, H), "n2"),
              ("down residual", (H, F), "res"), ("head", (V, H), "plain")]
    print(f"skinny vs gemv / F.linear, {'cold (weights cycled through > 1 GiB)' if cold else 'warm (one weight copy)'}",
          flush=True)
    for fmt in os.environ.get("SKINNY_FORMATS", "bf16,fp8").split(","):
        for name, shape, form in layers:
            ws = copies(shape, dev, dt, cold) if fmt == "bf16" else copies8(shape, dev, cold) if fmt == "fp8" else copies4(shape, dev, cold)
            w0 = ws[0]
            nb = sum(t.numel() * t.element_size() for t in (w0 if isinstance(w0, tuple) else (w0,)))
            wl = copies(shape, dev, dt, cold) if fmt != "bf16" else ws  # F.linear streams bf16 either way
            N, K = shape
            for p in range(int(os.environ.get("PASSES", "2"))):
                for M in (int(r) for r in os.environ.get("SKINNY_ROWS", "1,2,3,4,8,16").split(",")):
                    x = torch.randn(M, K, device=dev, dtype=dt)
                    add = torch.randn(M, K, device=dev, dtype=dt)
                    res = torch.randn(M, N, device=dev, dtype=dt)

                    def call(kind, i, M=M, x=x, add=add, res=res):
                        w = W(ws, i)
                        wa = w if isinstance(w, tuple) else (w,)
                        pre = kind + {"bf16": "", "fp8": "_w8", "mxfp4": "_w4"}[fmt]
                        if form == "n0":
                            return getattr(ext(), pre + "_norm")(x, None, g, 1e-5, *wa, 0)
                        if form == "n2":
                            return getattr(ext(), pre + "_norm")(x, add, g, 1e-5, *wa, 2)
                        if form == "res":
                            return getattr(ext(), pre + "_residual")(x, *wa, res)
                        return getattr(ext(), pre)(x, *wa, None)

                    row = [("skinny", timeit(lambda i: call("skinny", i)))]
                    if M <= 4:
                        row.append(("gemv", timeit(lambda i: call("gemv", i))))
                    else:
                        row.append(("F.linear(bf16)", timeit(lambda i: torch.nn.functional.linear(x, W(wl, i)))))
                    cells = "  ".join(f"{k} {us:7.2f} us {(nb if k != 'F.linear(bf16)' else N * K * 2) / us / 1e6:5.2f} TB/s"
                                      for k, us in row)
                    print(f"{fmt} {name:20s} pass {p} M={M:2d}  {cells}", flush=True)
            del ws, wl
            torch.cuda.empty_cache()


if __name__ == "__main__":
    if os.environ.get("W4_RULES", "0") != "0":
        w4_rules_main()
    elif os.environ.get("SKINNY", "0") != "0":
        skinny_main()
    else:
        main()
