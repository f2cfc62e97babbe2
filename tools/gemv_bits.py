"""Bit fingerprint of the decode GEMV entry points (``csrc/kernels/gemv.hip``: gemv / gemv_residual / gemv_swiglu /
gemv_norm / gemv_norm_rope over bf16 and fp16 weights, and every ``gemv_w8*`` form over FP8 weights) on fixed-seed
inputs at the tests' shapes -- M = 1..4, one wave per row and four, full / tail-only / ragged trips, bias, a
row-strided weight view and a row-strided x: run it under two builds (``SCALING_AMD_EXT_SO``) and diff the printed
lines to check that a kernel change is bit-identical.  The same for the MFMA kernel's entry points
(``csrc/kernels/skinny.hip``, ``skinny*`` / ``skinny_w8*``) at M = 1, 5, 16 and one shape per launch rule.
The MXFP4 entry points (``gemv_w4*`` / ``skinny_w4*``) follow as lines tagged ``w4`` when the build has them, at the
same shapes with K rounded up to a multiple of 32.

usage: python tools/gemv_bits.py
"""
import hashlib
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scaling_amd.ops import quant  # noqa: E402
from scaling_amd.ops._ext import ext  # noqa: E402

DEV = "cuda"
SHAPES = [(5, 16), (77, 64), (1003, 208), (64, 4112), (2064, 4112), (256, 1024)]  # (N, K)
DENSE_ONLY = [(5, 8), (1003, 200)]  # K % 16 != 0


def digest(t: torch.Tensor) -> str:
    return hashlib.sha1(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:12]


def randn(seed, *shape, dt=torch.bfloat16):
    return torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)).to(dt)


def weight(seed, N, K, dt):
    return (randn(seed, N, K, dt=torch.float32) / math.sqrt(K)).to(dt)


def strided(t, pad, off):
    """t as a row-strided view of a buffer ``pad`` columns wider, starting at column ``off``"""
    wide = torch.zeros(t.shape[0], t.shape[1] + pad, device=DEV, dtype=torch.uint8 if t.element_size() == 1 else t.dtype)
    view = wide[:, off : off + t.shape[1]]
    view.copy_(t.view(wide.dtype))
    return view.view(t.dtype)


def run(dt, fp8: bool, rope: bool, all_paths: bool) -> None:
    tag = "w8" if fp8 else {torch.bfloat16: "bf16", torch.float16: "fp16"}[dt]
    e = ext()
    fn = lambda name: getattr(e, name.replace("gemv", "gemv_w8", 1) if fp8 else name)  # noqa: E731
    wargs = lambda w: quant.quantize_rows_fp8(w) if fp8 else (w,)  # noqa: E731

    for N, K in SHAPES + ([] if fp8 else DENSE_ONLY):
        wa = wargs(weight(N + K, N, K, dt))
        wv = (strided(wa[0], 64, 32),) + tuple(wa[1:])
        for M in (1, 2, 3, 4):
            x = randn(7 * N + K + M, M, K, dt=dt)
            xs = strided(x, 24, 8)
            for b in (None, randn(3 * N + 1, N, dt=dt)):
                y = [fn("gemv")(xx, *ww, b) for xx, ww in ((x, wa), (x, wv), (xs, wa))]
                print(f"{tag} gemv N={N} K={K} M={M} bias={b is not None}: y {digest(y[0])} wview {digest(y[1])} "
                      f"xview {digest(y[2])}", flush=True)

    K = 528
    if all_paths:
        for M in (1, 2, 3, 4):
            x = randn(100 + M, M, K, dt=dt)
            for N in (136, 528):  # K-split (N <= 8192 and K >= 2 N) and one wave per row
                y = fn("gemv_residual")(x, *wargs(weight(7 + N, N, K, dt)), randn(4 * N + M, M, N, dt=dt))
                print(f"{tag} gemv_residual N={N} K={K} M={M}: y {digest(y)}", flush=True)
            F = 136
            w = weight(11, 2 * F, K, torch.float32)
            w[F:] *= 16  # the up half on its own row scales
            y = fn("gemv_swiglu")(x, *wargs(w.to(dt)))
            print(f"{tag} gemv_swiglu F={F} K={K} M={M}: y {digest(y)}", flush=True)

    for K in (528, 4112):
        gam = (1 + 0.1 * randn(3 * K, K, dt=torch.float32)).to(dt)
        for N in (264, 263):  # two rows per wave, and one
            F = N // 2 if N % 2 == 0 else N
            ws = {0: wargs(weight(N + K, N, K, dt)), 2: wargs(weight(5 + N + K, 2 * F, K, dt))}
            for M in (1, 2, 3, 4):
                x, add = randn(N + K + M, M, K, dt=dt), randn(2 * (N + K) + M, M, K, dt=dt)
                for a in (None, add):
                    for epi in (0, 2):
                        s, y = fn("gemv_norm")(x, a, gam, 1e-5, *ws[epi], epi)
                        print(f"{tag} gemv_norm N={N} K={K} M={M} add={a is not None} epi={epi}: s {digest(s)} "
                              f"y {digest(y)}", flush=True)

    if rope:
        nq, nkv, hd, K, cap = 8, 2, 128, 1024, 64
        x, gam = randn(1, 1, K, dt=dt), (1 + 0.1 * randn(2, K, dt=torch.float32)).to(dt)
        w = weight(3, (nq + 2 * nkv) * hd, K, dt)
        for rd in (hd, hd // 2):
            inv = 1.0 / (10000 ** (torch.arange(0, rd // 2, device=DEV, dtype=torch.float32) / (rd // 2)))
            ang = torch.arange(cap, device=DEV, dtype=torch.float32)[:, None] * inv[None]
            cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
            for pos in (29, cap):  # in range, and one past the cache
                kc, vc = randn(4, cap, nkv, hd, dt=dt), randn(5, cap, nkv, hd, dt=dt)
                err = torch.zeros(1, device=DEV, dtype=torch.int32)
                q = e.gemv_norm_rope(x, gam, 1e-5, w, cos, sin, torch.tensor([pos], device=DEV), nq, nkv, rd, kc, vc, err)
                print(f"{tag} gemv_norm_rope rd={rd} pos={pos}: q {digest(q)} kc {digest(kc)} vc {digest(vc)} "
                      f"err {int(err.item())}", flush=True)


def run_skinny(dt, fp8: bool) -> None:
    tag = "w8" if fp8 else {torch.bfloat16: "bf16", torch.float16: "fp16"}[dt]
    fn = lambda name: getattr(ext(), name.replace("skinny", "skinny_w8", 1) if fp8 else name)  # noqa: E731
    wargs = lambda w: quant.quantize_rows_fp8(w) if fp8 else (w,)  # noqa: E731
    # the tests' plain shapes, then one per launch rule: K split x 1 tile, K split x 2 tiles, no K split
    for N, K in [(5, 16), (1003, 208), (64, 4112), (263, 528), (136, 528), (8200, 64), (32781, 64)]:
        wa, w2 = wargs(weight(N + K, N, K, dt)), wargs(weight(5 + N + K, 2 * N, K, dt))
        wv = (strided(wa[0], 64, 32),) + tuple(wa[1:])
        gam = (1 + 0.1 * randn(3 * K, K, dt=torch.float32)).to(dt)
        for M in (1, 5, 16):
            x, add = randn(7 * N + K + M, M, K, dt=dt), randn(2 * (N + K) + M, M, K, dt=dt)
            b, res = randn(3 * N + 1, N, dt=dt), randn(4 * N + M, M, N, dt=dt)
            y = [fn("skinny")(xx, *ww, bb) for xx, ww, bb in ((x, wa, None), (x, wa, b), (x, wv, b), (strided(x, 24, 8), wa, b))]
            print(f"{tag} skinny N={N} K={K} M={M}: y {digest(y[0])} bias {digest(y[1])} wview {digest(y[2])} "
                  f"xview {digest(y[3])}", flush=True)
            print(f"{tag} skinny_residual N={N} K={K} M={M}: y {digest(fn('skinny_residual')(x, *wa, res))}", flush=True)
            print(f"{tag} skinny_swiglu F={N} K={K} M={M}: y {digest(fn('skinny_swiglu')(x, *w2))}", flush=True)
            for a in (None, add):
                for epi, ww in ((0, wa), (2, w2)):
                    s, yn = fn("skinny_norm")(x, a, gam, 1e-5, *ww, epi)
                    print(f"{tag} skinny_norm N={N} K={K} M={M} add={a is not None} epi={epi}: s {digest(s)} "
                          f"y {digest(yn)}", flush=True)


def run_w4() -> None:
    e = ext()
    up = lambda k: -(-k // 32) * 32  # noqa: E731
    q4 = lambda seed, N, K: quant.quantize_rows_mxfp4(weight(seed, N, K, torch.bfloat16))  # noqa: E731
    for kind, rows in (("gemv", (1, 2, 3, 4)), ("skinny", (1, 5, 16))):
        fn = lambda name: getattr(e, kind + "_w4" + name)  # noqa: E731
        shapes = SHAPES + [(136, 528)] if kind == "gemv" else [(5, 16), (1003, 208), (64, 4112), (263, 528), (136, 528),
                                                                (8200, 64), (32781, 64)]
        for N, K in [(n, up(k)) for n, k in shapes]:
            wa, w2 = q4(N + K, N, K), q4(5 + N + K, 2 * N, K)
            gam = (1 + 0.1 * randn(3 * K, K, dt=torch.float32)).to(torch.bfloat16)
            for M in rows:
                x, add = randn(7 * N + K + M, M, K), randn(2 * (N + K) + M, M, K)
                b, res = randn(3 * N + 1, N), randn(4 * N + M, M, N)
                y = [fn("")(xx, *wa, bb) for xx, bb in ((x, None), (x, b), (strided(x, 24, 8), b))]
                print(f"w4 {kind} N={N} K={K} M={M}: y {digest(y[0])} bias {digest(y[1])} xview {digest(y[2])}", flush=True)
                print(f"w4 {kind}_residual N={N} K={K} M={M}: y {digest(fn('_residual')(x, *wa, res))}", flush=True)
                print(f"w4 {kind}_swiglu F={N} K={K} M={M}: y {digest(fn('_swiglu')(x, *w2))}", flush=True)
                for a in (None, add):
                    for epi, ww in ((0, wa), (2, w2)):
                        s, yn = fn("_norm")(x, a, gam, 1e-5, *ww, epi)
                        print(f"w4 {kind}_norm N={N} K={K} M={M} add={a is not None} epi={epi}: s {digest(s)} "
                              f"y {digest(yn)}", flush=True)


run(torch.bfloat16, fp8=False, rope=True, all_paths=True)
run(torch.float16, fp8=False, rope=False, all_paths=False)  # the plain and NORM cases
run(torch.bfloat16, fp8=True, rope=False, all_paths=True)
run_skinny(torch.bfloat16, fp8=False)
run_skinny(torch.float16, fp8=False)
run_skinny(torch.bfloat16, fp8=True)
if hasattr(ext(), "gemv_w4"):
    run_w4()
torch.cuda.synchronize()
