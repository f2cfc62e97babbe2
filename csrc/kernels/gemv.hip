// Decode-time linear layer on gfx950:  y[M, N] = x[M, K] W[N, K]^T (+ b)  for M <= 4 input rows.
//
// Token-by-token generation runs every linear layer at M = 1: the layer is a weight stream (2 bytes of W per
// 2 FLOPs), and hipBLASLt's GEMM tiles move it at ~1.1 TB/s on the 7B decode step.  Here W is streamed once at
// full width (cdna_hip_programming.md, "GEMV / M <= 16 decode weights": straight to VGPRs, deep unroll, late wait):
//  * one wave per output row n (or four waves splitting K, see gemv_kernel), all M inputs at once; lanes split K
//    in 16-byte pieces (8 elements), four pieces per lane in flight per trip (4 KiB per wave), fp32 FMAs;
//  * x is tiny (M x K) and re-read by every wave from L1/L2 (at M <= 4 its L1 traffic stays within the CU's
//    load bandwidth);
//  * one wave reduction per (row, input) at the end; bias added in fp32, one rounding to the output type.
// Decode epilogues (each removes one latency-bound launch per layer and token from the graph-decode step):
//  * RES: y = rnd(rnd(x W^T) + res)   -- the residual add after the MLP down projection (torch's bf16 add order);
//  * SWIGLU: W holds [gate; up] (2F rows); the wave streams rows n and F + n and writes
//    y[:, n] = rnd(rnd(silu(g)) * u) with g, u rounded as the unfused GEMV stores them -- bit-identical to
//    gemv + swiglu_fwd_kernel.
// Decode prologue (NORM): the RMSNorm in front of the projection (optionally after the residual add
// s = rnd(x + add)) runs inside the same single pass over the weights.  Every wave already reads all of x, so it
// also accumulates sum(s^2) and dots the weights with s * gamma; the row's rstd scales the dot product at the end:
//     y = rstd * sum_k w_k s_k gamma_k      (fp32; the unfused path rounds s * rstd and * gamma to bf16 first)
// No prologue pass, no barrier, no extra launch: the two latency-bound norm launches per layer and token go away.
// The wave that owns output row 0 also writes s (the new residual stream).  Eager and graph decoding both run this
// kernel, so their tokens stay identical; against norm + GEMV it differs by the two skipped bf16 roundings.
//
// FP8 weights (E4M3W):  W = scale[n] * Q[n, :], Q OCP e4m3fn codes, one byte per weight, scale one fp32 power of two
// per output row (scaling_amd/ops/quant.py), so the layer streams half the bytes of its bf16 form.  The same kernel
// body, same launch rules, same rounding points; the weight format only changes
//  * the piece: still 16 bytes per lane, which is now 16 weights: K % 16 == 0, two 16-byte loads of x (and of
//    gamma / add for the NORM prologue) per piece and input row;
//  * the decoding: the codes stay raw across the trip and are converted two at a time by the hardware
//    (v_cvt_pk_f32_fp8, __builtin_amdgcn_cvt_pk_f32_fp8), once per piece and weight row, and reused by all M
//    inputs; products and sums are fp32 as before;
//  * the row scale, which multiplies the dot product ONCE per output row, after the wave / K-split reduction and
//    before rstd, the bias and the epilogue: a power of two, so the result is the dot product with the dequantised
//    bf16 weights up to the order of the fp32 sums.  SwiGLU: rows n and F + n each take their own scale.
// FP8 weights take bf16 activations only, and the one-launch RoPE step (EPI_ROPE) has no FP8 form.
//
// MXFP4 weights (MXFP4W):  OCP e2m1 codes, two per byte (even k in the low nibble), in blocks of 32 consecutive k of a
// row with one e8m0 scale byte b per block, value 2^(b - 127) (scaling_amd/ops/quant.py): 0.53125 bytes per weight.
// The same kernel, forms, epilogues and rounding points, with a streaming loop of its own (gemv_rows_w4); the format
// changes
//  * the piece: 16 bytes per lane are 32 weights = exactly ONE block: K % 32 == 0, four 16-byte loads of x (and of
//    gamma / add) per piece and input row; the block's scale byte is loaded with the piece and becomes the float
//    with the bits b << 23 (the quantiser never makes b = 0 or 255);
//  * the decoding: 8-weight sub-steps, one dword of codes each (never 32 floats per weight row), two codes per
//    v_cvt_scalef32_pk_f32_fp4 with the block scale applied by the instruction, so code * scale -- exactly the
//    dequantised bf16 weight -- enters the fp32 FMA and nothing is left to scale after the reduction;
//  * the launch rules, which are the format's own (w4_rules): at 4 bits a row is a quarter of the pieces.
// bf16 activations only, no EPI_ROPE form.
#include "common.h"
#include "launch.h"

#include <cstdlib>

using namespace sa;

namespace {

enum { EPI_NONE = 0, EPI_RES = 1, EPI_SWIGLU = 2, EPI_ROPE = 3 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Weight formats: T the element type of W's pointer arithmetic (ldw counts T's), P = 1 << kLog2P weights per 16-byte
// piece, S one piece as it is held across a trip (ld) until piece() turns it into P floats (unpack); ST the type of
// the scales: one fp32 per row (kScaled) or one byte per piece (kBlock, which has its own streaming loop below).
// Weights of the activation type E: converted to float at load time (staging them raw reschedules the whole kernel).
template <typename E>
struct DenseW {
    typedef E T;
    typedef float S[8];
    static constexpr int kLog2P = 3, P = 8;
    static constexpr bool kScaled = false, kBlock = false;
    typedef float ST;
    __device__ static __forceinline__ void ld(const E* p, S& s) { V8<E>::ld(p, s); }
    __device__ static __forceinline__ void unpack(const S& s, float (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = s[i];
    }
};
// e4m3fn codes with one fp32 scale per row (kScaled): 16 codes -> 16 floats, in memory order
struct E4M3W {
    typedef uint8_t T;
    typedef u32x4 S;
    static constexpr int kLog2P = 4, P = 16;
    static constexpr bool kScaled = true, kBlock = false;
    typedef float ST;
    __device__ static __forceinline__ void ld(const uint8_t* p, S& s) { s = *reinterpret_cast<const u32x4*>(p); }
    __device__ static __forceinline__ void unpack(const S& r, float (&v)[16]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[i], false);
            const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[i], true);
            v[4 * i] = lo[0];
            v[4 * i + 1] = lo[1];
            v[4 * i + 2] = hi[0];
            v[4 * i + 3] = hi[1];
        }
    }
};

// e2m1 codes, 32 per piece = one MX block with its e8m0 scale byte (kBlock): sub-step h is dword h, 8 codes -> 8 scaled
// floats in memory order (the low nibble of a byte is the even k)
struct MXFP4W {
    typedef uint8_t T;
    struct S {
        u32x4 c;
        float s;
    };
    typedef uint8_t ST;
    static constexpr int kLog2P = 5, P = 32, SUB = 4;
    static constexpr bool kScaled = false, kBlock = true;
    __device__ static __forceinline__ void ld(const uint8_t* w, const uint8_t* sc, int g, S& s) {
        s.c = *reinterpret_cast<const u32x4*>(w + 16 * g);
        s.s = __uint_as_float((uint32_t)sc[g] << 23);
    }
    __device__ static __forceinline__ void unpack(const S& r, int h, float (&v)[8]) {
        const f32x2 a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r.c[h], r.s, 0);
        const f32x2 b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r.c[h], r.s, 1);
        const f32x2 c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r.c[h], r.s, 2);
        const f32x2 d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r.c[h], r.s, 3);
        v[0] = a[0], v[1] = a[1], v[2] = b[0], v[3] = b[1], v[4] = c[0], v[5] = c[1], v[6] = d[0], v[7] = d[1];
    }
};

// one P-element piece of x / gamma / add / sum: P / 8 16-byte loads or stores
template <int P, typename E>
__device__ __forceinline__ void ld_piece(const E* p, float (&v)[P]) {
#pragma unroll
    for (int h = 0; h < P / 8; ++h) {
        float t[8];
        V8<E>::ld(p + 8 * h, t);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[8 * h + i] = t[i];
    }
}
template <int P, typename E>
__device__ __forceinline__ void st_piece(E* p, const float (&v)[P]) {
#pragma unroll
    for (int h = 0; h < P / 8; ++h) {
        float t[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) t[i] = v[8 * h + i];
        V8<E>::st(p + 8 * h, t);
    }
}

template <typename E>
struct NormArgs {
    const E* g;      // RMSNorm weight [K]; nullptr: no norm
    const E* add;    // residual added before the norm ([M, K] contiguous) or nullptr
    E* sum;          // rnd(x + add), written by the wave of output row 0 when add != nullptr
    float eps;
    // EPI_ROPE (one token, W = [q; k; v] heads of hd rows, interleaved rotary pairs = the wave's two rows):
    // rotate q -> q_out, rotate k -> kc row pos, copy v -> vc row pos (rope_kv_append_kernel's arithmetic)
    const float* cosb;
    const float* sinb;
    const int64_t* pos;
    E* q_out;
    E* kc;
    E* vc;
    int nq, nkv, hd, rd;
    int64_t lim;  // position bound: min(cache rows, rotary table rows)
    int* err;     // set when the position is out of [0, lim): nothing is written to the caches
};

// Streams this wave's share of K -- pieces g0, g0 + GS, ... (GS = 64 x waves per row) -- of NR weight rows against
// all M inputs; returns the wave-reduced (unscaled) dot products acc and (NORM) sums of squares ss.
template <int M, int NR, typename E, typename F, bool NORM>
__device__ __forceinline__ void gemv_rows(const E* __restrict__ x, int64_t ldx, const typename F::T* const (&w)[NR],
                                          int K, int g0, int GS, float (&acc)[NR][M], float (&ss)[M],
                                          const NormArgs<E>& na, bool write_sum) {
    constexpr int P = F::P;
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) ss[m] = 0.f;
    // one P-element piece p of every input row against the staged weight pieces ws (NR rows)
    auto piece = [&](int p, const typename F::S (&ws)[NR]) {
        float wv[NR][P];
#pragma unroll
        for (int r = 0; r < NR; ++r) F::unpack(ws[r], wv[r]);
        float gv[P];
        if constexpr (NORM) ld_piece<P>(na.g + P * p, gv);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float xv[P];
            ld_piece<P>(x + m * ldx + P * p, xv);
            if constexpr (NORM) {
                if (na.add != nullptr) {
                    float av[P];
                    ld_piece<P>(na.add + (int64_t)m * K + P * p, av);
#pragma unroll
                    for (int i = 0; i < P; ++i) xv[i] = rnd<E>(xv[i] + av[i]);
                    if (write_sum) st_piece<P>(na.sum + (int64_t)m * K + P * p, xv);
                }
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    ss[m] = __builtin_fmaf(xv[i], xv[i], ss[m]);
                    xv[i] *= gv[i];
                }
            }
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int i = 0; i < P; ++i) acc[r][m] = __builtin_fmaf(wv[r][i], xv[i], acc[r][m]);
        }
    };
    constexpr int U = 4 / NR > 0 ? 4 / NR : 1;  // pieces per weight row per trip (4 KiB per wave)
    const int G = K >> F::kLog2P;                // P-element pieces per row
    int g = g0;
    for (; g + GS * (U - 1) < G; g += GS * U) {
        typename F::S ws[U][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) F::ld(w[r] + P * (g + GS * u), ws[u][r]);
#pragma unroll
        for (int u = 0; u < U; ++u) piece(g + GS * u, ws[u]);
    }
    if (g < G) {  // the ragged tail as ONE predicated trip
        typename F::S ws[U][NR];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (g + GS * u < G) {
#pragma unroll
                for (int r = 0; r < NR; ++r) F::ld(w[r] + P * (g + GS * u), ws[u][r]);
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (g + GS * u < G) piece(g + GS * u, ws[u]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if constexpr (NORM) ss[m] = wave_sum(ss[m]);
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r][m] = wave_sum(acc[r][m]);
    }
}

// The same loop for the block-scaled format F (MXFP4W): pieces are F::P = 32 weights with their scale byte (sp: the
// rows' scale bytes, one per piece), decoded and multiplied in F::SUB sub-steps of P = 8 weights.  A loop of its own,
// so that the dense and FP8 instantiations keep the code they had.
// Streams this wave's share of K -- pieces g0, g0 + GS, ... (GS = 64 x waves per row) -- of NR weight rows against
// all M inputs; returns the wave-reduced (unscaled) dot products acc and (NORM) sums of squares ss.
template <int M, int NR, typename E, typename F, bool NORM>
__device__ __forceinline__ void gemv_rows_w4(const E* __restrict__ x, int64_t ldx, const typename F::T* const (&w)[NR],
                                          const typename F::ST* const (&sp)[NR], int K, int g0, int GS, float (&acc)[NR][M], float (&ss)[M],
                                          const NormArgs<E>& na, bool write_sum) {
    constexpr int P = F::P / F::SUB;  // weights per decoding sub-step
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) ss[m] = 0.f;
    // one piece p (F::SUB sub-steps of P elements) of every input row against the staged weight pieces ws (NR rows)
    auto piece = [&](int p, const typename F::S (&ws)[NR]) {
#pragma unroll
        for (int h = 0; h < F::SUB; ++h) {
            const int64_t k0 = (int64_t)F::P * p + P * h;
            float wv[NR][P];
#pragma unroll
            for (int r = 0; r < NR; ++r) F::unpack(ws[r], h, wv[r]);
            float gv[P];
            if constexpr (NORM) ld_piece<P>(na.g + k0, gv);
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float xv[P];
                ld_piece<P>(x + m * ldx + k0, xv);
                if constexpr (NORM) {
                    if (na.add != nullptr) {
                        float av[P];
                        ld_piece<P>(na.add + (int64_t)m * K + k0, av);
#pragma unroll
                        for (int i = 0; i < P; ++i) xv[i] = rnd<E>(xv[i] + av[i]);
                        if (write_sum) st_piece<P>(na.sum + (int64_t)m * K + k0, xv);
                    }
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        ss[m] = __builtin_fmaf(xv[i], xv[i], ss[m]);
                        xv[i] *= gv[i];
                    }
                }
#pragma unroll
                for (int r = 0; r < NR; ++r)
#pragma unroll
                    for (int i = 0; i < P; ++i) acc[r][m] = __builtin_fmaf(wv[r][i], xv[i], acc[r][m]);
            }
        }
    };
    constexpr int U = 4 / NR > 0 ? 4 / NR : 1;  // pieces per weight row per trip (4 KiB per wave)
    const int G = K >> F::kLog2P;                // P-element pieces per row
    int g = g0;
    for (; g + GS * (U - 1) < G; g += GS * U) {
        typename F::S ws[U][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) F::ld(w[r], sp[r], g + GS * u, ws[u][r]);
#pragma unroll
        for (int u = 0; u < U; ++u) piece(g + GS * u, ws[u]);
    }
    if (g < G) {  // the ragged tail as ONE predicated trip
        typename F::S ws[U][NR];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (g + GS * u < G) {
#pragma unroll
                for (int r = 0; r < NR; ++r) F::ld(w[r], sp[r], g + GS * u, ws[u][r]);
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (g + GS * u < G) piece(g + GS * u, ws[u]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if constexpr (NORM) ss[m] = wave_sum(ss[m]);
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[r][m] = wave_sum(acc[r][m]);
    }
}

// lane m < M picks input m's value out of the per-input accumulators (all lanes hold every sum after wave_sum)
template <int M>
__device__ __forceinline__ float pick(const float (&a)[M], int lane) {
    float v = a[0];
#pragma unroll
    for (int m = 1; m < M; ++m)
        if (lane == m) v = a[m];
    return v;
}

// RPW output rows per wave (consecutive rows r, r + 1): the NORM kernels take 2, which halves the per-weight-byte
// work on x / add / gamma (every wave recomputes the normalised row for the pieces it streams).
// KS waves per row (1 or 4): with few output rows (N = 4096: o / down projections) one wave per row leaves the CUs
// a quarter occupied, so the workgroup's four waves split K (interleaved 1 KiB slices, the workgroup streams
// contiguous 4 KiB) and reduce through LDS in a fixed order.
// F the weight format: W rows are ldw F::T's apart (elements, or bytes of codes); scale is one fp32 per row when
// F::kScaled, one byte per 32-k block in contiguous rows of K / 32 when F::kBlock, and not read otherwise.
template <int M, int EPI, typename E, typename F, bool NORM, int RPW, int KS>
__global__ __launch_bounds__(256) void gemv_kernel(const E* __restrict__ x, int64_t ldx,
                                                   const typename F::T* __restrict__ W, int64_t ldw,
                                                   const typename F::ST* __restrict__ scale, const E* __restrict__ bias,
                                                   const E* __restrict__ res, int64_t ldr, E* __restrict__ y,
                                                   int64_t ldy, int N, int K, NormArgs<E> na) {
    static_assert(!(F::kScaled || F::kBlock) || EPI != EPI_ROPE, "EPI_ROPE has no FP8 / MXFP4 form");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = (blockIdx.x * (4 / KS) + wv / KS) * RPW;
    const int kw = wv % KS;  // this wave's K slice
    if (row >= N) return;    // wave-uniform (N % RPW == 0); workgroup-uniform when KS == 4
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;  // weight rows per output row
    constexpr int NR = NS * RPW;
    const typename F::T* w[NR];
    int wrow[NR];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        wrow[q] = row + q;
        if constexpr (NS == 2) wrow[RPW + q] = row + q + N;  // up row F + n
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) w[r] = W + (int64_t)wrow[r] * ldw;
    float acc[NR][M], ss[M];
    if constexpr (F::kBlock) {
        const typename F::ST* sp[NR];  // the rows' block scales: K / 32 bytes per row, contiguous
#pragma unroll
        for (int r = 0; r < NR; ++r) sp[r] = scale + (int64_t)wrow[r] * (K >> 5);
        gemv_rows_w4<M, NR, E, F, NORM>(x, ldx, w, sp, K, lane + 64 * kw, 64 * KS, acc, ss, na, NORM && row == 0);
    } else {
        gemv_rows<M, NR, E, F, NORM>(x, ldx, w, K, lane + 64 * kw, 64 * KS, acc, ss, na, NORM && row == 0);  // row 0's waves write s
    }
    if constexpr (KS > 1) {
        // partial sums of the K slices: waves 1..KS-1 -> LDS, wave 0 adds them in slice order
        __shared__ float red[KS][NR + 1][M];
        if (kw > 0 && lane == 0) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
#pragma unroll
                for (int r = 0; r < NR; ++r) red[kw][r][m] = acc[r][m];
                red[kw][NR][m] = ss[m];
            }
        }
        __syncthreads();
        if (kw > 0) return;
#pragma unroll
        for (int k = 1; k < KS; ++k)
#pragma unroll
            for (int m = 0; m < M; ++m) {
#pragma unroll
                for (int r = 0; r < NR; ++r) acc[r][m] += red[k][r][m];
                ss[m] += red[k][NR][m];
            }
    }
    if constexpr (F::kScaled) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float sc = scale[wrow[r]];  // the row's power of two: exact
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] *= sc;
        }
    }
    if constexpr (NORM) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float rstd = rsqrtf(ss[m] / K + na.eps);
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r][m] *= rstd;
        }
    }
    if constexpr (EPI == EPI_ROPE) {
        static_assert(RPW == 2, "EPI_ROPE: a wave's two rows are one rotary pair");
        if (lane == 0) {
            const float v0 = rnd<E>(acc[0][0]), v1 = rnd<E>(acc[1][0]);  // the projection's bf16 outputs
            const int h = row / na.hd, d = row - h * na.hd;
            const int64_t ps = na.pos[0];
            if (ps < 0 || ps >= na.lim) {  // out-of-range position: no cache write, q zeroed, error word set
                if (row == 0) *na.err = 1;
                if (h < na.nq) {
                    IO<E>::st(na.q_out + (int64_t)h * na.hd, d, 0.f);
                    IO<E>::st(na.q_out + (int64_t)h * na.hd, d + 1, 0.f);
                }
                return;
            }
            float o0 = v0, o1 = v1;
            E* dst;
            if (h < na.nq + na.nkv) {
                if (d < na.rd) {
                    const float cs = na.cosb[ps * (na.rd / 2) + d / 2], sn = na.sinb[ps * (na.rd / 2) + d / 2];
                    rot_pair(v0, v1, cs, sn, o0, o1);
                }
                dst = h < na.nq ? na.q_out + (int64_t)h * na.hd : na.kc + (ps * na.nkv + (h - na.nq)) * na.hd;
            } else {
                dst = na.vc + (ps * na.nkv + (h - na.nq - na.nkv)) * na.hd;
            }
            IO<E>::st(dst, d, o0);
            IO<E>::st(dst, d + 1, o1);
        }
        return;
    }
    if (lane < M) {
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            float v = pick<M>(acc[q], lane);
            if constexpr (EPI == EPI_SWIGLU) {
                const float a = rnd<E>(v), b = rnd<E>(pick<M>(acc[RPW + q], lane));
                v = rnd<E>(a / (1.f + __expf(-a))) * b;
            } else {
                if (bias != nullptr) v += IO<E>::ld(bias, row + q);
                if constexpr (EPI == EPI_RES) v = rnd<E>(v) + IO<E>::ld(res, (int64_t)lane * ldr + row + q);
            }
            IO<E>::st(y, (int64_t)lane * ldy + row + q, v);
        }
    }
}

int rows_per_wave(bool norm, int N) {
    const int r = norm ? 2 : 1;  // two rows per wave amortise the folded norm's pass over x (profiles/decode_r3b.log)
    return (r == 2 && N % 2 == 0) ? 2 : 1;
}

// waves per output row (cold-cache micro-benchmark, tools/gemv_bench.py): 4 for the NORM and SwiGLU kernels (their
// per-piece work on x / gamma / two weight rows wants more waves in flight) and for long rows over few outputs
// (the 4096 x 11008 down projection), 1 for the plain projections
int waves_per_row(bool split) { return split ? 4 : 1; }

template <typename E, typename F>
struct Args {
    int M;
    const E* x;
    int64_t ldx;
    const typename F::T* W;
    int64_t ldw;
    const typename F::ST* scale;
    const E* b;
    const E* r;
    int64_t ldr;
    E* y;
    int64_t ldy;
    int N, K;
    hipStream_t st;
    NormArgs<E> na;
};

template <int M, int EPI, bool NORM, int RPW, int KS, typename E, typename F>
void launch_m(const Args<E, F>& a) {
    constexpr int RB = 4 / KS * RPW;  // output rows per workgroup
    hipLaunchKernelGGL((gemv_kernel<M, EPI, E, F, NORM, RPW, KS>), dim3((unsigned)((a.N + RB - 1) / RB)), dim3(256), 0,
                       a.st, a.x, a.ldx, a.W, a.ldw, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K, a.na);
}

template <int EPI, bool NORM, int RPW, int KS, typename E, typename F>
void launch_k(const Args<E, F>& a) {
    if constexpr (EPI == EPI_ROPE) {  // one token
        launch_m<1, EPI, NORM, RPW, KS>(a);
    } else {
        switch (a.M) {
            case 1: launch_m<1, EPI, NORM, RPW, KS>(a); break;
            case 2: launch_m<2, EPI, NORM, RPW, KS>(a); break;
            case 3: launch_m<3, EPI, NORM, RPW, KS>(a); break;
            default: launch_m<4, EPI, NORM, RPW, KS>(a); break;
        }
    }
}

template <int EPI, bool NORM, int RPW, typename E, typename F>
void launch_r(const Args<E, F>& a) {
    if (waves_per_row(NORM || EPI == EPI_SWIGLU || (a.N <= 8192 && a.K >= 2 * a.N)) == 4) launch_k<EPI, NORM, RPW, 4>(a);
    else launch_k<EPI, NORM, RPW, 1>(a);
}

// MXFP4 launch rules, from N, K and the form: {output rows per wave, waves per row}.  A 4-bit row is a quarter of the
// 16-byte pieces of its bf16 form (K = 4096: 128, two per lane of ONE wave), so the dense rules' four waves per row
// leave lanes without a piece, and the weight stream is so short that every wave's own pass over x (and gamma / add)
// weighs as much as its weights.  Measured on the five 7B shapes at one row, cold cache, every candidate of
// {1, 2, 4, 8} rows x {1, 4} waves (tools/gemv_bench.py W4_RULES=1, profiles/gemv_w4_rules.log):
//  * waves per row: 4 only for long rows over few outputs (the plain / residual forms with N <= 8192 and K >= 2 N:
//    down 10.0 us against 13.2), 1 everywhere else (q/k/v + norm 9.8 us against 15.3, gate/up + norm + SwiGLU 19.3
//    against 24.7, head 18.5 against 20.8);
//  * rows per wave: 4 once that still leaves 2048 waves (N x waves per row >= 8192: q/k/v 9.8 us against 15.3 with
//    two rows, gate/up 19.3 against 22.6, down 10.0 against 11.7, head 18.5 against 19.4), else 2 (o: 5.3 us against
//    6.6 with four), 1 for odd N.  Eight rows per wave never won (9.9 / 10.7 / 19.4 / 12.9 / 19.4 us) and are not built.
// The norm / SwiGLU forms were measured at K = 4096 only; they keep one wave per row for every K.
// The rules were chosen at M = 1 and do not depend on M.  At M = 3 and 4 some of the kernels they select exceed the
// register file and spill to scratch (the norm + SwiGLU form at four rows per wave: 44-72 VGPRs, 272-400 bytes; the
// plain SwiGLU form at four rows per wave: 112-144 bytes; the norm form at one row per wave and M = 3): correct, and
// slow, like every 4-row GEMV here -- 3 and more rows are the skinny kernel's (SKINNY_MIN_ROWS).
struct W4Rule {
    int rpw, ks;
};
W4Rule g_w4_override{0, 0};  // tools only (sa_launch::gemv_w4_rule): 0 = the rules below
W4Rule w4_rules(int N, int K, bool swiglu, bool norm) {
    W4Rule r;
    r.ks = (!norm && !swiglu && N <= 8192 && K >= 2 * (int64_t)N) ? 4 : 1;
    r.rpw = (int64_t)N * r.ks >= 8192 ? 4 : 2;
    if (g_w4_override.rpw > 0) r = g_w4_override;
    while (N % r.rpw != 0) r.rpw >>= 1;  // rpw divides N
    return r;
}

template <int EPI, bool NORM, int RPW, typename E, typename F>
void launch_w4_k(const Args<E, F>& a, int ks) {
    if (ks == 4) launch_k<EPI, NORM, RPW, 4>(a);
    else launch_k<EPI, NORM, RPW, 1>(a);
}

template <int EPI, bool NORM, typename E, typename F>
void launch_w4(const Args<E, F>& a) {
    const W4Rule r = w4_rules(a.N, a.K, EPI == EPI_SWIGLU, NORM);
    if (r.rpw == 4) launch_w4_k<EPI, NORM, 4>(a, r.ks);
    else if (r.rpw == 2) launch_w4_k<EPI, NORM, 2>(a, r.ks);
    else launch_w4_k<EPI, NORM, 1>(a, r.ks);
}

template <int EPI, bool NORM, typename E, typename F>
void launch(const Args<E, F>& a) {
    if constexpr (F::kBlock) {
        launch_w4<EPI, NORM>(a);
    } else if constexpr (EPI == EPI_ROPE) {
        if constexpr (NORM) launch_r<EPI, NORM, 2>(a);
    } else if (rows_per_wave(NORM, a.N) == 2) {
        launch_r<EPI, NORM, 2>(a);
    } else {
        launch_r<EPI, NORM, 1>(a);
    }
}

template <int EPI, typename E, typename F>
void launch_n(const Args<E, F>& a) {
    if (a.na.g != nullptr) launch<EPI, true>(a);
    else launch<EPI, false>(a);
}

template <typename E, typename F>
void launch_epi(int epi, int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const typename F::ST* scale,
                const void* b, const void* r, int64_t ldr, void* y, int64_t ldy, int N, int K, hipStream_t st,
                const void* norm_w, const void* norm_add, void* norm_sum, float eps, const GemvRope& rp) {
    const Args<E, F> a{M, (const E*)x, ldx, (const typename F::T*)W, ldw, scale, (const E*)b, (const E*)r, ldr, (E*)y,
                       ldy, N, K, st,
                       NormArgs<E>{(const E*)norm_w, (const E*)norm_add, (E*)norm_sum, eps, rp.cosb, rp.sinb, rp.pos,
                                   (E*)rp.q_out, (E*)rp.kc, (E*)rp.vc, rp.nq, rp.nkv, rp.hd, rp.rd, rp.lim, rp.err}};
    if constexpr (!F::kScaled && !F::kBlock) {
        if (epi == EPI_ROPE) return launch_n<EPI_ROPE>(a);
    }
    if (epi == EPI_SWIGLU) launch_n<EPI_SWIGLU>(a);
    else if (epi == EPI_RES) launch_n<EPI_RES>(a);
    else launch_n<EPI_NONE>(a);
}

}  // namespace

namespace sa_launch {
// epi 0: y = x W^T (+ b); 1: y = rnd(x W^T (+ b)) + res; 2: SwiGLU over W = [gate; up] (N = F output columns);
// 3 (with norm_w, one token, dense weights): q/k/v projection + interleaved RoPE + K/V cache append (rope; y unused).
// norm_w != nullptr: x is first replaced by rms_norm(x (+ norm_add), norm_w, eps) inside the same pass
// (norm_add / norm_sum [M, K] contiguous; norm_sum receives x + norm_add).
// scale != nullptr: W holds e4m3fn codes with rows ldw bytes apart and scale one fp32 per code row ([N], [2N] for
// epi 2); x, b, res, y, norm_* are bf16 whatever dtype says.
// bscale != nullptr: W holds e2m1 codes, two per byte (rows ldw bytes apart), and bscale one e8m0 byte per 32 k in
// contiguous rows of K / 32 ([N, K / 32], [2N, K / 32] for epi 2); K % 32 == 0, bf16 as above, epi 0 / 1 / 2.
void gemv(int dtype, int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* scale, const void* b,
          void* y, int64_t ldy, int N, int K, hipStream_t st, int epi, const void* res, int64_t ldr, const void* norm_w,
          const void* norm_add, void* norm_sum, float eps, const GemvRope* rope, const uint8_t* bscale) {
    const GemvRope z{};
    const GemvRope& rp = rope ? *rope : z;
    if (bscale != nullptr)
        launch_epi<u16, MXFP4W>(epi, M, x, ldx, W, ldw, bscale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, rp);
    else if (scale != nullptr)
        launch_epi<u16, E4M3W>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, rp);
    else if (dtype == DT_F16)
        launch_epi<_Float16, DenseW<_Float16>>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, rp);
    else
        launch_epi<u16, DenseW<u16>>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, rp);
}
void gemv_w4_rule(int rpw, int ks) { g_w4_override = W4Rule{rpw, ks}; }
}  // namespace sa_launch
