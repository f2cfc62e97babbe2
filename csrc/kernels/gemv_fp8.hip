// Decode-time linear layer on gfx950 with FP8 weights:  y[M, N] = x[M, K] (scale[n] * Q[N, K])^T (+ b)  for M <= 4.
//
// The FP8-weight variant of gemv.hip (same structure, same launch rules, same rounding points): Q holds OCP e4m3fn
// codes, one byte per weight, and scale one fp32 power of two per output row (scaling_amd/ops/quant.py), so the
// layer streams half the bytes of its bf16 form.  Differences from gemv_kernel:
//  * a piece is still 16 bytes per lane, which is now 16 weights: K % 16 == 0, two 16-byte loads of x (and of
//    gamma / add for the NORM prologue) per piece and input row;
//  * the codes are converted two at a time by the hardware (v_cvt_pk_f32_fp8, __builtin_amdgcn_cvt_pk_f32_fp8), once
//    per piece and weight row, and reused by all M inputs; products and sums are fp32 as before;
//  * the row scale multiplies the dot product ONCE per output row, after the wave / K-split reduction and before the
//    bias and the epilogue: a power of two, so the result is the dot product with the dequantised bf16 weights up
//    to the order of the fp32 sums.  SwiGLU: rows n and F + n each take their own scale.
// Epilogues RES and SWIGLU and the NORM prologue as in gemv.hip; the one-launch RoPE step (EPI_ROPE) has no FP8 form.
#include "common.h"
#include "launch.h"

using namespace sa;

namespace {

enum { EPI_NONE = 0, EPI_RES = 1, EPI_SWIGLU = 2 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct NormArgs8 {
    const u16* g;    // RMSNorm weight [K]; nullptr: no norm
    const u16* add;  // residual added before the norm ([M, K] contiguous) or nullptr
    u16* sum;        // rnd(x + add), written by the wave of output row 0 when add != nullptr
    float eps;
};

// 16 e4m3 codes (one 16-byte piece) -> 16 floats, in memory order
__device__ __forceinline__ void cvt16(const u32x4& r, float (&v)[16]) {
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

__device__ __forceinline__ void ld16(const u16* p, float (&v)[16]) {
    const u16x8 a = *reinterpret_cast<const u16x8*>(p), b = *reinterpret_cast<const u16x8*>(p + 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = bf2f(a[i]);
        v[i + 8] = bf2f(b[i]);
    }
}

__device__ __forceinline__ void st16(u16* p, const float (&v)[16]) {
    u16x8 a, b;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        a[i] = f2bf(v[i]);
        b[i] = f2bf(v[i + 8]);
    }
    *reinterpret_cast<u16x8*>(p) = a;
    *reinterpret_cast<u16x8*>(p + 8) = b;
}

// Streams this wave's share of K -- pieces g0, g0 + GS, ... (GS = 64 x waves per row) -- of NR code rows against
// all M inputs; returns the wave-reduced (unscaled) dot products acc and (NORM) sums of squares ss.
template <int M, int NR, bool NORM>
__device__ __forceinline__ void gemv8_rows(const u16* __restrict__ x, int64_t ldx, const uint8_t* const (&w)[NR], int K,
                                           int g0, int GS, float (&acc)[NR][M], float (&ss)[M], const NormArgs8& na,
                                           bool write_sum) {
#pragma unroll
    for (int r = 0; r < NR; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m) ss[m] = 0.f;
    // one 16-element piece p of every input row against the code pieces wq (NR rows)
    auto piece = [&](int p, const u32x4 (&wq)[NR]) {
        float wv[NR][16];
#pragma unroll
        for (int r = 0; r < NR; ++r) cvt16(wq[r], wv[r]);
        float gv[16];
        if constexpr (NORM) ld16(na.g + 16 * p, gv);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float xv[16];
            ld16(x + m * ldx + 16 * p, xv);
            if constexpr (NORM) {
                if (na.add != nullptr) {
                    float av[16];
                    ld16(na.add + (int64_t)m * K + 16 * p, av);
#pragma unroll
                    for (int i = 0; i < 16; ++i) xv[i] = rnd<u16>(xv[i] + av[i]);
                    if (write_sum) st16(na.sum + (int64_t)m * K + 16 * p, xv);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    ss[m] = __builtin_fmaf(xv[i], xv[i], ss[m]);
                    xv[i] *= gv[i];
                }
            }
#pragma unroll
            for (int r = 0; r < NR; ++r)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[r][m] = __builtin_fmaf(wv[r][i], xv[i], acc[r][m]);
        }
    };
    constexpr int U = 4 / NR > 0 ? 4 / NR : 1;  // pieces per code row per trip (4 KiB per wave)
    const int G = K >> 4;                        // 16-element pieces per row
    int g = g0;
    for (; g + GS * (U - 1) < G; g += GS * U) {
        u32x4 wq[U][NR];
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int u = 0; u < U; ++u) wq[u][r] = *reinterpret_cast<const u32x4*>(w[r] + 16 * (g + GS * u));
#pragma unroll
        for (int u = 0; u < U; ++u) piece(g + GS * u, wq[u]);
    }
    if (g < G) {  // the ragged tail as ONE predicated trip
        u32x4 wq[U][NR];
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (g + GS * u < G) {
#pragma unroll
                for (int r = 0; r < NR; ++r) wq[u][r] = *reinterpret_cast<const u32x4*>(w[r] + 16 * (g + GS * u));
            }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (g + GS * u < G) piece(g + GS * u, wq[u]);
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

// RPW output rows per wave and KS waves per row as in gemv_kernel (gemv.hip); Q rows are ldq BYTES apart.
template <int M, int EPI, bool NORM, int RPW, int KS>
__global__ __launch_bounds__(256) void gemv8_kernel(const u16* __restrict__ x, int64_t ldx,
                                                    const uint8_t* __restrict__ Q, int64_t ldq,
                                                    const float* __restrict__ scale, const u16* __restrict__ bias,
                                                    const u16* __restrict__ res, int64_t ldr, u16* __restrict__ y,
                                                    int64_t ldy, int N, int K, NormArgs8 na) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int row = (blockIdx.x * (4 / KS) + wv / KS) * RPW;
    const int kw = wv % KS;  // this wave's K slice
    if (row >= N) return;    // wave-uniform (N % RPW == 0); workgroup-uniform when KS == 4
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;  // code rows per output row
    constexpr int NR = NS * RPW;
    const uint8_t* w[NR];
    int wrow[NR];
#pragma unroll
    for (int q = 0; q < RPW; ++q) {
        wrow[q] = row + q;
        if constexpr (NS == 2) wrow[RPW + q] = row + q + N;  // up row F + n
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) w[r] = Q + (int64_t)wrow[r] * ldq;
    float acc[NR][M], ss[M];
    gemv8_rows<M, NR, NORM>(x, ldx, w, K, lane + 64 * kw, 64 * KS, acc, ss, na, NORM && row == 0);  // row 0's waves write s
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
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const float sc = scale[wrow[r]];  // the row's power of two: exact
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] *= sc;
    }
    if constexpr (NORM) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float rstd = rsqrtf(ss[m] / K + na.eps);
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r][m] *= rstd;
        }
    }
    if (lane < M) {
#pragma unroll
        for (int q = 0; q < RPW; ++q) {
            float v = pick<M>(acc[q], lane);
            if constexpr (EPI == EPI_SWIGLU) {
                const float a = rnd<u16>(v), b = rnd<u16>(pick<M>(acc[RPW + q], lane));
                v = rnd<u16>(a / (1.f + __expf(-a))) * b;
            } else {
                if (bias != nullptr) v += IO<u16>::ld(bias, row + q);
                if constexpr (EPI == EPI_RES) v = rnd<u16>(v) + IO<u16>::ld(res, (int64_t)lane * ldr + row + q);
            }
            IO<u16>::st(y, (int64_t)lane * ldy + row + q, v);
        }
    }
}

struct Args8 {
    int M;
    const u16* x;
    int64_t ldx;
    const uint8_t* Q;
    int64_t ldq;
    const float* scale;
    const u16* b;
    const u16* r;
    int64_t ldr;
    u16* y;
    int64_t ldy;
    int N, K;
    hipStream_t st;
    NormArgs8 na;
};

template <int EPI, bool NORM, int RPW, int KS>
void launch_k(const Args8& a) {
    constexpr int RB = 4 / KS * RPW;  // output rows per workgroup
    const dim3 grid((unsigned)((a.N + RB - 1) / RB)), block(256);
    switch (a.M) {
        case 1: hipLaunchKernelGGL((gemv8_kernel<1, EPI, NORM, RPW, KS>), grid, block, 0, a.st, a.x, a.ldx, a.Q, a.ldq, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K, a.na); break;
        case 2: hipLaunchKernelGGL((gemv8_kernel<2, EPI, NORM, RPW, KS>), grid, block, 0, a.st, a.x, a.ldx, a.Q, a.ldq, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K, a.na); break;
        case 3: hipLaunchKernelGGL((gemv8_kernel<3, EPI, NORM, RPW, KS>), grid, block, 0, a.st, a.x, a.ldx, a.Q, a.ldq, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K, a.na); break;
        default: hipLaunchKernelGGL((gemv8_kernel<4, EPI, NORM, RPW, KS>), grid, block, 0, a.st, a.x, a.ldx, a.Q, a.ldq, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K, a.na); break;
    }
}

// the launch rules of gemv.hip: two rows per wave for the NORM kernels over an even N; four waves per row (K split)
// for the NORM and SwiGLU kernels and for long rows over few outputs, one otherwise
template <int EPI, bool NORM, int RPW>
void launch_r(const Args8& a) {
    if (NORM || EPI == EPI_SWIGLU || (a.N <= 8192 && a.K >= 2 * a.N)) launch_k<EPI, NORM, RPW, 4>(a);
    else launch_k<EPI, NORM, RPW, 1>(a);
}

template <int EPI, bool NORM>
void launch(const Args8& a) {
    if (NORM && a.N % 2 == 0) launch_r<EPI, NORM, 2>(a);
    else launch_r<EPI, NORM, 1>(a);
}

template <int EPI>
void launch_n(const Args8& a) {
    if (a.na.g != nullptr) launch<EPI, true>(a);
    else launch<EPI, false>(a);
}

}  // namespace

namespace sa_launch {
// x, b, res, y, norm_* bf16; Q e4m3fn codes with rows ldq bytes apart; scale fp32 per code row ([N], [2N] for epi 2).
// epi 0: y = x W^T (+ b); 1: y = rnd(x W^T (+ b)) + res; 2: SwiGLU over W = [gate; up] (N = F output columns), with
// W = scale * Q.  norm_w != nullptr: the RMSNorm prologue of gemv().
void gemv_w8(int M, const void* x, int64_t ldx, const void* Q, int64_t ldq, const float* scale, const void* b, void* y,
             int64_t ldy, int N, int K, hipStream_t st, int epi, const void* res, int64_t ldr, const void* norm_w,
             const void* norm_add, void* norm_sum, float eps) {
    const Args8 a{M, (const u16*)x, ldx, (const uint8_t*)Q, ldq, scale, (const u16*)b, (const u16*)res, ldr, (u16*)y,
                  ldy, N, K, st, NormArgs8{(const u16*)norm_w, (const u16*)norm_add, (u16*)norm_sum, eps}};
    if (epi == EPI_SWIGLU) launch_n<EPI_SWIGLU>(a);
    else if (epi == EPI_RES) launch_n<EPI_RES>(a);
    else launch_n<EPI_NONE>(a);
}
}  // namespace sa_launch
