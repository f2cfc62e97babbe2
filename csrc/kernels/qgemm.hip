// Prefill GEMM over the quantised weight copies of ops/quant.py:  Y[M, N] = X[M, K] deq(W)[N, K]^T (+ bias[N]), any
// M >= 1 (tuned for M >= 65: below, the decode kernels gemv / skinny / wide.hip are the fast ones), any N >= 1.
//  * X bf16, rows ldx elements apart (a strided row view); Y bf16, contiguous [M, N].
//  * W FP8: e4m3fn codes [N, K] (rows ldw bytes apart) and one fp32 power-of-two scale per row; K % 16 == 0.
//  * W MXFP4: e2m1 codes [N, K / 2], low nibble first, and one e8m0 byte per block of 32 k ([N, K / 32]); K % 32 == 0.
// fp32 accumulation over k in ascending order, the bias added in fp32, ONE rounding to bf16 at the store.  No split-K,
// no atomics, no workspace: a call is bitwise deterministic.
//
// Design (gfx950).  A workgroup of 4 waves owns a BM x 128 macro tile of Y, BM = 128 or 64; wave (wv >> 1, wv & 1) owns
// the (BM / 2) x 64 quadrant as (BM / 32) x 4 tiles of v_mfma_f32_16x16x32_bf16 with the weight tile as A and the x
// tile as B (wide.hip's orientation: lane l holds y[m0 + (l & 15)][n0 + 4 (l >> 4) + 0..3], four neighbouring columns
// of one row: an 8-byte store).  K is walked in chunks of 64 = two MFMA k-steps; both operands come from LDS, one
// ds_read_b128 per fragment, and every A fragment feeds BM / 32 MFMAs, every B fragment 4.
//  * LDS image = fragment order, for both operands: the 16-byte unit (f, row) -- k 8 f .. 8 f + 7 of a tile row --
//    sits at f * R + row (R rows in the tile).  A fragment read of k-step s is unit (4 s + (l >> 4), r0 + (l & 15)):
//    the 16 lanes of a k-group read 256 contiguous bytes.  Every staging write is shaped the same way -- 16
//    neighbouring lanes write ONE f at 16 consecutive rows --, so reads and writes are conflict-free by construction;
//    the xor that flash_attn.h and wide.hip need (their staging threads walk along k) has nothing left to permute.
//    Two buffers of (BM + 128) x 64 bf16: 64 KiB at BM = 128 (the static limit, two workgroups per CU), 48 at 64.
//  * X tile: global -> VGPR -> LDS.  Thread t stages rows 16 (t >> 6) + (t & 15) (+ 64) and units (t >> 4 & 3) (+ 4):
//    the four k-groups of a wave read 64 contiguous bytes of each of 16 rows.  Rows >= M and k >= K are zero-filled in
//    LDS and never loaded: x may be exactly M rows long.
//  * W tile: global -> VGPR -> LDS; the codes never sit in LDS.  A lane's 16-byte load is 16 e4m3 codes (two per thread
//    and chunk: rows 16 wv + (l & 15) (+ 64), piece l >> 4) or one MXFP4 block of 32 codes plus its scale byte (one per
//    thread: row 16 (t >> 5) + (t & 15), block t >> 4 & 1).  After the MFMA phase the piece is decoded in registers --
//    v_cvt_pk_f32_fp8 keeping the high half, v_cvt_scalef32_pk_bf16_fp4 with the block scale applied by the
//    instruction, both exact -- into 2 / 4 units of the other buffer.  The LDS image is exactly the dequantised bf16
//    weight (FP8: without the row scale, which multiplies the fp32 accumulators once in the epilogue: a power of two,
//    exact).  Weight rows past N are clamped to N - 1 and never stored; pieces with k >= K are zero-filled (x's zeros
//    alone would not do: a garbage code could decode to NaN).
//  * Pipeline: the loads of chunk t + 1 (x and codes) are issued before the MFMAs of chunk t and written to the other
//    buffer after them, then ONE barrier.  (Buffer (t + 1) & 1 was last read in step t - 1, and every wave has passed
//    that step's barrier.)
//  * Tile choice, from M alone (a host value): BM = 64 for M <= 64 (half the LDS, three workgroups per CU, no MFMAs on
//    64 rows of zeros), else 128.  Both variants add the same k-steps of the same instruction in the
//    same order into an element of Y, and an MFMA's output columns are independent, so row m of Y is bitwise the same
//    whichever variant runs, for every M and whatever the other rows hold.
// Grid: x = row tiles (fastest: neighbouring workgroups share a weight tile), y = column tiles.
//
// Bounds: x is touched only for row < M, k < K; W at rows <= N - 1 and whole pieces below K; scales at rows <= N - 1,
// blocks < K / 32; y / bias only for m < M, n < N; LDS units f < 8, row < R.
//
// Out of scope: the scaled FP8 / FP4 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) with quantised activations (it would
// change the function computed); SwiGLU, RMSNorm and residual epilogues; fp16; split-K for small N; tensor parallelism.
#include "common.h"
#include "decode_formats.h"
#include "launch.h"

using namespace sa;

namespace {

constexpr int BN = 128, KC = 64, NFU = KC / 8;  // columns per tile, k per chunk, 16-byte units per row and chunk

// the codes a thread holds for one chunk: NP pieces (F::H units each) and, MXFP4, the block scale as a float
template <typename F>
struct Codes {
    static constexpr int NP = 4 / F::H;  // 128 rows x (8 / H) pieces over 256 threads
    u32x4 w[NP];
    float s[NP];
};

template <typename F, int BM>
__global__ __launch_bounds__(256) void qgemm_kernel(int M, const u16* __restrict__ x, int64_t ldx,
                                                    const uint8_t* __restrict__ W, int64_t ldw,
                                                    const typename F::ST* __restrict__ scale,
                                                    const u16* __restrict__ bias, u16* __restrict__ y, int N, int K) {
    constexpr int H = F::H;             // units per piece: 2 (FP8), 4 (MXFP4)
    constexpr int PPR = NFU / H;        // pieces per tile row and chunk: 4 / 2
    constexpr int NP = Codes<F>::NP;    // pieces per thread and chunk: 2 / 1
    constexpr int XJ = BM / 64;         // x row groups per thread
    constexpr int MB = BM / 32;         // 16-row blocks per wave
    static_assert(NP * 256 == BN * PPR, "one chunk of the weight tile per pass");
    __shared__ u32x4 xs[2][NFU * BM];
    __shared__ u32x4 ws[2][NFU * BN];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, h = lane >> 4;
    const int wm = wv >> 1, wn = wv & 1;
    const int m0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int TC = (K + KC - 1) / KC;

    // staging roles.  x: rows xr0 (+ 64), units h (+ 4).  W: piece wpc of tile rows wr0 (+ 64 for the second FP8 piece)
    const int xr0 = 16 * wv + c;
    const int wr0 = H == 2 ? 16 * wv + c : 16 * (tid >> 5) + c;
    const int wpc = H == 2 ? h : (h & 1);
    const uint8_t* wp[NP];
    const uint8_t* sp[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int n = min(n0 + wr0 + 64 * j, N - 1);  // clamped: that row's accumulators are never stored
        wp[j] = W + (int64_t)n * ldw;
        sp[j] = F::kBlock ? (const uint8_t*)scale + (int64_t)n * (K / 32) : nullptr;
    }
    const u16* xp[XJ];
    bool xok[XJ];
#pragma unroll
    for (int j = 0; j < XJ; ++j) {
        const int m = m0 + xr0 + 64 * j;
        xok[j] = m < M;
        xp[j] = x + (int64_t)(xok[j] ? m : 0) * ldx;  // dereferenced only when xok
    }

    f32x4 acc[4][MB];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = f32x4{0.f, 0.f, 0.f, 0.f};

    typedef Codes<F> CodesT;
    auto load_w = [&](CodesT& cd, int ch) {
        const int k = ch * KC + wpc * (8 * H);  // the piece's first k; whole pieces: K is a multiple of 8 H
        const bool ok = k < K;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            cd.w[j] = u32x4{0u, 0u, 0u, 0u};
            cd.s[j] = 0.f;
            if (ok) {
                cd.w[j] = *reinterpret_cast<const u32x4*>(wp[j] + (int64_t)(k / (8 * H)) * 16);
                if constexpr (F::kBlock) cd.s[j] = __uint_as_float((uint32_t)sp[j][k / 32] << 23);
            }
        }
    };
    auto store_w = [&](const CodesT& cd, int ch, int buf) {
        const bool ok = ch * KC + wpc * (8 * H) < K;
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int hh = 0; hh < H; ++hh) {
                const u32x4 v = ok ? F::frag(cd.w[j], hh, cd.s[j]) : u32x4{0u, 0u, 0u, 0u};
                ws[buf][(wpc * H + hh) * BN + wr0 + 64 * j] = v;
            }
    };
    auto load_x = [&](u32x4 (&xr)[XJ][2], int ch) {
#pragma unroll
        for (int j = 0; j < XJ; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = ch * KC + 8 * (h + 4 * q);
                xr[j][q] = u32x4{0u, 0u, 0u, 0u};
                if (xok[j] && k < K) xr[j][q] = *reinterpret_cast<const u32x4*>(xp[j] + k);
            }
    };
    auto store_x = [&](const u32x4 (&xr)[XJ][2], int buf) {
#pragma unroll
        for (int j = 0; j < XJ; ++j)
#pragma unroll
            for (int q = 0; q < 2; ++q) xs[buf][(h + 4 * q) * BM + xr0 + 64 * j] = xr[j][q];
    };
    auto compute = [&](int buf) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int f = 4 * s + h;
            u32x4 a[4], b[MB];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) a[nb] = ws[buf][f * BN + wn * 64 + 16 * nb + c];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) b[mb] = xs[buf][f * BM + wm * (BM / 2) + 16 * mb + c];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[nb][mb] = Act<u16>::mma(a[nb], b[mb], acc[nb][mb]);
        }
    };

    CodesT cd;
    u32x4 xr[XJ][2];
    load_x(xr, 0);
    load_w(cd, 0);
    store_x(xr, 0);
    store_w(cd, 0, 0);
    __syncthreads();
    for (int t = 0; t < TC; ++t) {
        const bool more = t + 1 < TC;
        if (more) {
            load_x(xr, t + 1);
            load_w(cd, t + 1);
        }
        compute(t & 1);
        if (more) {
            store_x(xr, (t + 1) & 1);
            store_w(cd, t + 1, (t + 1) & 1);
        }
        __syncthreads();
    }

    // epilogue: (row scale,) bias, one rounding; four neighbouring columns of one row per lane and tile
    const bool vec = (N & 3) == 0;  // rows of y 8-byte aligned
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int n = n0 + wn * 64 + 16 * nb + 4 * h;
        if (n >= N) continue;
        float sc[4], bv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int nn = min(n + r, N - 1);
            sc[r] = F::kScaled ? ((const float*)scale)[nn] : 1.f;
            bv[r] = bias != nullptr ? bf2f(bias[nn]) : 0.f;
        }
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int m = m0 + wm * (BM / 2) + 16 * mb + c;
            if (m >= M) continue;
            u16 o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[nb][mb][r];
                if constexpr (F::kScaled) v *= sc[r];
                if (bias != nullptr) v += bv[r];
                o[r] = f2bf(v);
            }
            u16* yp = y + (int64_t)m * N + n;
            if (vec) {  // (n % 4 == 0 and N % 4 == 0: n + 3 < N)
                *reinterpret_cast<u16x4*>(yp) = u16x4{o[0], o[1], o[2], o[3]};
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < N) yp[r] = o[r];
            }
        }
    }
}

template <typename F>
void launch(int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const typename F::ST* scale, const void* bias,
            void* y, int N, int K, hipStream_t st) {
    const int tn = (N + BN - 1) / BN;
    if (M <= 64)
        hipLaunchKernelGGL((qgemm_kernel<F, 64>), dim3(1u, (unsigned)tn), dim3(256), 0, st, M,
                           (const u16*)x, ldx, (const uint8_t*)W, ldw, scale, (const u16*)bias, (u16*)y, N, K);
    else
        hipLaunchKernelGGL((qgemm_kernel<F, 128>), dim3((unsigned)((M + 127) / 128), (unsigned)tn), dim3(256), 0, st, M,
                           (const u16*)x, ldx, (const uint8_t*)W, ldw, scale, (const u16*)bias, (u16*)y, N, K);
}

}  // namespace

namespace sa_launch {
void qgemm(int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* scale, const uint8_t* bscale,
           const void* bias, void* y, int N, int K, hipStream_t st) {
    if (M < 1 || N < 1 || K < 16 || (N + BN - 1) / BN > 65535) return;  // (the bindings reject these; never launch on them)
    if (bscale != nullptr) {
        if (K % 32 != 0) return;
        launch<MXFP4W>(M, x, ldx, W, ldw, bscale, bias, y, N, K, st);
    } else if (scale != nullptr && K % 16 == 0) {
        launch<E4M3W>(M, x, ldx, W, ldw, scale, bias, y, N, K, st);
    }
}
}  // namespace sa_launch
