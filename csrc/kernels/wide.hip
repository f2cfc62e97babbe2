// Decode-time linear layer on the matrix cores for 1 <= M <= 64 input rows:  y[M, N] = x[M, K] W[N, K]^T (+ b).
// The forms, weight formats and rounding points are those of skinny.hip (its header comment is the specification:
// plain (+ bias), RES, SWIGLU over [gate; up], the RMSNorm prologue with epilogue 0 / 2; dense bf16 / fp16, e4m3 with
// per-row scales, MXFP4 with e8m0 block scales).  What differs is the path of x.
//
// skinny.hip loads a wave's B operand (16 rows of x) per lane from global memory and every wave re-reads all of x; at
// 64 rows that is four times the fragments per wave and the x side would outweigh the weight stream.  Here:
//  * Weights: unchanged.  Global -> VGPR, one 16-byte load IS the A fragment of v_mfma_f32_16x16x32 (lane l: weight row
//    n0 + (l & 15), k-group l >> 4), addresses clamped instead of predicated, two register buffers so that the next
//    chunk's loads are in flight during this chunk's MFMAs.  They are read once and never touch LDS.
//  * x: through LDS, once per workgroup.  The workgroup's four waves own different weight tiles (TPW output tiles each,
//    x 2 weight tiles for SwiGLU) and walk the SAME k chunks, so one staged chunk serves 4 NT weight tiles.  A chunk is
//    64 rows x NF fragments of 8 k (KC = 8 NF = 64 .. 256 k, chosen so that a lane holds at most 8 weight pieces per
//    buffer: the skinny kernel's bytes in flight).  Thread t stages row t >> 2, fragments (t & 3) + 4 q: four
//    neighbouring lanes read 64 contiguous bytes of a row, and a thread always works on ONE row, so the NORM
//    prologue's sum of squares stays in a register.  The next chunk's global loads are issued before this chunk's
//    MFMAs and written to the other LDS buffer after them: one barrier per chunk.
//  * LDS layout = fragment order: unit (f, row) of 16 bytes sits at f * 64 + (row ^ ((f & 3) << 2)).  A wave's B
//    fragment for row block mb is ONE ds_read_b128 per lane at (f, 16 mb + c): the 16 lanes of a k-group read 256
//    contiguous bytes (the xor only permutes them), conflict-free.  The staging write of 16 lanes covers rows
//    4 i .. 4 i + 3 x fragments f0 .. f0 + 3; the xor spreads the four fragments over the four 64-byte bank groups, so
//    it is conflict-free too without padding (two 32 KiB buffers at most: the static 64 KiB, two workgroups per CU).
//  * Rows >= M and k >= K are zero-filled in LDS and never loaded: x / add / res may be exactly M rows long.
//  * NORM prologue at staging, once per workgroup and chunk (not per wave and tile): s = rnd(x + add) (written by
//    the workgroups of column block 0, each its own K range), ss += s^2 in fp32 per thread in k order, then the row's
//    four threads by xor 1, xor 2; the staged value is rnd(s * gamma), ONE rounding as in skinny.hip; rstd scales the
//    fp32 accumulators at the end.
//  * Row blocks: MB = ceil(M / 16) <= 4, wave-uniform.  Every A fragment (an FP8 / MXFP4 piece decoded ONCE) feeds MB
//    MFMAs into acc[tile][mb]; lane l holds y[16 mb + (l & 15)][n0 + 4 (l >> 4) + 0..3].
//  * Small N (o / down: 256 tiles): K is split across workgroups (gridDim.y slices of whole chunks) until about one
//    workgroup per CU exists.  A slice writes its fp32 partial sums (and partial sums of squares) to a workspace the
//    caller passes in, and a second small launch adds them IN SLICE ORDER and applies the epilogue.  No atomics, no
//    waiting between workgroups: bitwise deterministic, and nothing can hang.  (The arrival-counter merge was the
//    alternative; it needs zeroed counters that survive graph replays and concurrent streams, a second launch needs
//    neither.)
// Launch rules (wide_rules) depend on N, K, the form and the format, NEVER on M, the staging thread of a row and its k
// order are fixed, and every output column of an MFMA is independent of the others: row m of y is bitwise the same
// for every M in 1..64 and whatever the other rows hold.
//
// Bounds: weight rows are clamped to N - 1 (never stored), pieces to G - 1 (the same row, met by a zero x fragment);
// x / add / gamma / s are touched only for row < M and k < K; LDS indices are f < NF, row < 64; a partial is written
// only for tile < tiles into rows < 16 MB of a workspace of 16 MB x 16 tiles floats per slice and half.
#include <algorithm>

#include "common.h"
#include "decode_formats.h"
#include "launch.h"

using namespace sa;

namespace {

enum { EPI_NONE = 0, EPI_RES = 1, EPI_SWIGLU = 2 };

template <typename E>
struct NormArgs {
    const E* g;    // RMSNorm weight [K]
    const E* add;  // residual added before the norm ([M, K] contiguous) or nullptr
    E* sum;        // rnd(x + add) [M, K], written when add != nullptr
    float eps;
};

// steps (32 H k each) per chunk for NT weight tiles per wave: at most 8 weight pieces per lane and buffer (4 with the
// NORM prologue, whose staging holds x, add and gamma), at most 32 (NORM: 16) x fragments per row and chunk
constexpr int wide_steps(int H, int NT, bool norm) {
    const int bud = (norm ? 4 : 8) / NT, cap = (norm ? 16 : 32) / (4 * H);
    return bud > cap ? cap : (bud < 1 ? 1 : bud);
}

// the weight pieces of one chunk: U steps of NT tiles; BS: the block scales as floats
template <int NT, int U, bool BS>
struct Trip {
    u32x4 w[NT][U];
    float s[BS ? NT : 1][BS ? U : 1];
};
// the staged pieces of one chunk held by one thread: SQ fragments of its row (x, and add / gamma for NORM)
template <int SQ, bool NORM>
struct Stage {
    u32x4 x[SQ];
    u32x4 a[NORM ? SQ : 1];
    u32x4 g[NORM ? SQ : 1];
};

// the epilogue of one output element; v / up are the fp32 sums over K (up: the SwiGLU up half)
template <typename E, int EPI>
__device__ __forceinline__ void epi_store(float v, float up, int m, int n, const float* scale, bool norm, float rstd,
                                          const E* bias, const E* res, int64_t ldr, E* y, int64_t ldy, int N) {
    if (scale != nullptr) v *= scale[n];  // the row's power of two: exact
    if (norm) v *= rstd;
    if constexpr (EPI == EPI_SWIGLU) {
        if (scale != nullptr) up *= scale[(int64_t)N + n];
        if (norm) up *= rstd;
        const float a = rnd<E>(v), b = rnd<E>(up);
        v = rnd<E>(a / (1.f + __expf(-a))) * b;
    } else {
        if (bias != nullptr) v += IO<E>::ld(bias, n);
        if constexpr (EPI == EPI_RES) v = rnd<E>(v) + IO<E>::ld(res, (int64_t)m * ldr + n);
    }
    IO<E>::st(y, (int64_t)m * ldy + n, v);
}

// grid (column blocks of 4 TPW tiles, K slices); cps chunks per slice.  gridDim.y > 1: partial sums -> part / ssp
// (wide_merge_kernel finishes); gridDim.y == 1: the epilogue here
template <typename E, typename F, int EPI, bool NORM, int TPW>
__global__ __launch_bounds__(256) void wide_kernel(int M, const E* __restrict__ x, int64_t ldx,
                                                   const typename F::T* __restrict__ W, int64_t ldw,
                                                   const typename F::ST* __restrict__ scale, const E* __restrict__ bias,
                                                   const E* __restrict__ res, int64_t ldr, E* __restrict__ y, int64_t ldy,
                                                   int N, int K, NormArgs<E> na, float* __restrict__ part,
                                                   float* __restrict__ ssp, int cps) {
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;  // weight tiles per output tile
    constexpr int NT = NS * TPW;                   // weight tiles per wave
    constexpr int P = F::P, H = F::H;
    constexpr int U = wide_steps(H, NT, NORM);
    constexpr int NF = 4 * H * U;  // x fragments (8 k) per row and chunk
    constexpr int KC = 8 * NF;     // k per chunk
    constexpr int SQ = NF / 4;     // fragments a thread stages per chunk
    static_assert(NT <= 2 && NF <= 32 && SQ >= 1, "tiles per wave / chunk size");
    __shared__ u32x4 xs[2][NF * 64];

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = lane & 15, h = lane >> 4;  // weight row inside the tile (= input row inside a row block), k-group
    const int srow = tid >> 2, sf = tid & 3;  // the row this thread stages, and its fragments sf + 4 q
    const int MB = (M + 15) >> 4;
    const int tiles = (N + 15) / 16;
    const int tile0 = ((int)blockIdx.x * 4 + wv) * TPW;
    const int ky = blockIdx.y;
    const int G = K / P;  // 16-byte pieces per weight row
    const int TC = (K + KC - 1) / KC;
    const int c0 = ky * cps;
    const int T = max(min(c0 + cps, TC) - c0, 0);  // this slice's chunks (the same for every thread of the workgroup)

    // weight rows of this lane, clamped into [0, N): a clamped row's accumulators are never stored
    const typename F::T* wp[NT];
    const typename F::ST* sp[NT];  // kBlock: the rows' block scales, one byte per piece
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        const int n = min((tile0 + j) * 16 + c, N - 1);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            wp[s * TPW + j] = W + ((int64_t)n + (int64_t)s * N) * ldw;
            sp[s * TPW + j] = F::kBlock ? scale + ((int64_t)n + (int64_t)s * N) * G : nullptr;
        }
    }
    const bool srow_ok = srow < M;
    const E* xr = x + (int64_t)srow * ldx;  // dereferenced only when srow_ok
    const bool has_add = NORM && na.add != nullptr;
    const E* ar = has_add ? na.add + (int64_t)srow * K : nullptr;  // likewise
    const bool write_s = has_add && blockIdx.x == 0;

    f32x4 acc[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) acc[j][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;

    typedef Trip<NT, U, F::kBlock> TripT;
    typedef Stage<SQ, NORM> StageT;
    auto load_w = [&](TripT& tr, int ch) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int pc = min(ch * (4 * U) + 4 * u + h, G - 1);  // clamped: the row's last piece, met by zeros of x
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                tr.w[j][u] = *reinterpret_cast<const u32x4*>(wp[j] + (int64_t)pc * (16 / (int)sizeof(typename F::T)));
                if constexpr (F::kBlock) tr.s[j][u] = __uint_as_float((uint32_t)sp[j][pc] << 23);
            }
        }
    };
    auto stage_load = [&](StageT& sg, int ch) {
#pragma unroll
        for (int q = 0; q < SQ; ++q) {
            const int k = ch * KC + 8 * (sf + 4 * q);
            const bool ok = srow_ok && k < K;
            sg.x[q] = u32x4{0u, 0u, 0u, 0u};
            if (ok) sg.x[q] = *reinterpret_cast<const u32x4*>(xr + k);
            if constexpr (NORM) {
                sg.g[q] = u32x4{0u, 0u, 0u, 0u};
                sg.a[q] = u32x4{0u, 0u, 0u, 0u};
                if (ok) sg.g[q] = *reinterpret_cast<const u32x4*>(na.g + k);
                if (ok && has_add) sg.a[q] = *reinterpret_cast<const u32x4*>(ar + k);
            }
        }
    };
    auto stage_store = [&](const StageT& sg, int ch, int buf) {
#pragma unroll
        for (int q = 0; q < SQ; ++q) {
            const int f = sf + 4 * q;
            u32x4 b = sg.x[q];
            if constexpr (NORM) {
                float xv[8], gv[8];
                Act<E>::unpack(b, xv);
                if (has_add) {
                    float av[8];
                    Act<E>::unpack(sg.a[q], av);
#pragma unroll
                    for (int i = 0; i < 8; ++i) xv[i] = rnd<E>(xv[i] + av[i]);
                    const int k = ch * KC + 8 * f;
                    if (write_s && srow_ok && k < K)
                        *reinterpret_cast<u32x4*>(na.sum + (int64_t)srow * K + k) = Act<E>::pack(xv);
                }
                Act<E>::unpack(sg.g[q], gv);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    ss = __builtin_fmaf(xv[i], xv[i], ss);
                    xv[i] *= gv[i];
                }
                b = Act<E>::pack(xv);  // rnd(s * gamma)
            }
            xs[buf][f * 64 + (srow ^ (sf << 2))] = b;
        }
    };
    auto compute = [&](const TripT& tr, int buf) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int hh = 0; hh < H; ++hh) {
                const int f = H * (4 * u + h) + hh;
                const u32x4* bp = &xs[buf][f * 64];
                const int cs = c ^ ((f & 3) << 2);
                u32x4 b[4];
#pragma unroll
                for (int mb = 0; mb < 4; ++mb) b[mb] = mb < MB ? bp[mb * 16 + cs] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const u32x4 a = F::frag(tr.w[j][u], hh, F::kBlock ? tr.s[j][u] : 0.f);
#pragma unroll
                    for (int mb = 0; mb < 4; ++mb)
                        if (mb < MB) acc[j][mb] = Act<E>::mma(a, b[mb], acc[j][mb]);
                }
            }
        }
    };

    TripT ta, tb;
    StageT sg;
    if (T > 0) {
        stage_load(sg, c0);
        load_w(ta, c0);
        stage_store(sg, c0, 0);
    }
    __syncthreads();
    // chunk t: the next chunk's loads first, this chunk's MFMAs, then the next chunk into the other LDS buffer (all
    // waves passed the previous barrier after their MFMAs on it) and one barrier
    auto step = [&](const TripT& cur, TripT& nxt, int t) {
        const bool more = t + 1 < T;
        if (more) {
            stage_load(sg, c0 + t + 1);
            load_w(nxt, c0 + t + 1);
        }
        compute(cur, t & 1);
        if (more) stage_store(sg, c0 + t + 1, (t + 1) & 1);
        __syncthreads();
    };
    for (int t = 0; t < T; t += 2) {
        step(ta, tb, t);
        if (t + 1 < T) step(tb, ta, t + 1);
    }
    if constexpr (NORM) {  // the four staging threads of a row, fixed order
        ss += __shfl_xor(ss, 1, 64);
        ss += __shfl_xor(ss, 2, 64);
    }

    if (gridDim.y > 1) {
        // this slice's partial sums: part [slice][half][16 MB rows][16 tiles columns], ssp [slice][64 rows]
        if (NORM && blockIdx.x == 0 && sf == 0) ssp[ky * 64 + srow] = ss;
        const int64_t Np = (int64_t)tiles * 16, MR = MB * 16;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            if (tile0 + j >= tiles) continue;
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int mb = 0; mb < 4; ++mb)
                    if (mb < MB)
                        *reinterpret_cast<f32x4*>(part + (((int64_t)ky * NS + s) * MR + mb * 16 + c) * Np +
                                                  (tile0 + j) * 16 + 4 * h) = acc[s * TPW + j][mb];
        }
        return;
    }
    float* ssum = reinterpret_cast<float*>(&xs[0][0]);  // (the loop's last barrier freed the buffers)
    if constexpr (NORM) {
        if (sf == 0) ssum[srow] = ss;
        __syncthreads();
    }
#pragma unroll
    for (int mb = 0; mb < 4; ++mb) {
        const int m = mb * 16 + c;
        if (mb >= MB || m >= M) continue;
        const float rstd = NORM ? rsqrtf(ssum[m] / K + na.eps) : 1.f;
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = (tile0 + j) * 16 + 4 * h + r;
                if (n >= N) continue;
                epi_store<E, EPI>(acc[j][mb][r], NS == 2 ? acc[NT - TPW + j][mb][r] : 0.f, m, n,
                                  F::kScaled ? (const float*)scale : nullptr, NORM, rstd, bias, res, ldr, y, ldy, N);
            }
        }
    }
}

// the second launch of the K-split rule: thread (n, m) adds the KS partial sums in slice order and applies the epilogue
template <typename E, int EPI>
__global__ __launch_bounds__(256) void wide_merge_kernel(int M, int KS, const float* __restrict__ part, int64_t Np,
                                                         const float* __restrict__ ssp, const float* __restrict__ scale,
                                                         const E* __restrict__ bias, const E* __restrict__ res, int64_t ldr,
                                                         E* __restrict__ y, int64_t ldy, int N, int K, float eps) {
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;
    const int n = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
    if (n >= N || m >= M) return;
    const int64_t MR = (int64_t)((M + 15) >> 4) * 16;
    float v = 0.f, up = 0.f, ss = 0.f;
    for (int k = 0; k < KS; ++k) {
        v += part[(((int64_t)k * NS) * MR + m) * Np + n];
        if constexpr (NS == 2) up += part[(((int64_t)k * NS + 1) * MR + m) * Np + n];
        if (ssp != nullptr) ss += ssp[k * 64 + m];
    }
    const float rstd = ssp != nullptr ? rsqrtf(ss / K + eps) : 1.f;
    epi_store<E, EPI>(v, up, m, n, scale, ssp != nullptr, rstd, bias, res, ldr, y, ldy, N);
}

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
    float* ws;
};

// Launch rules, from N, K, the form (ns weight tiles per output tile, the NORM prologue) and the format (H MFMAs per
// piece), nothing else -- in particular not M (batch invariance):
//  * more than 2048 weight tiles (gate/up): no K split, 2 weight tiles per wave (TPW = 2, SwiGLU 1): 344+ workgroups;
//  * at most 2048: one output tile per wave, and K split into slices of whole chunks across workgroups until there are
//    about 256 workgroups (one per CU; o / down: 64 column blocks x 4 slices), at most 8 slices and one per chunk.
struct Rules {
    int tpw, ks, cps;  // output tiles per wave, K slices, chunks per slice
};
Rules wide_rules(int N, int K, int ns, int H, bool norm) {
    const int tiles = (N + 15) / 16;
    if (tiles * ns > 2048) return {2 / ns, 1, 1 << 30};
    const int kc = 32 * H * wide_steps(H, ns, norm), tc = (K + kc - 1) / kc;
    const int nbx = (tiles + 3) / 4;
    const int want = std::min(std::min(std::max(256 / nbx, 1), 8), tc);
    const int cps = (tc + want - 1) / want;
    return {1, (tc + cps - 1) / cps, cps};
}

template <int EPI, bool NORM, int TPW, typename E, typename F>
void launch_t(const Args<E, F>& a, const Rules& r) {
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;
    const int tiles = (a.N + 15) / 16, MB = (a.M + 15) / 16;
    const int64_t Np = (int64_t)tiles * 16;
    float* part = r.ks > 1 ? a.ws : nullptr;
    float* ssp = r.ks > 1 && NORM ? a.ws + (int64_t)r.ks * NS * MB * 16 * Np : nullptr;
    hipLaunchKernelGGL((wide_kernel<E, F, EPI, NORM, TPW>), dim3((unsigned)((tiles + 4 * TPW - 1) / (4 * TPW)), (unsigned)r.ks),
                       dim3(256), 0, a.st, a.M, a.x, a.ldx, a.W, a.ldw, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K,
                       a.na, part, ssp, r.cps);
    if (r.ks > 1)
        hipLaunchKernelGGL((wide_merge_kernel<E, EPI>), dim3((unsigned)((a.N + 255) / 256), (unsigned)a.M), dim3(256), 0,
                           a.st, a.M, r.ks, part, Np, ssp, F::kScaled ? (const float*)a.scale : nullptr, a.b, a.r, a.ldr,
                           a.y, a.ldy, a.N, a.K, a.na.eps);
}

template <int EPI, bool NORM, typename E, typename F>
void launch(const Args<E, F>& a) {
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;
    const Rules r = wide_rules(a.N, a.K, NS, F::H, NORM);
    if (r.ks > 1 && a.ws == nullptr) return;  // (the bindings pass wide_workspace() bytes; never launch without them)
    if constexpr (NS == 1) {
        if (r.tpw == 2) return launch_t<EPI, NORM, 2>(a, r);
    }
    launch_t<EPI, NORM, 1>(a, r);
}

template <typename E, typename F>
void launch_epi(int epi, int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const typename F::ST* scale,
                const void* b, const void* r, int64_t ldr, void* y, int64_t ldy, int N, int K, hipStream_t st,
                const void* norm_w, const void* norm_add, void* norm_sum, float eps, float* ws) {
    const Args<E, F> a{M, (const E*)x, ldx, (const typename F::T*)W, ldw, scale, (const E*)b, (const E*)r, ldr, (E*)y,
                       ldy, N, K, st, NormArgs<E>{(const E*)norm_w, (const E*)norm_add, (E*)norm_sum, eps}, ws};
    if (norm_w != nullptr) {
        if (epi == EPI_SWIGLU) launch<EPI_SWIGLU, true>(a);
        else launch<EPI_NONE, true>(a);
    } else if (epi == EPI_SWIGLU) {
        launch<EPI_SWIGLU, false>(a);
    } else if (epi == EPI_RES) {
        launch<EPI_RES, false>(a);
    } else {
        launch<EPI_NONE, false>(a);
    }
}

}  // namespace

namespace sa_launch {
// bytes of fp32 workspace wide() needs for these operands (0: the rule does not split K); fmt 0 dense, 1 FP8, 2 MXFP4
int64_t wide_workspace(int fmt, int M, int N, int K, int epi, bool norm) {
    const int ns = epi == EPI_SWIGLU ? 2 : 1;
    const Rules r = wide_rules(N, K, ns, fmt == 2 ? 4 : fmt == 1 ? 2 : 1, norm);
    if (r.ks <= 1) return 0;
    const int64_t tiles = (N + 15) / 16, MB = (M + 15) / 16;
    return ((int64_t)r.ks * ns * MB * 16 * tiles * 16 + (int64_t)r.ks * 64) * (int64_t)sizeof(float);
}
// the arguments of skinny (launch.h) for M <= 64, plus the workspace of wide_workspace() bytes (16-byte aligned)
void wide(int dtype, int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* scale, const void* b,
          void* y, int64_t ldy, int N, int K, hipStream_t st, int epi, const void* res, int64_t ldr, const void* norm_w,
          const void* norm_add, void* norm_sum, float eps, const uint8_t* bscale, float* ws) {
    if (M < 1 || M > 64 || N < 1 || K < 8) return;  // (the bindings reject these; never launch on them)
    if (bscale != nullptr) {
        if (K % 32 != 0) return;
        launch_epi<u16, MXFP4W>(epi, M, x, ldx, W, ldw, bscale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, ws);
    } else if (scale != nullptr)
        launch_epi<u16, E4M3W>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, ws);
    else if (dtype == DT_F16)
        launch_epi<_Float16, DenseW<_Float16>>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, ws);
    else
        launch_epi<u16, DenseW<u16>>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps, ws);
}
}  // namespace sa_launch
