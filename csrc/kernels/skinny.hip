// Decode-time linear layer on the matrix cores:  y[M, N] = x[M, K] W[N, K]^T (+ b)  for 1 <= M <= 16 input rows.
//
// gemv.hip streams W once and does the per-row work in fp32 FMAs, so its time grows with M (its 4-row kernels take
// 2.4-3.5x the 1-row time).  Here the weight stream is the same (cdna_hip_programming.md, "GEMV / M <= 16 decode
// weights": straight to VGPRs, deep unroll, late wait, no LDS round trip) but the arithmetic is one
// v_mfma_f32_16x16x32 per 16 weight rows x 32 k, whatever M is:
//  * A = a tile of 16 weight rows.  Lane l holds W[n0 + (l & 15)][k + 8 (l >> 4) + 0..7]: one 16-byte global load
//    IS the A fragment (no transpose, no LDS).  B = x: the same lane holds x[l & 15][the same k].  Lanes whose input
//    row (l & 15) >= M hold zeros and issue no load of x / add / res and no store: x may be exactly M rows long.
//  * D: lane l holds y[m = l & 15][n0 + 4 (l >> 4) + 0..3] in its four accumulators.
//  * A wave owns TPW consecutive tiles (x NS = 2 weight tiles each for SwiGLU: gate rows n and up rows F + n) and
//    reuses every x fragment for all of them, so x traffic (L1 / L2) is 1 / (NS TPW) of the weight stream at most.
//  * A trip is U consecutive 32-k steps of every tile (up to 8 weight loads per lane, 8 KiB per wave), so every
//    weight row contributes runs of 64 bytes per load instruction and 64 U bytes per trip; the next trip's loads are
//    issued before the current trip's MFMAs (two register buffers), so one wave per SIMD still overlaps memory and
//    arithmetic.
//  * KS = 4: the workgroup's four waves share the tiles and split K (interleaved trips, the workgroup streams
//    contiguous memory); partial accumulators go through LDS and wave 0 adds them in slice order 1, 2, 3.  No
//    atomics: results are bitwise deterministic.  KS = 1: every wave owns its own tiles and all of K.
// Launch rules (skinny_rules) depend on N, K, the weight format and the form, NEVER on M, and every output column
// of an MFMA is computed independently of the others: row m of y is bitwise the same whatever M is and whatever the
// other rows hold (batch invariance; tests/test_skinny_gpu.py).
//
// Bounds by construction: weight addresses are clamped (row min(n, N - 1), piece min(p, G - 1)) instead of
// predicated -- a clamped piece belongs to the same weight row and meets a zero x fragment, a clamped row feeds
// accumulators that are never stored -- so no weight row >= N and no k >= K is ever read; x / add loads are
// predicated on (row < M and k < K) and zero-filled, which also is the K tail (K % 8 == 0 dense, % 16 FP8; not
// necessarily a multiple of 32).
//
// Forms (those of gemv.hip, no RoPE form):  plain (+ bias);  RES: rnd(rnd(x W^T (+ b)) + res);  SWIGLU over
// W = [gate; up]: rnd(rnd(silu(g)) * u) with g, u rounded as the unfused kernel stores them;  NORM prologue
// (RMSNorm, optionally after s = rnd(x + add)) with epilogue plain or SWIGLU.  NORM rounding points:
//  * s = rnd(x + add): bit-identical to add_rms_norm's; written by the workgroup (KS = 4) / wave (KS = 1) of tile 0;
//  * sum(s^2) in fp32 per lane over its pieces in k order, then across the four k-groups of lanes (xor 16, xor 32)
//    and the K-split waves in slice order;
//  * the B operand is rnd(s * gamma): ONE rounding to the activation type (gemv.hip keeps this product in fp32, the
//    unfused path rounds s * rstd and * gamma separately);
//  * rstd = rsqrt(sum / K + eps) scales the fp32 accumulators at the end.
//
// FP8 weights (E4M3W, W = scale[n] * Q[n, :]): activations stay bf16, so the codes are decoded to bf16 in registers
// (v_cvt_pk_f32_fp8, keep the high half: exact, e4m3 has 3 mantissa bits and its subnormals are normal bf16 numbers)
// and feed the bf16 MFMA.  A 16-byte piece is 16 codes = two MFMAs of that lane's k (codes 0..7, 8..15 against
// x[16 p + 0..7], x[16 p + 8..15]).  The row's power-of-two scale multiplies the fp32 result once, after the
// reduction and before rstd / bias / epilogue; SwiGLU rows n and F + n keep their own scales.
//
// MXFP4 weights (MXFP4W, e2m1 codes in blocks of 32 k with one e8m0 scale byte; ops/quant.py): a lane's 16-byte load is
// 32 codes of one weight row = exactly one block, and four MFMAs of that lane's k (H = 4): codes 8 hh .. 8 hh + 7 are
// decoded to bf16 WITH the block scale by v_cvt_scalef32_pk_bf16_fp4 (exact: a code has 2 significant bits, the scale
// is a power of two) and meet x[32 p + 8 hh ..].  The scale byte is loaded with the piece (same clamped row and
// piece); nothing is scaled after the reduction.  Four x fragments per step: the per-trip budget shrinks to a quarter.
#include "common.h"
#include "launch.h"

using namespace sa;

namespace {

enum { EPI_NONE = 0, EPI_RES = 1, EPI_SWIGLU = 2 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// the activation type E: MFMA, and 8 elements <-> 8 floats of one 16-byte fragment (pack rounds to nearest even)
template <typename E> struct Act;
template <> struct Act<u16> {
    __device__ static __forceinline__ f32x4 mma(const u32x4& a, const u32x4& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    __device__ static __forceinline__ void unpack(const u32x4& r, float (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(r[i] << 16);
            v[2 * i + 1] = __uint_as_float(r[i] & 0xffff0000u);
        }
    }
    __device__ static __forceinline__ u32x4 pack(const float (&v)[8]) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (uint32_t)f2bf(v[2 * i]) | ((uint32_t)f2bf(v[2 * i + 1]) << 16);
        return r;
    }
};
template <> struct Act<_Float16> {
    __device__ static __forceinline__ f32x4 mma(const u32x4& a, const u32x4& b, const f32x4& c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    __device__ static __forceinline__ void unpack(const u32x4& r, float (&v)[8]) {
        const f16x8 h = __builtin_bit_cast(f16x8, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (float)h[i];
    }
    __device__ static __forceinline__ u32x4 pack(const float (&v)[8]) {
        f16x8 h;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = (_Float16)v[i];
        return __builtin_bit_cast(u32x4, h);
    }
};

// Weight formats: T the element type of W's pointer arithmetic (ldw counts T's), P weights per 16-byte piece, H MFMAs
// (8 weights of this lane each) per piece; frag(piece, hh) is the A fragment of the piece's hh-th MFMA.
template <typename E>
struct DenseW {
    typedef E T;
    static constexpr int P = 8, H = 1;
    static constexpr bool kScaled = false, kBlock = false;
    typedef float ST;
    __device__ static __forceinline__ u32x4 frag(const u32x4& w, int, float) { return w; }
};
struct E4M3W {
    typedef uint8_t T;
    static constexpr int P = 16, H = 2;
    static constexpr bool kScaled = true, kBlock = false;
    typedef float ST;
    // eight codes -> eight bf16 in memory order (e4m3x4_to_bf16, common.h)
    __device__ static __forceinline__ u32x4 frag(const u32x4& w, int hh, float) {
        u32x4 r;
        uint32_t a, b;
        e4m3x4_to_bf16(w[2 * hh], a, b);
        r[0] = a;
        r[1] = b;
        e4m3x4_to_bf16(w[2 * hh + 1], a, b);
        r[2] = a;
        r[3] = b;
        return r;
    }
};

// e2m1 codes, P = 32 per piece = one MX block (kBlock: ST one e8m0 byte per piece, rows of K / 32 contiguous)
struct MXFP4W {
    typedef uint8_t T;
    typedef uint8_t ST;
    static constexpr int P = 32, H = 4;
    static constexpr bool kScaled = false, kBlock = true;
    // dword hh = eight codes -> eight bf16 (code * block scale) in memory order: the low nibble of a byte is the even k
    __device__ static __forceinline__ u32x4 frag(const u32x4& w, int hh, float sc) {
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        u32x4 r;
        r[0] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[hh], sc, 0));
        r[1] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[hh], sc, 1));
        r[2] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[hh], sc, 2));
        r[3] = __builtin_bit_cast(uint32_t, (bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w[hh], sc, 3));
        return r;
    }
};

// the once-read weight stream; SA_SKINNY_NT=1 builds it with non-temporal loads (an A/B switch: slower, see the rules)
__device__ __forceinline__ u32x4 ld_w(const void* p) {
#if defined(SA_SKINNY_NT) && SA_SKINNY_NT
    return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
#else
    return *reinterpret_cast<const u32x4*>(p);
#endif
}

template <typename E>
struct NormArgs {
    const E* g;    // RMSNorm weight [K]
    const E* add;  // residual added before the norm ([M, K] contiguous) or nullptr
    E* sum;        // rnd(x + add) [M, K], written when add != nullptr
    float eps;
};

// one trip of a wave: U 32-k (dense) / 64-k (FP8) / 128-k (MXFP4) steps of NT weight tiles, and the x (add, gamma)
// pieces they meet; BS: the block scales of the weight pieces as floats
template <int NT, int U, int H, bool NORM, bool BS>
struct Trip {
    u32x4 w[NT][U];
    float s[BS ? NT : 1][BS ? U : 1];
    u32x4 x[U][H];
    u32x4 a[NORM ? U : 1][H];
    u32x4 g[NORM ? U : 1][H];
};

// TPW output tiles (16 columns of y each) per wave, KS waves (1 or 4) splitting K over the same tiles
template <typename E, typename F, int EPI, bool NORM, int KS, int TPW>
__global__ __launch_bounds__(256) void skinny_kernel(int M, const E* __restrict__ x, int64_t ldx,
                                                     const typename F::T* __restrict__ W, int64_t ldw,
                                                     const typename F::ST* __restrict__ scale, const E* __restrict__ bias,
                                                     const E* __restrict__ res, int64_t ldr, E* __restrict__ y,
                                                     int64_t ldy, int N, int K, NormArgs<E> na) {
    constexpr int NS = EPI == EPI_SWIGLU ? 2 : 1;  // weight tiles per output tile
    constexpr int NT = NS * TPW;                   // weight tiles per wave
    constexpr int P = F::P, H = F::H;
    // steps per trip: NT U weight loads per lane and buffer, two buffers (8 - 16 KiB per wave in flight for the plain
    // dense forms); halved where a step also holds add / gamma (NORM) or two x fragments (FP8), and again for the four
    // x fragments of MXFP4, to stay in registers
    constexpr int BUD = 8 >> ((NORM ? 1 : 0) + (H == 2 ? 1 : 0) + (H == 4 ? 2 : 0));
    constexpr int U = BUD / NT > 4 ? 4 : (BUD / NT < 1 ? 1 : BUD / NT);
    static_assert(NT <= 8 && (KS == 1 || KS == 4), "tiles per wave / K split");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int c = lane & 15, h = lane >> 4;  // input row m (= weight row inside the tile) and k-group
    const int kw = KS > 1 ? wv : 0;          // this wave's K slice
    const int tile0 = (KS > 1 ? (int)blockIdx.x : (int)blockIdx.x * 4 + wv) * TPW;
    if (tile0 * 16 >= N) return;  // KS == 1 only (wave-uniform, no barrier on that path); never true for KS == 4
    const int G = K / P;          // 16-byte pieces per weight row
    const bool row_ok = c < M;

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
    const E* xr = x + (int64_t)c * ldx;                       // dereferenced only when row_ok
    const bool has_add = NORM && na.add != nullptr;
    const E* ar = has_add ? na.add + (int64_t)c * K : nullptr;  // likewise
    const bool write_s = has_add && tile0 == 0;

    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float ss = 0.f;

    typedef Trip<NT, U, H, NORM, F::kBlock> TripT;
    // this lane's piece of step u of trip t
    auto piece = [&](int t, int u) { return (t * KS + kw) * (4 * U) + 4 * u + h; };
    auto load = [&](TripT& tr, int t) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int p = piece(t, u);
            const int pc = min(p, G - 1);  // clamped: the same row's last piece, met by a zero x fragment
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                tr.w[j][u] = ld_w(wp[j] + (int64_t)pc * (16 / (int)sizeof(typename F::T)));
                if constexpr (F::kBlock) tr.s[j][u] = __uint_as_float((uint32_t)sp[j][pc] << 23);
            }
            const bool ok = row_ok && p < G;
#pragma unroll
            for (int hh = 0; hh < H; ++hh) {
                tr.x[u][hh] = u32x4{0u, 0u, 0u, 0u};
                if (ok) tr.x[u][hh] = *reinterpret_cast<const u32x4*>(xr + (int64_t)p * P + 8 * hh);
                if constexpr (NORM) {
                    tr.g[u][hh] = *reinterpret_cast<const u32x4*>(na.g + (int64_t)pc * P + 8 * hh);
                    tr.a[u][hh] = u32x4{0u, 0u, 0u, 0u};
                    if (ok && has_add) tr.a[u][hh] = *reinterpret_cast<const u32x4*>(ar + (int64_t)p * P + 8 * hh);
                }
            }
        }
    };
    auto compute = [&](const TripT& tr, int t) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int hh = 0; hh < H; ++hh) {
                u32x4 b = tr.x[u][hh];
                if constexpr (NORM) {
                    float xv[8], gv[8];
                    Act<E>::unpack(b, xv);
                    if (has_add) {
                        float av[8];
                        Act<E>::unpack(tr.a[u][hh], av);
#pragma unroll
                        for (int i = 0; i < 8; ++i) xv[i] = rnd<E>(xv[i] + av[i]);
                        const int p = piece(t, u);
                        if (write_s && row_ok && p < G)
                            *reinterpret_cast<u32x4*>(na.sum + (int64_t)c * K + (int64_t)p * P + 8 * hh) = Act<E>::pack(xv);
                    }
                    Act<E>::unpack(tr.g[u][hh], gv);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        ss = __builtin_fmaf(xv[i], xv[i], ss);
                        xv[i] *= gv[i];
                    }
                    b = Act<E>::pack(xv);  // rnd(s * gamma)
                }
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[j] = Act<E>::mma(F::frag(tr.w[j][u], hh, F::kBlock ? tr.s[j][u] : 0.f), b, acc[j]);
            }
        }
    };

    // every wave runs the same number of trips; trips past its share of K are all-clamped / all-zero
    const int T = (G + 4 * U * KS - 1) / (4 * U * KS);
    TripT ta, tb;
    load(ta, 0);
    for (int t = 0; t < T; t += 2) {
        if (t + 1 < T) load(tb, t + 1);
        compute(ta, t);
        if (t + 1 < T) {
            if (t + 2 < T) load(ta, t + 2);
            compute(tb, t + 1);
        }
    }
    if constexpr (NORM) {  // the four k-groups of lanes hold the same input row
        ss += __shfl_xor(ss, 16, 64);
        ss += __shfl_xor(ss, 32, 64);
    }
    if constexpr (KS > 1) {
        // partial sums of the K slices: waves 1..KS-1 -> LDS, wave 0 adds them in slice order
        __shared__ float red[KS - 1][NT * 4 + 1][64];
        if (kw > 0) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[kw - 1][j * 4 + r][lane] = acc[j][r];
            red[kw - 1][NT * 4][lane] = ss;
        }
        __syncthreads();
        if (kw > 0) return;
#pragma unroll
        for (int k = 0; k < KS - 1; ++k) {
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[j][r] += red[k][j * 4 + r][lane];
            ss += red[k][NT * 4][lane];
        }
    }
    if (!row_ok) return;
    const float rstd = NORM ? rsqrtf(ss / K + na.eps) : 1.f;
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = (tile0 + j) * 16 + 4 * h + r;
            if (n >= N) continue;
            float v = acc[j][r];
            if constexpr (F::kScaled) v *= scale[n];  // the row's power of two: exact
            if constexpr (NORM) v *= rstd;
            if constexpr (EPI == EPI_SWIGLU) {
                float up = acc[TPW + j][r];
                if constexpr (F::kScaled) up *= scale[(int64_t)N + n];
                if constexpr (NORM) up *= rstd;
                const float a = rnd<E>(v), b = rnd<E>(up);
                v = rnd<E>(a / (1.f + __expf(-a))) * b;
            } else {
                if (bias != nullptr) v += IO<E>::ld(bias, n);
                if constexpr (EPI == EPI_RES) v = rnd<E>(v) + IO<E>::ld(res, (int64_t)c * ldr + n);
            }
            IO<E>::st(y, (int64_t)c * ldy + n, v);
        }
    }
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
};

// Launch rules, from N (output columns) and the form, nothing else -- in particular not M (batch invariance):
//  * at most 2048 weight tiles (twice the device's 1024 SIMDs): the workgroup's four waves split K, so that the
//    o / down projections (256 tiles) still put a wave on every SIMD; above, a wave owns its tiles' whole K;
//  * two output tiles per wave once that leaves a workgroup per CU (512 tiles), one below.
// A/B on the five 7B shapes (profiles/skinny_variants.log): K split over 8 / 16 waves and one tile per wave (more
// waves, less reuse of x) gained 10-22 % at M = 2 on o, gate/up and the head but lost 9-11 % at M = 16 on down and
// the head, where the x fragments' L2 traffic is what grows; non-temporal weight loads lost 2-14 % everywhere.
struct Rules {
    int ks, tpw;
};
Rules skinny_rules(int N, int ns) {
    const int tiles = (N + 15) / 16;
    if (tiles * ns > 2048) return {1, 2};
    return {4, tiles >= 512 ? 2 : 1};
}

template <int EPI, bool NORM, int KS, int TPW, typename E, typename F>
void launch_t(const Args<E, F>& a) {
    const int tiles = (a.N + 15) / 16;
    const int per_wg = TPW * (KS > 1 ? 1 : 4);
    hipLaunchKernelGGL((skinny_kernel<E, F, EPI, NORM, KS, TPW>), dim3((unsigned)((tiles + per_wg - 1) / per_wg)),
                       dim3(256), 0, a.st, a.M, a.x, a.ldx, a.W, a.ldw, a.scale, a.b, a.r, a.ldr, a.y, a.ldy, a.N, a.K,
                       a.na);
}

template <int EPI, bool NORM, typename E, typename F>
void launch(const Args<E, F>& a) {
    const Rules r = skinny_rules(a.N, EPI == EPI_SWIGLU ? 2 : 1);
    if (r.ks == 1) launch_t<EPI, NORM, 1, 2>(a);
    else if (r.tpw == 2) launch_t<EPI, NORM, 4, 2>(a);
    else launch_t<EPI, NORM, 4, 1>(a);
}

template <typename E, typename F>
void launch_epi(int epi, int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const typename F::ST* scale,
                const void* b, const void* r, int64_t ldr, void* y, int64_t ldy, int N, int K, hipStream_t st,
                const void* norm_w, const void* norm_add, void* norm_sum, float eps) {
    const Args<E, F> a{M, (const E*)x, ldx, (const typename F::T*)W, ldw, scale, (const E*)b, (const E*)r, ldr, (E*)y,
                       ldy, N, K, st, NormArgs<E>{(const E*)norm_w, (const E*)norm_add, (E*)norm_sum, eps}};
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
// epi 0: y = x W^T (+ b); 1: y = rnd(x W^T (+ b)) + res; 2: SwiGLU over W = [gate; up] (N = F output columns).
// norm_w != nullptr (epi 0 / 2): x is first replaced by rms_norm(x (+ norm_add), norm_w, eps) inside the same pass.
// scale != nullptr: W holds e4m3fn codes (rows ldw bytes apart), x / b / res / y / norm_* are bf16 whatever dtype says.
// bscale != nullptr: W holds e2m1 codes, two per byte, bscale one e8m0 byte per 32 k ([N, K / 32] contiguous; launch.h).
void skinny(int dtype, int M, const void* x, int64_t ldx, const void* W, int64_t ldw, const float* scale, const void* b,
            void* y, int64_t ldy, int N, int K, hipStream_t st, int epi, const void* res, int64_t ldr, const void* norm_w,
            const void* norm_add, void* norm_sum, float eps, const uint8_t* bscale) {
    if (M < 1 || M > 16 || N < 1 || K < 8) return;  // (the bindings reject these; never launch on them)
    if (bscale != nullptr) {
        if (K % 32 != 0) return;
        launch_epi<u16, MXFP4W>(epi, M, x, ldx, W, ldw, bscale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps);
    } else if (scale != nullptr)
        launch_epi<u16, E4M3W>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps);
    else if (dtype == DT_F16)
        launch_epi<_Float16, DenseW<_Float16>>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps);
    else
        launch_epi<u16, DenseW<u16>>(epi, M, x, ldx, W, ldw, scale, b, res, ldr, y, ldy, N, K, st, norm_w, norm_add, norm_sum, eps);
}
}  // namespace sa_launch
