// SwiGLU and rotary-embedding kernels (memory-bound; 16 B per lane per access).
#include "common.h"
#include "launch.h"

using namespace sa;

// ------------------------------------------------------------------ SwiGLU
// out[t, j] = rnd(silu(a[t, j])) * b[t, j]  (torch: silu(x) then * y, each rounded to the storage type)
template <typename T>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(const T* __restrict__ a, const T* __restrict__ b, int64_t lda,
                                                         T* __restrict__ out, int64_t rows, int F) {
    const int vpr = F / 8;
    const int64_t n = rows * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / vpr;
        const int c = (int)(i - r * vpr) * 8;
        float av[8], bv[8], o[8];
        V8<T>::ld(a + r * lda + c, av);
        V8<T>::ld(b + r * lda + c, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float s = av[j] / (1.f + __expf(-av[j]));
            o[j] = rnd<T>(s) * bv[j];
        }
        V8<T>::st(out + r * F + c, o);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ a,
                                                         const T* __restrict__ b, int64_t lda, T* __restrict__ da,
                                                         T* __restrict__ db, int64_t ldd, int64_t rows, int F) {
    const int vpr = F / 8;
    const int64_t n = rows * vpr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / vpr;
        const int c = (int)(i - r * vpr) * 8;
        float g[8], av[8], bv[8], oa[8], ob[8];
        V8<T>::ld(dy + r * F + c, g);
        V8<T>::ld(a + r * lda + c, av);
        V8<T>::ld(b + r * lda + c, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float sig = 1.f / (1.f + __expf(-av[j]));
            const float s = av[j] * sig;
            ob[j] = g[j] * rnd<T>(s);
            const float ds = g[j] * bv[j];
            oa[j] = ds * (sig * (1.f + av[j] * (1.f - sig)));
        }
        V8<T>::st(da + r * ldd + c, oa);
        V8<T>::st(db + r * ldd + c, ob);
    }
}

// ------------------------------------------------------------------ RoPE
// x, out: [T, nh, hd] with arbitrary token/head strides (elements, unit element stride); out may alias x
// (every work item reads its elements before writing the same elements), which the fused attention
// backward uses to rotate dq/dk in place inside the dQKV buffer.
// table: fp32 cos/sin [max_pos, rd/2] (NeoX: pair (i, i+rd/2); complex: pair (2i, 2i+1)).
// sign = +1 forward, -1 backward (rotation transpose). Dims >= rd are copied through.
struct RopeArgs {
    int64_t xt, xh, ot, oh;  // token / head strides of x and out
    const float* cosb;
    const float* sinb;
    const int64_t* pos;
    int T, nh, hd, rd, seq_len;
    float sign;
};

// Vector path: one work item = 8 pair slots of one (token, head) row — NeoX: elements p..p+7 and
// half+p..half+p+7 (two 16 B loads); complex: elements e..e+7 (four pairs, one 16 B load); the
// pass-through tail [rd, hd) moves in 8-element chunks.  Needs 16 B aligned rows (checked on host).
template <typename T, bool IL>
__global__ __launch_bounds__(256) void rope_v8_kernel(const T* __restrict__ x, T* __restrict__ out, RopeArgs a) {
    const int half = a.rd / 2;
    const int rc = IL ? a.rd / 8 : half / 8;  // rotating chunks per row
    const int CR = rc + (a.hd - a.rd) / 8;
    const int n = a.T * a.nh * CR;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int row = i / CR, c = i - row * CR;
        const int t = row / a.nh, h = row - t * a.nh;
        const T* xr = x + t * a.xt + h * a.xh;
        T* orow = out + t * a.ot + h * a.oh;
        if (c < rc) {
            const int64_t ps = a.pos ? a.pos[t] : (t % a.seq_len);
            const float* cb = a.cosb + ps * half;
            const float* sb = a.sinb + ps * half;
            if (!IL) {
                const int p = c * 8;
                float x0[8], x1[8], cs[8], sn[8], o0[8], o1[8];
                V8<T>::ld(xr + p, x0);
                V8<T>::ld(xr + half + p, x1);
                V8<float>::ld(cb + p, cs);
                V8<float>::ld(sb + p, sn);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float sj = sn[j] * a.sign;
                    rot_pair(x0[j], x1[j], cs[j], sj, o0[j], o1[j]);
                }
                V8<T>::st(orow + p, o0);
                V8<T>::st(orow + half + p, o1);
            } else {
                const int e = c * 8;
                float v[8], o[8];
                V8<T>::ld(xr + e, v);
                const f32x4 cs = *reinterpret_cast<const f32x4*>(cb + e / 2);
                const f32x4 sn = *reinterpret_cast<const f32x4*>(sb + e / 2);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sj = sn[j] * a.sign;
                    rot_pair(v[2 * j], v[2 * j + 1], cs[j], sj, o[2 * j], o[2 * j + 1]);
                }
                V8<T>::st(orow + e, o);
            }
        } else {
            const int e = a.rd + (c - rc) * 8;
            float v[8];
            V8<T>::ld(xr + e, v);
            V8<T>::st(orow + e, v);
        }
    }
}

// Scalar fallback (odd rotary dims / unaligned views): one thread per (token, head, pair).
template <typename T, bool INTERLEAVED>
__global__ __launch_bounds__(256) void rope_kernel(const T* __restrict__ x, T* __restrict__ out, RopeArgs a) {
    const int half = a.rd / 2;
    const int pairs = half + (a.hd - a.rd + 1) / 2;  // rotated pairs + pass-through element pairs
    const int64_t n = (int64_t)a.T * a.nh * pairs;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % pairs);
        const int64_t th = i / pairs;
        const int h = (int)(th % a.nh);
        const int64_t t = th / a.nh;
        const T* xr = x + t * a.xt + (int64_t)h * a.xh;
        T* orow = out + t * a.ot + (int64_t)h * a.oh;
        if (p < half) {
            const int64_t ps = a.pos ? a.pos[t] : (t % a.seq_len);
            const float c = a.cosb[ps * half + p];
            const float s = a.sinb[ps * half + p] * a.sign;
            const int i0 = INTERLEAVED ? 2 * p : p;
            const int i1 = INTERLEAVED ? 2 * p + 1 : p + half;
            const float x0 = IO<T>::ld(xr, i0), x1 = IO<T>::ld(xr, i1);
            float r0, r1;
            rot_pair(x0, x1, c, s, r0, r1);
            IO<T>::st(orow, i0, r0);
            IO<T>::st(orow, i1, r1);
        } else {
            const int j = a.rd + 2 * (p - half);
            const T v0 = xr[j];
            const T v1 = j + 1 < a.hd ? xr[j + 1] : v0;
            orow[j] = v0;
            if (j + 1 < a.hd) orow[j + 1] = v1;
        }
    }
}

// Graph-decode step (one token per sequence): RoPE of the q and k heads and the K/V cache append in ONE launch.  x is
// the QKV projection [B][nq + 2 nkv heads][hd] (contiguous), blockIdx.y = b the sequence; q heads are rotated into
// q_out [b][nq][hd]; k heads are rotated straight into row b * cap + pos[b] of the K cache and v heads copied into the
// same row of the V cache ([B * cap][nkv][hd] each: one slab of cap rows per sequence; B = 1 is the one-sequence
// cache) -- replacing rope(q), rope(k) and two index_copy launches.  One work item = 8 pair slots (as rope_v8_kernel).
// lim = min(cap, rotary table rows): a sequence whose position is outside [0, lim) writes no cache row, zeros its own
// q row and sets *err (the caller checks the word on the host; an out-of-range row index would otherwise write past
// its slab silently); the other sequences are unaffected.
// Chunk c of one row of the append step (CR = rc + (hd - rd) / 8 chunks, rc of them rotating, as rope_v8_kernel): the
// values before rounding, a[8] for elements ea.. and -- NeoX rotating chunks -- b[8] for elements eb.. (eb < 0: none).
// Shared by the bf16 and the FP8 append kernels, so both round the same numbers.
template <typename T, bool IL>
__device__ __forceinline__ void append_chunk(const T* xr, int c, int rc, int half, int rd, const float* cb,
                                             const float* sb, float (&a)[8], float (&b)[8], int& ea, int& eb) {
    eb = -1;
    if (c < rc) {
        if (!IL) {
            const int p = c * 8;
            float x0[8], x1[8], cs[8], sn[8];
            V8<T>::ld(xr + p, x0);
            V8<T>::ld(xr + half + p, x1);
            V8<float>::ld(cb + p, cs);
            V8<float>::ld(sb + p, sn);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                rot_pair(x0[j], x1[j], cs[j], sn[j], a[j], b[j]);
            }
            ea = p;
            eb = half + p;
        } else {
            const int e = c * 8;
            float v[8];
            V8<T>::ld(xr + e, v);
            const f32x4 cs = *reinterpret_cast<const f32x4*>(cb + e / 2);
            const f32x4 sn = *reinterpret_cast<const f32x4*>(sb + e / 2);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                rot_pair(v[2 * j], v[2 * j + 1], cs[j], sn[j], a[2 * j], a[2 * j + 1]);
            }
            ea = e;
        }
    } else {
        ea = rd + (c - rc) * 8;
        V8<T>::ld(xr + ea, a);
    }
}

// Paged form (template flag PG; AppendPages): the caches are a pool of pages and sequence b's row is
// table[b][pos / page] * page + pos % page; lim = min(table width * page, rotary table rows).  A table entry outside
// [0, num_pages) is a position error like a position outside [0, lim): nothing is written, q is zeroed, bit 0 of *err.
// Rotation, quantisation and q_out are the slab form's code.  The paged kernels are the instantiations with one trailing
// AppendPages argument (the pack P); with the empty pack the kernels keep the slab form's signature and code.
template <typename A>
__device__ __forceinline__ const A& only_arg(const A& a) { return a; }

template <typename T, bool IL, typename... P>
__global__ __launch_bounds__(256) void rope_kv_append_kernel(const T* __restrict__ x, T* __restrict__ q_out,
                                                             T* __restrict__ kc, T* __restrict__ vc,
                                                             const int64_t* __restrict__ pos, const float* cosb,
                                                             const float* sinb, int nq, int nkv, int hd, int rd,
                                                             int64_t lim, int64_t cap, int* __restrict__ err,
                                                             P... pages) {
    constexpr bool PG = sizeof...(P) == 1;
    const int half = rd / 2;
    const int rc = IL ? rd / 8 : half / 8;
    const int CR = rc + (hd - rd) / 8;
    const int nh = nq + 2 * nkv;
    const int b = blockIdx.y;
    const int64_t ps = pos[b];
    x += (int64_t)b * nh * hd;
    q_out += (int64_t)b * nq * hd;
    bool bad = false;
    int64_t prow = 0;  // paged: the pool row
    if constexpr (PG) {
        const AppendPages& pg = only_arg(pages...);
        bad = ps < 0 || ps >= lim;
        if (!bad) {
            const int e = pg.table[b * pg.stride + ps / pg.page];
            bad = (unsigned)e >= (unsigned)pg.num_pages;
            prow = (int64_t)e * pg.page + ps % pg.page;
        }
    }
    auto cache_row = [&]() -> int64_t {
        if constexpr (PG) return prow;
        else return b * cap + ps;
    };
    if (PG ? bad : (ps < 0 || ps >= lim)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *err = 1;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nq * hd / 8; i += gridDim.x * blockDim.x) {
            const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            V8<T>::st(q_out + 8 * i, z);
        }
        return;
    }
    const int n = nh * CR;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int h = i / CR, c = i - h * CR;
        const T* xr = x + (int64_t)h * hd;
        T* orow;
        if (h < nq) orow = q_out + (int64_t)h * hd;
        else if (h < nq + nkv) orow = kc + (cache_row() * nkv + (h - nq)) * hd;
        else orow = vc + (cache_row() * nkv + (h - nq - nkv)) * hd;
        if (h >= nq + nkv) {  // v: plain copy of the row's chunks
            for (int e = 8 * c; e < hd; e += 8 * CR) {
                float v[8];
                V8<T>::ld(xr + e, v);
                V8<T>::st(orow + e, v);
            }
            continue;
        }
        float o0[8], o1[8];
        int e0, e1;
        append_chunk<T, IL>(xr, c, rc, half, rd, cosb + ps * half, sinb + ps * half, o0, o1, e0, e1);
        V8<T>::st(orow + e0, o0);
        if (e1 >= 0) V8<T>::st(orow + e1, o1);
    }
}

// a k / v value as the bf16 cache would hold it; NaN becomes 0 and a magnitude above 2^127 (infinity included) +-2^127:
// a row whose amax lies in (240 * 2^120, bf16 max] would round it to the code of 256 at scale 2^120, and 256 * 2^120 is
// 2^128, infinite in bf16.  The cut sits at the power of two below, 2^127, where amax / s <= 448 * 2^119 stays finite
// (ops/quant.py sanitize_kv is the torch form)
__device__ __forceinline__ float kv_finite_bf(float v, bool& bad) {
    uint32_t u = f2bf(v);
    if ((u & 0x7fffu) > 0x7f00u) {
        bad = true;
        u = (u & 0x7fffu) > 0x7f80u ? 0u : ((u & 0x8000u) | 0x7f00u);
    }
    return bf2f((u16)u);
}
// eight values times inv -> eight e4m3fn codes (v_cvt_pk_fp8_f32: round to nearest even), in memory order
__device__ __forceinline__ uint2 e4m3_pack8(const float (&v)[8], float inv) {
    int w0 = 0, w1 = 0;
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0] * inv, v[1] * inv, w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2] * inv, v[3] * inv, w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4] * inv, v[5] * inv, w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6] * inv, v[7] * inv, w1, true);
    return make_uint2((uint32_t)w0, (uint32_t)w1);
}

// rope_kv_append_kernel over an FP8 K/V cache (bf16 x): kc / vc hold e4m3fn codes [B * cap][nkv][hd], one byte each, and
// k_scale / v_scale [nkv][s_head] one fp32 power-of-two scale per (kv head, cache row).  Waves [0, 2 nkv) of a sequence
// take one k or v head each, so the row's amax is one 64-lane reduction: lane c holds chunk c of the row (append_chunk:
// the numbers the bf16 kernel rounds), rounds it to bf16 -- the value the bf16 cache would hold --, and the row is
// quantised as ops/quant.py quantize_rows_fp8 does: s = 2^e the smallest power of two with amax <= 448 s, e >= -100,
// s = 1 for an all-zero row, formed from amax's exponent and mantissa bits (amax / 448 = m 2^e with m <= 1/2 exactly
// when amax's significand is <= 1.75); codes = e4m3(value / s), |value / s| <= 448 by construction.  The remaining
// waves rotate the q heads, one lane per chunk as the bf16 kernel (q_out is bitwise its output).  A non-finite k / v
// value never becomes the NaN code: kv_finite_bf replaces it and bit 1 of *err is set; bit 0 is the position error.
template <bool IL, typename... P>
__global__ __launch_bounds__(256) void rope_kv_append_q8_kernel(const u16* __restrict__ x, u16* __restrict__ q_out,
                                                                uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                                float* __restrict__ k_scale, float* __restrict__ v_scale,
                                                                int64_t s_head, const int64_t* __restrict__ pos,
                                                                const float* cosb, const float* sinb, int nq, int nkv,
                                                                int hd, int rd, int64_t lim, int64_t cap,
                                                                int* __restrict__ err, P... pages) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr bool PG = sizeof...(P) == 1;
    const int half = rd / 2;
    const int rc = IL ? rd / 8 : half / 8;
    const int CR = rc + (hd - rd) / 8;
    const int nh = nq + 2 * nkv;
    const int b = blockIdx.y;
    const int64_t ps = pos[b];
    x += (int64_t)b * nh * hd;
    q_out += (int64_t)b * nq * hd;
    bool oob = false;
    int64_t prow = 0;  // paged: the pool row
    if constexpr (PG) {
        const AppendPages& pg = only_arg(pages...);
        oob = ps < 0 || ps >= lim;
        if (!oob) {
            const int e = pg.table[b * pg.stride + ps / pg.page];
            oob = (unsigned)e >= (unsigned)pg.num_pages;
            prow = (int64_t)e * pg.page + ps % pg.page;
        }
    }
    if (PG ? oob : (ps < 0 || ps >= lim)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(err, 1);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nq * hd / 8; i += gridDim.x * blockDim.x) {
            const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            V8<u16>::st(q_out + 8 * i, z);
        }
        return;
    }
    const float* cb = cosb + ps * half;
    const float* sb = sinb + ps * half;
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);  // wave-uniform
    if (w >= 2 * nkv) {  // q heads
        const int i = (w - 2 * nkv) * 64 + lane;
        if (i < nq * CR) {
            const int h = i / CR, c = i - h * CR;
            float o0[8], o1[8];
            int e0, e1;
            append_chunk<u16, IL>(x + (int64_t)h * hd, c, rc, half, rd, cb, sb, o0, o1, e0, e1);
            V8<u16>::st(q_out + (int64_t)h * hd + e0, o0);
            if (e1 >= 0) V8<u16>::st(q_out + (int64_t)h * hd + e1, o1);
        }
        return;
    }
    const bool isv = w >= nkv;
    const int hk = isv ? w - nkv : w;
    const u16* xr = x + (int64_t)(nq + w) * hd;  // heads are ordered q | k | v
    float o0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int e0 = -1, e1 = -1;
    if (isv) {
        if (lane < hd / 8) {
            e0 = 8 * lane;
            V8<u16>::ld(xr + e0, o0);
        }
    } else if (lane < CR) {
        append_chunk<u16, IL>(xr, lane, rc, half, rd, cb, sb, o0, o1, e0, e1);
    }
    bool bad = false;
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        o0[j] = kv_finite_bf(o0[j], bad);
        o1[j] = kv_finite_bf(o1[j], bad);
        am = fmaxf(am, fmaxf(fabsf(o0[j]), fabsf(o1[j])));
    }
    am = wave_max(am);
    const uint32_t bits = __float_as_uint(am);
    const int E = (int)(bits >> 23);
    int es = (bits & 0x7fffffu) <= 0x600000u ? E - 135 : E - 134;
    if (es < -100) es = -100;  // covers the subnormal amax (E == 0)
    const float s = bits == 0u ? 1.f : __uint_as_float((uint32_t)(es + 127) << 23);
    const float inv = bits == 0u ? 1.f : __uint_as_float((uint32_t)(127 - es) << 23);
    const int64_t row = PG ? prow : (int64_t)b * cap + ps;
    uint8_t* orow = (isv ? vc : kc) + (row * nkv + hk) * hd;
    if (e0 >= 0) *reinterpret_cast<uint2*>(orow + e0) = e4m3_pack8(o0, inv);
    if (e1 >= 0) *reinterpret_cast<uint2*>(orow + e1) = e4m3_pack8(o1, inv);
    if (lane == 0) (isv ? v_scale : k_scale)[(int64_t)hk * s_head + row] = s;
    if (__any(bad) && lane == 0) atomicOr(err, 2);
#endif
}

static int grid_for(int64_t n) {
    int64_t g = (n + 255) / 256;
    return (int)(g < 8192 ? (g < 1 ? 1 : g) : 8192);
}

namespace sa_launch {
bool rope_kv_append(int dtype, bool interleaved, const void* x, void* q_out, void* kc, void* vc, const int64_t* pos,
                    const float* cosb, const float* sinb, int nq, int nkv, int hd, int rd, int64_t lim, int* err,
                    hipStream_t st, int B, int64_t cap, float* k_scale, float* v_scale, int64_t s_head,
                    const AppendPages* pages) {
    const AppendPages pg = pages != nullptr ? *pages : AppendPages{nullptr, 0, 0, 0};
    if (pages != nullptr && (pg.table == nullptr || pg.page < 1 || pg.num_pages < 1)) return false;
    if (dtype == DT_F32 || hd % 8 || (interleaved ? rd % 8 : rd % 16) || B < 1 || B > 65535) return false;
    const int CR = (interleaved ? rd / 8 : rd / 16) + (hd - rd) / 8;
    if (k_scale != nullptr) {  // FP8 cache: one wave per k / v head, then the q chunks
        if (dtype != DT_BF16 || v_scale == nullptr || hd > 512) return false;
        const dim3 g((2 * nkv + (nq * CR + 63) / 64 + 3) / 4, B);
#define SA_RKV8(IL)                                                                                                 \
    hipLaunchKernelGGL((rope_kv_append_q8_kernel<IL>), g, 256, 0, st, (const u16*)x, (u16*)q_out, (uint8_t*)kc,      \
                       (uint8_t*)vc, k_scale, v_scale, s_head, pos, cosb, sinb, nq, nkv, hd, rd, lim, cap, err)
#define SA_RKV8P(IL)                                                                                                  \
    hipLaunchKernelGGL((rope_kv_append_q8_kernel<IL, AppendPages>), g, 256, 0, st, (const u16*)x, (u16*)q_out,        \
                       (uint8_t*)kc, (uint8_t*)vc, k_scale, v_scale, s_head, pos, cosb, sinb, nq, nkv, hd, rd, lim,   \
                       cap, err, pg)
        if (pages != nullptr) { if (interleaved) SA_RKV8P(true); else SA_RKV8P(false); }
        else { if (interleaved) SA_RKV8(true); else SA_RKV8(false); }
#undef SA_RKV8P
#undef SA_RKV8
        return true;
    }
    const dim3 g(grid_for((int64_t)(nq + 2 * nkv) * CR), B);
#define SA_RKV(TT, IL)                                                                                            \
    hipLaunchKernelGGL((rope_kv_append_kernel<TT, IL>), g, 256, 0, st, (const TT*)x, (TT*)q_out, (TT*)kc, (TT*)vc, \
                       pos, cosb, sinb, nq, nkv, hd, rd, lim, cap, err)
#define SA_RKVP(TT, IL)                                                                                            \
    hipLaunchKernelGGL((rope_kv_append_kernel<TT, IL, AppendPages>), g, 256, 0, st, (const TT*)x, (TT*)q_out,      \
                       (TT*)kc, (TT*)vc, pos, cosb, sinb, nq, nkv, hd, rd, lim, cap, err, pg)
    if (pages != nullptr) {
        if (dtype == DT_BF16) { if (interleaved) SA_RKVP(u16, true); else SA_RKVP(u16, false); }
        else { if (interleaved) SA_RKVP(f16, true); else SA_RKVP(f16, false); }
    } else {
        if (dtype == DT_BF16) { if (interleaved) SA_RKV(u16, true); else SA_RKV(u16, false); }
        else { if (interleaved) SA_RKV(f16, true); else SA_RKV(f16, false); }
    }
#undef SA_RKVP
#undef SA_RKV
    return true;
}
void swiglu_fwd(int dtype, const void* a, const void* b, int64_t lda, void* out, int64_t rows, int F, hipStream_t st) {
    const int g = grid_for(rows * (F / 8));
    if (dtype == DT_BF16) hipLaunchKernelGGL(swiglu_fwd_kernel<u16>, g, 256, 0, st, (const u16*)a, (const u16*)b, lda, (u16*)out, rows, F);
    else if (dtype == DT_F16) hipLaunchKernelGGL(swiglu_fwd_kernel<f16>, g, 256, 0, st, (const f16*)a, (const f16*)b, lda, (f16*)out, rows, F);
    else hipLaunchKernelGGL(swiglu_fwd_kernel<float>, g, 256, 0, st, (const float*)a, (const float*)b, lda, (float*)out, rows, F);
}
void swiglu_bwd(int dtype, const void* dy, const void* a, const void* b, int64_t lda, void* da, void* db, int64_t ldd,
                int64_t rows, int F, hipStream_t st) {
    const int g = grid_for(rows * (F / 8));
    if (dtype == DT_BF16) hipLaunchKernelGGL(swiglu_bwd_kernel<u16>, g, 256, 0, st, (const u16*)dy, (const u16*)a, (const u16*)b, lda, (u16*)da, (u16*)db, ldd, rows, F);
    else if (dtype == DT_F16) hipLaunchKernelGGL(swiglu_bwd_kernel<f16>, g, 256, 0, st, (const f16*)dy, (const f16*)a, (const f16*)b, lda, (f16*)da, (f16*)db, ldd, rows, F);
    else hipLaunchKernelGGL(swiglu_bwd_kernel<float>, g, 256, 0, st, (const float*)dy, (const float*)a, (const float*)b, lda, (float*)da, (float*)db, ldd, rows, F);
}
void rope(int dtype, bool interleaved, const void* x, int64_t x_tok, int64_t x_head, void* out, int64_t o_tok,
          int64_t o_head, const float* cosb, const float* sinb, const int64_t* pos, int64_t T_, int nh, int hd, int rd,
          int seq_len, float sign, hipStream_t st) {
    const RopeArgs a{x_tok, x_head, o_tok, o_head, cosb, sinb, pos, (int)T_, nh, hd, rd, seq_len, sign};
    const int vec_elems = dtype == DT_F32 ? 4 : 8;  // 16 B
    const bool aligned = ((uintptr_t)x % 16 == 0) && ((uintptr_t)out % 16 == 0) && x_tok % vec_elems == 0 &&
                         x_head % vec_elems == 0 && o_tok % vec_elems == 0 && o_head % vec_elems == 0;
    const bool vec = aligned && hd % 8 == 0 && (interleaved ? rd % 8 == 0 : rd % 16 == 0) &&
                     T_ * nh * (hd / 8) < (int64_t)INT32_MAX;
    if (vec) {
        const int CR = (interleaved ? rd / 8 : rd / 16) + (hd - rd) / 8;
        const int g = grid_for(T_ * nh * CR);
#define SA_ROPE(TT, IL) hipLaunchKernelGGL((rope_v8_kernel<TT, IL>), g, 256, 0, st, (const TT*)x, (TT*)out, a)
        if (dtype == DT_BF16) { if (interleaved) SA_ROPE(u16, true); else SA_ROPE(u16, false); }
        else if (dtype == DT_F16) { if (interleaved) SA_ROPE(f16, true); else SA_ROPE(f16, false); }
        else { if (interleaved) SA_ROPE(float, true); else SA_ROPE(float, false); }
#undef SA_ROPE
        return;
    }
    const int pairs = rd / 2 + (hd - rd + 1) / 2;
    const int g = grid_for(T_ * nh * pairs);
#define SA_ROPE(TT, IL) hipLaunchKernelGGL((rope_kernel<TT, IL>), g, 256, 0, st, (const TT*)x, (TT*)out, a)
    if (dtype == DT_BF16) { if (interleaved) SA_ROPE(u16, true); else SA_ROPE(u16, false); }
    else if (dtype == DT_F16) { if (interleaved) SA_ROPE(f16, true); else SA_ROPE(f16, false); }
    else { if (interleaved) SA_ROPE(float, true); else SA_ROPE(float, false); }
#undef SA_ROPE
}
}  // namespace sa_launch
