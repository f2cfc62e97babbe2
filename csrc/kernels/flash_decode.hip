// Flash-decoding for short query segments (token-by-token generation, speculative / chunked steps) on gfx950.
// The prefill kernels tile 256 query rows per workgroup and walk all keys serially: for one query per segment
// that is 1/256 useful rows and one workgroup per q head.  Here:
//  * GQA packing: the Lq queries of all Hq/Hkv q heads sharing a KV head form the 32 MFMA rows of ONE wave
//    (packed row r -> head r / Lq, query r % Lq), so each K/V row is read once per KV head, not per q head;
//  * split-K: the key range is cut into splits across workgroups (grid split x kv head x segment) so a
//    single decode step fills the chip; each split writes an unnormalised (O, max, sum) partial in fp32 and
//    fa_decode_combine merges them (and writes lse, so the result is interchangeable with the prefill path).
//    (Merging in the last-arriving split instead -- arrival counter, agent-scope acquire/release -- measured
//    45 vs 9.8 + 6.6 us on the 7B decode step: the release writes back L2 in every split);
//  * per split, 32-key tiles: S^T = K Q^T with K fragments loaded straight from global memory (16 B per lane,
//    contiguous rows), online softmax in base 2 with lane-local row statistics (+1 lane^32 exchange), and
//    O^T += V^T P^T with V^T read transposed (ds_read_b64_tr_b16) from a swizzled LDS image of the V tile.
// Causal masking is bottom-right aligned (key <= q + Lk - Lq), sliding windows per head (local_heads) as in
// the prefill kernels.  Rows / keys past their ranges contribute nothing.
// A segment's keys are rows [cu_k[seg], cu_k[seg + 1]) or, with DecArgs::k_range, rows [start, start + length) of a
// buffer that holds one fixed-capacity slab per sequence (batched decoding over a static cache).
//
// FP8 K/V (template flag Q8, bf16 queries; DecArgs::k_scale): K and V are OCP e4m3fn codes with one fp32 power-of-two
// scale per (kv head, row) -- an exact encoding of a bf16 cache (ops/quant.py).  Same tiles, split plan, dim-to-MFMA
// mapping, masking and partials as the bf16 form; per tile a lane loads
//  * 8 K codes per MFMA step (8 bytes where the bf16 form loads 16), decoded to bf16 in registers (e4m3x4_to_bf16) for
//    the same MFMA; the key's scale multiplies its fp32 score before the softmax scale, x = (s ks[key]) c2 -- a power of
//    two on an fp32 accumulator is exact, so x is the bf16 kernel's score on the dequantised cache;
//  * 16 V codes per pass, decoded, multiplied by the row's scale (a bf16 number, exactly) and written into the same
//    swizzled LDS image, so the transposed reads and the P V MFMAs are untouched.  (Folding the V scale into P instead
//    would be equal only short of underflow of P; the image form has no such condition and was kept.)
// o and lse are bit for bit those of the bf16 kernel on the dequantised cache.  Rows past k_end load neither codes nor
// scales.
//
// Paged K/V (template flag PG; DecArgs::block_table): k / v are a pool of pages of `page` rows, page % 32 == 0, and
// logical key j of segment s is pool row block_table[s][j / page] * page + j % page (k_range gives (0, length)).  Splits
// start at multiples of 32, so every 32-key tile lies in one page and needs ONE wave-uniform table entry, which replaces
// the tile's base row; everything else -- tiles, split plan, masking, partials, the FP8 loads -- is the slab form, so o
// and lse are bit for bit those of the k_range call on a contiguous buffer holding the same rows.  The entry of a tile is
// fetched one tile before the tile's loads are issued (two tiles earlier than that in the FP8 form, which loads two
// tiles ahead), never for a tile at or past k_end, and an entry outside [0, num_pages) is not dereferenced: its keys are
// masked.  The slab instantiations (PG = false) contain none of this.
#include <algorithm>
#include <type_traits>

#include "flash_attn.h"
#include "launch.h"

using namespace sa;
using namespace sa::fa;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));  // four floats at a dword-aligned address

// out[token][hq][d] = sum_s 2^(m_s - M) O_s[d] / sum_s 2^(m_s - M) l_s ; lse = (M + log2 L) ln 2 (written for d == 0)
template <int D, bool F16>
__device__ __forceinline__ void merge_dim(const DecArgs& a, int64_t tok, int hq, int d) {
    float M = -INFINITY, L = 0.f, O = 0.f;
    constexpr int R = 16;  // up to R splits: every partial load issued before the first use (one round trip)
    if (a.nsplit <= R) {
        float ms[R], ls[R], os[R];
#pragma unroll
        for (int s = 0; s < R; ++s) {
            const int64_t row = (s * a.Tq + tok) * a.Hq + hq;
            const bool on = s < a.nsplit;
            ms[s] = on ? a.part_ml[2 * row] : -INFINITY;
            ls[s] = on ? a.part_ml[2 * row + 1] : 0.f;
            os[s] = on ? a.part_o[row * D + d] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < R; ++s) M = fmaxf(M, ms[s]);
        if (M != -INFINITY) {
#pragma unroll
            for (int s = 0; s < R; ++s) {
                const float w = ms[s] == -INFINITY ? 0.f : fast_exp2(ms[s] - M);
                L += w * ls[s];
                O += w * os[s];
            }
        }
    } else {
        for (int s = 0; s < a.nsplit; ++s) M = fmaxf(M, a.part_ml[2 * ((s * a.Tq + tok) * a.Hq + hq)]);
        if (M != -INFINITY) {
            for (int s = 0; s < a.nsplit; ++s) {
                const int64_t row = (s * a.Tq + tok) * a.Hq + hq;
                const float ms = a.part_ml[2 * row];
                if (ms == -INFINITY) continue;
                const float w = fast_exp2(ms - M);
                L += w * a.part_ml[2 * row + 1];
                O += w * a.part_o[row * D + d];
            }
        }
    }
    const float out = L > 0.f ? O / L : 0.f;
    a.o[tok * a.o_tok + (int64_t)hq * a.o_head + d] = f2t<F16>(out);
    if (d == 0) a.lse[(int64_t)hq * a.lse_stride + tok] = L > 0.f ? (M + __log2f(L)) * 0.69314718055994530942f : INFINITY;
}

template <int D, bool F16, bool Q8, bool PG>
__global__ __launch_bounds__(64) void fa_decode_kernel(DecArgs a) {
    static_assert(!(F16 && Q8), "FP8 K/V: bf16 queries only");
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ __attribute__((aligned(16))) char vimg[32 * D * 2];
    constexpr int NKS = D / 16, NT = D / 32;
    const int split = blockIdx.x, hk = blockIdx.y, seg = blockIdx.z;
    const int q0s = a.cu_q[seg];
    const int Lq = a.cu_q[seg + 1] - q0s;
    int k0s, Lk;
    if constexpr (PG) {  // (0, length): the keys are the table's pages in order, clipped to the table's width
        k0s = 0;
        Lk = a.k_range[2 * seg + 1];
        Lk = (int)min((int64_t)max(Lk, 0), (int64_t)a.max_pages * a.page);
    } else if (a.k_range) {  // (first row, count) of this segment's keys, clipped to the buffer
        k0s = a.k_range[2 * seg];
        Lk = a.k_range[2 * seg + 1];
        if (k0s < 0 || Lk < 0 || k0s > a.k_rows) k0s = 0, Lk = 0;
        Lk = (int)min((int64_t)Lk, a.k_rows - k0s);
    } else {
        k0s = a.cu_k[seg];
        Lk = a.cu_k[seg + 1] - k0s;
    }
    const int grp = a.Hq / a.Hkv;
    const int lane = threadIdx.x, h = lane >> 5, r = lane & 31;
    const int off = Lk - Lq;
    const int g = Lq > 0 ? r / Lq : 0, qi = Lq > 0 ? r % Lq : 0;
    const bool valid = Lq > 0 && r < Lq * grp;
    const int hq = hk * grp + min(g, grp - 1);
    const int win = hq < a.local_heads ? a.window : -1;
    const int k_begin = split * a.split_keys;
    int k_end = min(Lk, k_begin + a.split_keys);
    if (a.causal) k_end = min(k_end, Lq + off);  // beyond the last query's causal bound nothing is visible
    const float c2 = a.scale_log2;

    bf16x8 qf[NKS];
    {
        const u16* qp = a.q + (int64_t)(q0s + (valid ? qi : 0)) * a.q_tok + (int64_t)hq * a.q_head;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const u16x8 v = valid ? *reinterpret_cast<const u16x8*>(qp + 16 * ks + 8 * h) : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            qf[ks] = __builtin_bit_cast(bf16x8, v);
        }
    }
    f32x16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = f32x16{};
    float m = -INFINITY, l = 0.f;
    const u16* kb = a.k + (int64_t)k0s * a.k_tok + (int64_t)hk * a.k_head;
    const u16* vb = a.v + (int64_t)k0s * a.v_tok + (int64_t)hk * a.v_head;
    // FP8 K/V: codes, one byte per element (strides in bytes), and the per-row scales of this kv head
    const uint8_t* kb8 = reinterpret_cast<const uint8_t*>(a.k) + (int64_t)k0s * a.k_tok + (int64_t)hk * a.k_head;
    const uint8_t* vb8 = reinterpret_cast<const uint8_t*>(a.v) + (int64_t)k0s * a.v_tok + (int64_t)hk * a.v_head;
    const float* ksb = Q8 ? a.k_scale + (int64_t)hk * a.s_head + k0s : nullptr;
    const float* vsb = Q8 ? a.v_scale + (int64_t)hk * a.s_head + k0s : nullptr;

    // paged: the pool row of a tile's first key (the tile's base row), -1 for a table entry outside the pool; tiles are
    // asked for in order from k_begin, one call per tile.  slab: the base row of tile kt is kt itself (row_t stays int)
    using row_t = std::conditional_t<PG, int64_t, int>;
    const int* bt = PG ? a.block_table + (int64_t)seg * a.bt_stride : nullptr;
    int c_kt = k_begin, c_pg = PG ? k_begin / a.page : 0, c_in = PG ? k_begin % a.page : 0;
    auto next_base = [&]() -> int64_t {
        int64_t base = -1;
        if (c_kt < k_end) {  // k_end <= max_pages * page: c_pg is inside the table
            const int e = bt[c_pg];
            if ((unsigned)e < (unsigned)a.num_pages) base = (int64_t)e * a.page + c_in;
        }
        c_kt += 32;
        c_in += 32;
        if (c_in >= a.page) c_in = 0, ++c_pg;
        return base;
    };

    // FP8: the codes and scales of a tile are loaded two tiles ahead (n1, n2).  A tile of codes is half the bytes of a
    // bf16 tile and a workgroup is one wave, so two tiles in flight are the bf16 form's bytes in flight, and their round
    // trip overlaps the decode -> MFMA -> softmax -> MFMA chain of the tile being computed.  The loads are unconditional
    // instructions (every lane guards its own rows against k_end), so the waits stay counted, not drained.
    // QP 16-byte V loads per lane: 16 codes = two 8-element chunks of the image
    constexpr int QP = 32 * D / 16 / 64;
    struct Q8Tile {
        u32x2 kq[NKS];  // K codes: key kt + r, dims 16 ks + 8 h ..
        f32x4 ksc[4];   // K scales of the keys of this lane's 16 score registers: group g = keys kt + 8 g + 4 h + 0..3
        u32x4 vq[QP];
        float vs[QP];
    };
    auto load_q8 = [&](int kt, int64_t tb, Q8Tile& t) {  // rows past k_end load neither codes nor scales
        const bool tile_on = !PG || tb >= 0;
        const row_t ab = PG ? (row_t)tb : (row_t)kt;  // address of key kt + i: row ab + i
        const bool krow = kt + r < k_end && tile_on;
        const uint8_t* kp = kb8 + (int64_t)(krow ? ab + r : (PG ? 0 : kt)) * a.k_tok;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            t.kq[ks] = krow ? *reinterpret_cast<const u32x2*>(kp + 16 * ks + 8 * h) : u32x2{0, 0};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int kg = kt + 8 * g + 4 * h;
            const row_t ag = ab + 8 * g + 4 * h;
            if (kg + 3 < k_end && tile_on) {  // one 16-byte load; a slab may start at any row, so only dword alignment is assumed
                t.ksc[g] = *reinterpret_cast<const f32x4_a4*>(ksb + ag);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) t.ksc[g][i] = kg + i < k_end && tile_on ? ksb[ag + i] : 0.f;
            }
        }
#pragma unroll
        for (int p = 0; p < QP; ++p) {
            const int id = lane + 64 * p, row = id / (D / 16), c = id % (D / 16);
            const bool on = kt + row < k_end && tile_on;
            t.vq[p] = on ? *reinterpret_cast<const u32x4*>(vb8 + (int64_t)(ab + row) * a.v_tok + c * 16) : u32x4{0, 0, 0, 0};
            t.vs[p] = on ? vsb[ab + row] : 0.f;
        }
    };
    Q8Tile n1, n2;
    // tb_cur: base row of the tile being computed; tb_nxt: of the next tile whose loads are issued (bf16: kt + 32, FP8:
    // kt + 64), fetched an iteration before it is needed so that no load of a tile waits for its table entry
    int64_t tb_cur = -1, tb_nxt = -1;
    bool on_n1 = true, on_n2 = true;  // FP8 paged: whether the tiles in n1 / n2 have a table entry inside the pool
    if constexpr (Q8) {
        const int64_t b0 = PG ? next_base() : 0, b1 = PG ? next_base() : 0;
        if constexpr (PG) tb_nxt = next_base(), on_n1 = b0 >= 0, on_n2 = b1 >= 0;
        load_q8(k_begin, b0, n1);
        load_q8(k_begin + 32, b1, n2);
    } else if constexpr (PG) {
        tb_cur = next_base();
        tb_nxt = next_base();
    }

    for (int kt = k_begin; kt < k_end; kt += 32) {
        // K rows (A operand: key kt + r, dims 16 ks + 8 h) and the V tile are all issued before anything waits on
        // them: one memory round trip per tile instead of V, then K
        bool tile_on = true;  // paged: whether this tile's table entry lies inside the pool
        if constexpr (PG && !Q8) tile_on = tb_cur >= 0;
        const row_t ab = PG ? (row_t)tb_cur : (row_t)kt;  // bf16 form: address of key kt + i is row ab + i
        const bool krow = kt + r < k_end && tile_on;
        u16x8 kv[NKS];
        // PASSES 16-byte loads per lane of 8 bf16 each
        constexpr int PASSES = Q8 ? 1 : 32 * D / 8 / 64;
        u16x8 vv[PASSES];
        Q8Tile cur;
        if constexpr (Q8) {
            cur = n1;
            n1 = n2;
            load_q8(kt + 64, tb_nxt, n2);
            if constexpr (PG) {
                tile_on = on_n1, on_n1 = on_n2, on_n2 = tb_nxt >= 0;
                tb_nxt = next_base();  // tile kt + 96: loaded by the next iteration
            }
            // codes -> bf16 in registers (exact); the key's scale multiplies its fp32 score below
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                u32x4 w;
                uint32_t w0, w1;
                e4m3x4_to_bf16(cur.kq[ks][0], w0, w1);
                w[0] = w0;
                w[1] = w1;
                e4m3x4_to_bf16(cur.kq[ks][1], w0, w1);
                w[2] = w0;
                w[3] = w1;
                kv[ks] = __builtin_bit_cast(u16x8, w);
            }
        } else {
            const u16* kp = kb + (int64_t)(krow ? ab + r : (PG ? 0 : kt)) * a.k_tok;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                kv[ks] = krow ? *reinterpret_cast<const u16x8*>(kp + 16 * ks + 8 * h) : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            // V tile [32][D] -> swizzled LDS image (rows past k_end as zeros)
#pragma unroll
            for (int p = 0; p < PASSES; ++p) {
                const int id = lane + 64 * p, row = id / (D / 8), c = id % (D / 8);
                vv[p] = kt + row < k_end && tile_on
                            ? *reinterpret_cast<const u16x8*>(vb + (int64_t)(ab + row) * a.v_tok + c * 8)
                            : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
            if constexpr (PG) {  // the next tile's entry is in hand; fetch the one after it
                tb_cur = tb_nxt;
                tb_nxt = next_base();
            }
        }
        // S^T = K Q^T
        f32x16 s = f32x16{};
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) s = mma<F16>(__builtin_bit_cast(bf16x8, kv[ks]), qf[ks], s);
        if constexpr (Q8) {
            // V codes times the row's scale are bf16 numbers (exact: the product has 4 significant bits and the scale
            // exponent is bounded below), written into the image the bf16 kernel would have loaded
#pragma unroll
            for (int p = 0; p < QP; ++p) {
                const int id = lane + 64 * p, row = id / (D / 16), c = id % (D / 16);
                const float vsp = cur.vs[p];
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    u32x4 w;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)cur.vq[p][2 * q + i], false);
                        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)cur.vq[p][2 * q + i], true);
                        w[2 * i] = (__float_as_uint(lo[0] * vsp) >> 16) | (__float_as_uint(lo[1] * vsp) & 0xffff0000u);
                        w[2 * i + 1] = (__float_as_uint(hi[0] * vsp) >> 16) | (__float_as_uint(hi[1] * vsp) & 0xffff0000u);
                    }
                    *reinterpret_cast<u32x4*>(vimg + row * D * 2 + 16 * swz<D>(row, 2 * c + q)) = w;
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < PASSES; ++p) {
                const int id = lane + 64 * p, row = id / (D / 8), c = id % (D / 8);
                *reinterpret_cast<u16x8*>(vimg + row * D * 2 + 16 * swz<D>(row, c)) = vv[p];
            }
        }
        // scale + mask; key of register j: kt + crow(j) + 4h
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int key = kt + crow(j) + 4 * h;
            bool ok = valid && key < k_end;
            if constexpr (PG) ok = ok && tile_on;
            if (a.causal) ok = ok && key <= qi + off;
            if (win >= 0) ok = ok && key >= qi + off - win && (a.causal || key <= qi + off + win);
            float x;
            if constexpr (Q8) x = ok ? (s[j] * cur.ksc[j >> 2][j & 3]) * c2 : -INFINITY;  // power-of-two scale: exact, before c2
            else x = ok ? s[j] * c2 : -INFINITY;
            s[j] = x;
            mx = fmaxf(mx, x);
        }
        mx = max_xchg32(mx);
        const float mnew = fmaxf(m, mx);
        const float msafe = mnew == -INFINITY ? 0.f : mnew;
        const float alpha = fast_exp2(m - msafe);
        float rs = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float p = fast_exp2(s[j] - msafe);
            s[j] = p;
            rs += p;
        }
        l = l * alpha + sum_xchg32(rs);
        m = mnew;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) o[t][j] *= alpha;
        __syncthreads();  // V image complete
        const bf16x8 p0 = pack_acc_t<F16>(s, 0), p1 = pack_acc_t<F16>(s, 1);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            o[t] = mma<F16>(ld_tr<D>(vimg, 0, 32 * t), p0, o[t]);
            o[t] = mma<F16>(ld_tr<D>(vimg, 16, 32 * t), p1, o[t]);
        }
        __syncthreads();  // before the next tile overwrites the image
    }
    if (valid) {
        const int64_t row = ((int64_t)split * a.Tq + q0s + qi) * a.Hq + hq;
        float* po = a.part_o + row * D;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int j = 0; j < 16; ++j) po[32 * t + crow(j) + 4 * h] = o[t][j];
        if (h == 0) {
            a.part_ml[2 * row] = m;
            a.part_ml[2 * row + 1] = l;
        }
    }
#endif
}

template <int D, bool F16>
__global__ __launch_bounds__(D) void fa_decode_combine_kernel(DecArgs a) {
    merge_dim<D, F16>(a, blockIdx.x, blockIdx.y, threadIdx.x);
}

template <int D, bool F16>
void launch(const DecArgs& a, int nseg, hipStream_t st) {
    const dim3 grid(a.nsplit, a.Hkv, nseg);
    bool q8 = false;
    const bool pg = a.block_table != nullptr;
    if constexpr (!F16) {
        q8 = a.k_scale != nullptr;
        if (q8 && pg) hipLaunchKernelGGL((fa_decode_kernel<D, false, true, true>), grid, dim3(64), 0, st, a);
        else if (q8) hipLaunchKernelGGL((fa_decode_kernel<D, false, true, false>), grid, dim3(64), 0, st, a);
    }
    if (!q8 && pg) hipLaunchKernelGGL((fa_decode_kernel<D, F16, false, true>), grid, dim3(64), 0, st, a);
    else if (!q8) hipLaunchKernelGGL((fa_decode_kernel<D, F16, false, false>), grid, dim3(64), 0, st, a);
    hipLaunchKernelGGL((fa_decode_combine_kernel<D, F16>), dim3((unsigned)a.Tq, a.Hq), dim3(D), 0, st, a);
}

}  // namespace

namespace sa_launch {
// splits so that split x kv head x segment workgroups fill the chip; split length a multiple of the 32-key tile
void fa_decode_plan(int64_t max_k, int Hkv, int nseg, int& split_keys, int& nsplit) {
    const int64_t want = std::max<int64_t>(1, (1024 + (int64_t)Hkv * nseg - 1) / ((int64_t)Hkv * nseg));
    const int64_t tiles = std::max<int64_t>(1, (max_k + 31) / 32);
    // one 32-key tile per split while that still leaves <= `want` splits: a decode step is a latency chain of
    // (load K/V tile -> MFMA -> softmax -> MFMA) per tile, so short contexts want the tiles side by side
    const int64_t per = std::max<int64_t>(1, (tiles + want - 1) / want);
    split_keys = (int)(per * 32);
    nsplit = (int)std::max<int64_t>(1, (max_k + split_keys - 1) / split_keys);
}
void fa_decode(const DecArgs& a, int D, bool f16, hipStream_t st) {
    const int nseg = a.nseg;
    if (f16) {
        if (D == 128) launch<128, true>(a, nseg, st);
        else if (D == 64) launch<64, true>(a, nseg, st);
        else launch<32, true>(a, nseg, st);
    } else {
        if (D == 128) launch<128, false>(a, nseg, st);
        else if (D == 64) launch<64, false>(a, nseg, st);
        else launch<32, false>(a, nseg, st);
    }
}
}  // namespace sa_launch
