// Chunk attention for gfx950: a chunk of queries of any length over keys held in a KV cache (slab ranges or a paged
// pool; bf16, fp16 or FP8 codes), forward only.  The prefill kernel (flash_fwd.hip) wants packed cu_k keys and runs one
// workgroup per q head; the decode kernel (flash_decode.hip) packs at most 32 rows per segment into one wave.  This one
// serves what lies between: chunked prefill into the cache, prefix reuse, multi-token verification steps.
//
// Work split.  A workgroup of 4 waves owns 128 PACKED rows of one (segment, kv head): packed row p is query p / group
// of q head hk * group + p % group (group = Hq / Hkv).  Query-major, so the causal bound is monotone in p and a wave's
// 32 rows share nearly one bound.  Every K/V tile is read once per kv head and shared by the 4 waves (group x fewer
// K/V bytes than one workgroup per q head).  Grid: attn_grid(kv head x split, segment, row tile) -- heaviest causal
// row tiles first.
//
// Key tiles of 64 keys = two 32-key halves.  page % 32 == 0, so a half lies in one page and takes one wave-uniform
// table entry.  The entries of the workgroup's key span are fetched with vector loads BEFORE the loop (lane l of every
// wave keeps halves l, l + 64, ... in registers) and picked per tile with v_readlane: no table load, scalar or vector,
// sits between a tile and its K/V loads.  The registers hold 256 halves, so a paged span is at most 8192 keys per
// workgroup; fa_chunk_plan splits longer paged contexts (a deviation from "split only to fill the chip", recorded
// here).  An entry outside [0, num_pages) masks its 32 keys and is never dereferenced; keys at or past the
// workgroup's span end (<= Lk) are never loaded.
//
// LDS: K and V, double buffered, in the swizzled image of flash_attn.h, so K is read by ds_read_b128 row reads, V^T by
// ds_read_b64_tr_b16, and the softmax stays lane-local (S^T = K Q^T, the accumulator packed as the B operand of
// O^T += V^T P^T), as in fa_fwd_v2_kernel.  Tiles are staged through registers in every form: the next tile's global
// loads are issued before the current tile's MFMA phase and written to the other buffer after it (one barrier per
// tile).  Register staging rather than LDS-DMA because the paged form needs two base rows per tile and the FP8 form
// decodes on the way; one staging path serves all forms.
//
// FP8 (Q8): e4m3 codes at half the bytes plus one fp32 power-of-two scale per (kv head, row), decoded at staging:
// code * scale is exactly a bf16 number, so the LDS image holds the dequantised K and V and the MFMA phases are the bf16
// ones -- o and lse equal this kernel's bf16 form on the dequantised pool bit for bit.  Rows that are not loaded load
// neither codes nor scales.
//
// Masking: tiles wholly above the workgroup's causal bound or wholly below every row's window are not visited; a wave
// skips a tile wholly above its own bound; the mask arithmetic runs on boundary tiles only, behind a wave-uniform
// branch (mask_fence).  Lazy rescale (threshold 2^8) as in fa_fwd_v2_kernel.
//
// Measured (7B head shape, page 64, profiles/chunk_attn_bench.log): against fa_fwd over contiguous keys plus the copy
// into the pages, x0.21-0.39 of the time for a 128-token chunk over 2048 / 8192 cached keys, x0.62-0.82 for 512 tokens,
// level at 2048 tokens over <= 2048 keys (440-720 TF against fa_fwd's ~1 PF: register staging against LDS-DMA), x1.4
// slower for a 512-token prompt with no context, and x1.9 slower at 2048 tokens over 8192 keys, where the 8192-key
// table limit forces two splits on a grid that already fills the chip (eight table registers would lift it; not done).
//
// Split-K (nsplit > 1): the key span is cut at multiples of 64 keys; a workgroup writes its unnormalised (O, m, l) in
// fa_decode_kernel's partial layout and fa_decode_combine merges them.  With one split o and lse are written directly.
//
// Key bias (KB; dense bf16 / fp16 slab keys only): score = scale * q.k + key_bias[buffer row of the key], one fp32 value
// per key (attention-score manipulation: log of a suppression factor, -10000 or -inf for factor 0).  In S^T = K Q^T the
// key is the accumulator's ROW, so a lane needs 32 biases per tile (rows 32b + 8g + 4h + 0..3), each wanted by the 32
// lanes of its half.  The bias is NOT added by VALU: the QK accumulators are SEEDED with key_bias / scale (= key_bias *
// kb_mul, multiplied once where the value is loaded) instead of zero, the MFMAs add the raw q.k on top, and the softmax
// that follows is the unbiased kernel's instruction for instruction -- (bias / scale + q.k) * scale_log2 is the biased
// score in base 2, rounded at the magnitude fp32 math rounds bias + scale * q.k at.  So the running max sees the bias,
// lse includes it (the split-K partials and the combine stay valid unchanged), a masked key stays masked (the mask
// overwrites the accumulator), an all-zero bias gives the unbiased kernel's bits, and -inf needs no care: the seed
// stays -inf through the MFMAs (K and Q are finite), and an all -inf row of a tile takes the guards an all-masked row
// takes already (no rescale from m = -inf, exp2(-inf) = 0): no inf - inf, no NaN in m, l or O.
// Transport: thread t < 64 fetches the bias of key kt + t with the K/V register staging of that tile (one VGPR, in
// flight across the MFMA phase; keys at or past the span end load nothing and read 0) and writes it beside the tile's
// K/V image (256 B per buffer) at the staging store, so it rides the existing barrier; a lane then reads its 32 seeds
// as 8 ds_read_b128 (two addresses per instruction, broadcast: conflict-free) straight into the accumulator registers.
// Through LDS rather than registers alone because a lane's 32 values for tile t + 1, held across tile t's MFMA phase on
// top of tile t's, are 64 VGPRs the D = 128 form does not have below its 256-register cap.
#include <algorithm>

#include "flash_attn.h"
#include "launch.h"

using namespace sa;
using namespace sa::fa;

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kTabRegs = 4;                       // block-table registers per lane
constexpr int kMaxPagedSpan = 64 * kTabRegs * 32;  // keys of one workgroup's paged span

// 8 e4m3 codes times their row's power-of-two scale -> 8 bf16 (exact)
__device__ __forceinline__ u32x4 dequant8(u32x2 c, float sc) {
    u32x4 w;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[i], true);
        w[2 * i] = (__float_as_uint(lo[0] * sc) >> 16) | (__float_as_uint(lo[1] * sc) & 0xffff0000u);
        w[2 * i + 1] = (__float_as_uint(hi[0] * sc) >> 16) | (__float_as_uint(hi[1] * sc) & 0xffff0000u);
    }
    return w;
}

template <int D, bool F16, bool Q8, bool PG, bool KB = false>
__global__ __launch_bounds__(256, 2) void fa_chunk_kernel(DecArgs a) {
    static_assert(!(F16 && Q8), "FP8 K/V: bf16 queries only");
    static_assert(!(KB && (Q8 || PG)), "key bias: dense slab keys only");
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int KT = 64, TILE = KT * D * 2, NKS = D / 16, NT = D / 32;
    constexpr int CPR = D / 8, RPP = 256 / CPR, NPT = KT / RPP;  // 8-element chunks per row, rows per pass, passes
    constexpr float TH = 8.f;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int seg = attn_seg();
    const int hk = (int)blockIdx.x % a.Hkv, split = (int)blockIdx.x / a.Hkv;
    const int q0s = a.cu_q[seg];
    const int Lq = a.cu_q[seg + 1] - q0s;
    int k0s, Lk;
    if constexpr (PG) {  // (0, length): the keys are the table's pages in order, clipped to the table's width
        k0s = 0;
        Lk = a.k_range[2 * seg + 1];
        Lk = (int)min((int64_t)max(Lk, 0), (int64_t)a.max_pages * a.page);
    } else {  // (first row, count) of this segment's keys, clipped to the buffer
        k0s = a.k_range[2 * seg];
        Lk = a.k_range[2 * seg + 1];
        if (k0s < 0 || Lk < 0 || k0s > a.k_rows) k0s = 0, Lk = 0;
        Lk = (int)min((int64_t)Lk, a.k_rows - k0s);
    }
    const int grp = a.Hq / a.Hkv;
    const int P = Lq * grp;  // packed rows of this (segment, kv head)
    const int pwg0 = attn_qtile(a.causal) * 128;
    if (pwg0 >= P) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 5,
              lq = lane & 31;
    const int pw0 = pwg0 + 32 * wave, myp = pw0 + lq;
    const bool valid = myp < P;
    const int pc = min(myp, P - 1);
    const int qi = pc / grp, hq = hk * grp + pc % grp;
    const int W = min(a.window, 1 << 30);
    const int win = (W >= 0 && hq < a.local_heads) ? W : -1;  // per-head window (mixed local/global heads)
    const int off = Lk - Lq;                                  // bottom-right causal alignment
    // wave-uniform query bounds of the workgroup and of this wave, and whether the kv group has windowed heads
    const int qlo_wg = pwg0 / grp, qhi_wg = min(pwg0 + 127, P - 1) / grp;
    const int qlo_w = min(pw0, P - 1) / grp, qhi_w = min(pw0 + 31, P - 1) / grp;
    const bool any_local = W >= 0 && hk * grp < a.local_heads, all_local = W >= 0 && (hk + 1) * grp <= a.local_heads;

    // key span of the workgroup: [klo, khi), klo a multiple of 64; every key >= khi is masked for all of its rows
    int khi = Lk;
    if (a.causal) khi = min(Lk, qhi_wg + off + 1);
    else if (all_local) khi = min(Lk, qhi_wg + off + W + 1);
    int klo = all_local ? max(0, qlo_wg + off - W) : 0;
    klo &= ~(KT - 1);
    if (a.nsplit > 1) {
        klo = max(klo, split * a.split_keys);
        khi = min(khi, (split + 1) * a.split_keys);
    }
    if constexpr (PG) khi = min(khi, klo + kMaxPagedSpan);  // the host plan never needs this clip
    const int ntiles = khi > klo ? (khi - klo + KT - 1) / KT : 0;

    // paged: base pool row of every 32-key half of the span (-1: entry outside the pool), lane l holds halves l + 64 j
    int tabv[kTabRegs];
    if constexpr (PG) {
        const int* bt = a.block_table + (int64_t)seg * a.bt_stride;
        const int nh = ntiles > 0 ? (khi - klo + 31) / 32 : 0;
#pragma unroll
        for (int j = 0; j < kTabRegs; ++j) {
            const int idx = lane + 64 * j, key = klo + 32 * idx;
            int e = -1;
            if (idx < nh) e = bt[key / a.page];  // key < khi <= max_pages * page: inside the table
            tabv[j] = (unsigned)e < (unsigned)a.num_pages ? e * a.page + key % a.page : -1;
        }
    }
    // base row (of the key buffer) of the 32-key half starting at key kt + 32 b
    auto half_base = [&](int kt, int b) -> int {
        if constexpr (PG) {
            const int hidx = __builtin_amdgcn_readfirstlane(((kt - klo) >> 5) + b);
            int r = -1;
#pragma unroll
            for (int j = 0; j < kTabRegs; ++j) {
                const int v = __builtin_amdgcn_readlane(tabv[j], hidx & 63);
                r = (hidx >> 6) == j ? v : r;
            }
            return r;
        } else {
            return k0s + kt + 32 * b;
        }
    };

    // ---- staging: thread owns chunk c of rows r0 + RPP i
    const int r0 = tid / CPR, c = tid % CPR;
    const u16* kb = a.k + (int64_t)hk * a.k_head + c * 8;
    const u16* vb = a.v + (int64_t)hk * a.v_head + c * 8;
    const uint8_t* kb8 = reinterpret_cast<const uint8_t*>(a.k) + (int64_t)hk * a.k_head + c * 8;  // strides in bytes
    const uint8_t* vb8 = reinterpret_cast<const uint8_t*>(a.v) + (int64_t)hk * a.v_head + c * 8;
    const float* ksb = Q8 ? a.k_scale + (int64_t)hk * a.s_head : nullptr;
    const float* vsb = Q8 ? a.v_scale + (int64_t)hk * a.s_head : nullptr;
    u16x8 rk[Q8 ? 1 : NPT], rv[Q8 ? 1 : NPT];
    u32x2 ck[Q8 ? NPT : 1], cv[Q8 ? NPT : 1];
    float sk[Q8 ? NPT : 1], sv[Q8 ? NPT : 1];
    float rb = 0.f;  // KB: accumulator seed of key kt + tid (threads 0..63)
    auto load = [&](int kt) {
        if constexpr (KB) {  // k0s + kt + tid < k0s + khi <= k_rows = the bias's length
            if (tid < KT) rb = kt + tid < khi ? a.key_bias[(int64_t)k0s + kt + tid] * a.kb_mul : 0.f;
        }
        const int b0 = half_base(kt, 0), b1 = half_base(kt, 1);
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int row = r0 + RPP * i;
            const int base = row < 32 ? b0 : b1;
            const bool on = kt + row < khi && base >= 0;
            const int64_t g = on ? base + (row & 31) : 0;
            if constexpr (Q8) {
                ck[i] = on ? *reinterpret_cast<const u32x2*>(kb8 + g * a.k_tok) : u32x2{0, 0};
                cv[i] = on ? *reinterpret_cast<const u32x2*>(vb8 + g * a.v_tok) : u32x2{0, 0};
                sk[i] = on ? ksb[g] : 0.f;
                sv[i] = on ? vsb[g] : 0.f;
            } else {
                rk[i] = on ? *reinterpret_cast<const u16x8*>(kb + g * a.k_tok) : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
                rv[i] = on ? *reinterpret_cast<const u16x8*>(vb + g * a.v_tok) : u16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        }
    };
    // KB: the 64 seeds of the tile in buffer `buf` (0 or 1), behind the four K/V images
    auto seeds = [&](const char* buf) -> char* { return smem + 4 * TILE + (buf == smem ? 0 : 4 * KT); };
    auto store = [&](char* buf) {
        if constexpr (KB) {
            if (tid < KT) *reinterpret_cast<float*>(seeds(buf) + 4 * tid) = rb;
        }
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int row = r0 + RPP * i;
            const int o = row * D * 2 + 16 * swz<D>(row, c);
            if constexpr (Q8) {
                *reinterpret_cast<u32x4*>(buf + o) = dequant8(ck[i], sk[i]);
                *reinterpret_cast<u32x4*>(buf + TILE + o) = dequant8(cv[i], sv[i]);
            } else {
                *reinterpret_cast<u16x8*>(buf + o) = rk[i];
                *reinterpret_cast<u16x8*>(buf + TILE + o) = rv[i];
            }
        }
    };

    LdsOffsets<D> L;
    L.init(lane);
    bf16x8 qf[NKS];
    {
        const u16* qp = a.q + (int64_t)(q0s + qi) * a.q_tok + (int64_t)hq * a.q_head;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
            qf[ks] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u16x8*>(qp + 16 * ks + 8 * h));
    }
    f32x16 o[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) o[t] = f32x16{};
    float m = -INFINITY, l = 0.f;
    const float c2 = a.scale_log2;

    auto tile = [&](const char* K, int kt) {
        // wave-uniform skips: a wave of padding rows, a tile wholly above this wave's causal bound
        if (pw0 >= P || (a.causal && kt > qhi_w + off)) return;
        const char* V = K + TILE;
        f32x16 s[2] = {f32x16{}, f32x16{}};
        if constexpr (KB) {  // registers 4g .. 4g + 3 of block b are keys kt + 32b + 8g + 4h + 0..3
            const char* sd = seeds(K) + 16 * h;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 w = *reinterpret_cast<const f32x4*>(sd + 128 * b + 32 * g);
#pragma unroll
                    for (int j = 0; j < 4; ++j) s[b][4 * g + j] = w[j];
                }
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int b = 0; b < 2; ++b)
                s[b] = mma<F16>(*reinterpret_cast<const bf16x8*>(K + 32 * b * D * 2 + L.row(ks)), qf[ks], s[b]);
#pragma unroll
        for (int i = 0; i < 2 * NKS; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
        }
        int hb[2] = {0, 0};
        if constexpr (PG) hb[0] = half_base(kt, 0), hb[1] = half_base(kt, 1);
        // wave-uniform: does any element of this wave's 32 x 64 block need a mask?
        const bool need_mask = (kt + KT > khi) || (a.causal && kt + KT - 1 > qlo_w + off) ||
                               (any_local && (kt < qhi_w + off - W || (!a.causal && kt + KT - 1 > qlo_w + off + W))) ||
                               (PG && (hb[0] < 0 || hb[1] < 0));
        if (need_mask) {
            mask_fence();
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int base = kt + 32 * b + 4 * h;  // key of register j = base + crow(j)
                int hi = khi - 1 - base;
                if (a.causal) hi = min(hi, qi + off - base);
                else if (win >= 0) hi = min(hi, qi + off + win - base);
                const int lo = win >= 0 ? qi + off - win - base : -1;
                if (PG && hb[b] < 0) hi = -1;
#pragma unroll
                for (int j = 0; j < 16; ++j) s[b][j] = (crow(j) <= hi && crow(j) >= lo) ? s[b][j] : -INFINITY;
            }
        }
        const float m0 = vmax16(s[0]), m1 = vmax16(s[1]);
        const float mx = vmax3(m0, m1, m1);
        const float mrow = max_xchg32(mx) * c2;
        if (__builtin_amdgcn_ballot_w64(mrow > m + TH) != 0) {  // rare after the first tiles
            mask_fence();
            const float mnew = fmaxf(m, mrow);
            const float alpha = mnew == -INFINITY ? 1.f : fast_exp2(m - mnew);
            l *= alpha;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int j = 0; j < 16; ++j) o[t][j] *= alpha;
            m = mnew;
        }
        const float nm = m == -INFINITY ? 0.f : -m;
        float rs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float p = fast_exp2(__builtin_fmaf(s[b][j], c2, nm));
                s[b][j] = p;
                rs[j & 3] += p;
            }
        l += sum_xchg32((rs[0] + rs[1]) + (rs[2] + rs[3]));
        bf16x8 pf[2][2];
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) pf[b][ss] = pack_acc_t<F16>(s[b], ss);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int ss = 0; ss < 2; ++ss)
                    o[t] = mma<F16>(rd_tr<D>(V, (32 * b + 16 * ss) * D * 2, L, t), pf[b][ss], o[t]);
#pragma unroll
        for (int i = 0; i < 4 * NT; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);  // 2 x ds_read_b64_tr_b16
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);  // MFMA
        }
    };

    char* buf0 = smem;
    char* buf1 = smem + 2 * TILE;
    if (ntiles > 0) {
        load(klo);
        store(buf0);
    }
    __syncthreads();
    // pairs of tiles (buffer 0 then 1) so every LDS address is register + immediate; odd tail peeled.  A buffer is
    // rewritten only after the barrier that follows its last read.
    int kt = klo;
    for (int pr = 0; pr < ntiles / 2; ++pr, kt += 2 * KT) {
        load(kt + KT);
        tile(buf0, kt);
        store(buf1);
        __syncthreads();
        const bool more = kt + 2 * KT < khi;
        if (more) load(kt + 2 * KT);
        tile(buf1, kt + KT);
        if (more) store(buf0);
        __syncthreads();
    }
    if (ntiles & 1) tile(buf0, kt);

    if (!valid) return;
    if (a.nsplit > 1) {  // unnormalised partial in fa_decode_kernel's layout; m is any reference exponent
        const int64_t row = ((int64_t)split * a.Tq + q0s + qi) * a.Hq + hq;
        float* po = a.part_o + row * D;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 w;
#pragma unroll
                for (int j = 0; j < 4; ++j) w[j] = o[t][4 * g + j];
                *reinterpret_cast<f32x4*>(po + 32 * t + 8 * g + 4 * h) = w;
            }
        if (h == 0) {
            a.part_ml[2 * row] = m;
            a.part_ml[2 * row + 1] = l;
        }
        return;
    }
    const float inv = l > 0.f ? 1.f / l : 0.f;
    u16* op = a.o + (int64_t)(q0s + qi) * a.o_tok + (int64_t)hq * a.o_head;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            u16x4 w;
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = f2t<F16>(o[t][4 * g + j] * inv);
            *reinterpret_cast<u16x4*>(op + 32 * t + 8 * g + 4 * h) = w;
        }
    if (h == 0)
        a.lse[(int64_t)hq * a.lse_stride + q0s + qi] = l > 0.f ? (m + __log2f(l)) * 0.69314718055994530942f : INFINITY;
#endif
}

template <int D, bool F16>
void launch(const DecArgs& a, int max_q, hipStream_t st) {
    const int grp = a.Hq / a.Hkv;
    const int rtiles = (int)(((int64_t)max_q * grp + 127) / 128);
    const dim3 grid = attn_grid(a.Hkv * a.nsplit, a.nseg, rtiles), block(256);
    constexpr int smem = 4 * 64 * D * 2;
    const bool pg = a.block_table != nullptr;
    bool q8 = false;
    if (a.key_bias != nullptr) {  // the caller has refused pages and FP8 scales; 512 B more LDS for the seeds
        constexpr int smem_kb = smem + 2 * 64 * 4;
        if constexpr (smem_kb > 65536) {  // more than 64 KiB of dynamic LDS is asked for once per device (sample.hip)
            static bool asked[64] = {};
            int dev = 0;
            (void)hipGetDevice(&dev);
            if (dev < 0 || dev >= 64 || !asked[dev]) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fa_chunk_kernel<D, F16, false, false, true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, smem_kb);
                if (dev >= 0 && dev < 64) asked[dev] = true;
            }
        }
        hipLaunchKernelGGL((fa_chunk_kernel<D, F16, false, false, true>), grid, block, smem_kb, st, a);
        if (a.nsplit > 1) sa_launch::fa_decode_combine(a, D, F16, st);
        return;
    }
    if constexpr (!F16) {
        q8 = a.k_scale != nullptr;
        if (q8 && pg) hipLaunchKernelGGL((fa_chunk_kernel<D, false, true, true>), grid, block, smem, st, a);
        else if (q8) hipLaunchKernelGGL((fa_chunk_kernel<D, false, true, false>), grid, block, smem, st, a);
    }
    if (!q8 && pg) hipLaunchKernelGGL((fa_chunk_kernel<D, F16, false, true>), grid, block, smem, st, a);
    else if (!q8) hipLaunchKernelGGL((fa_chunk_kernel<D, F16, false, false>), grid, block, smem, st, a);
    if (a.nsplit > 1) sa_launch::fa_decode_combine(a, D, F16, st);
}

}  // namespace

namespace sa_launch {
int fa_chunk_max_split_keys(bool paged) { return paged ? kMaxPagedSpan : (1 << 30); }

// One split unless the row tiles leave compute units idle; then splits of whole 64-key tiles until the grid fills the
// chip (256 CUs) or every split is one tile.  Host values only.  splits > 0 forces that many (tests).
void fa_chunk_plan(int64_t max_q, int64_t max_k, int Hkv, int group, int nseg, bool paged, int splits, int& split_keys,
                   int& nsplit) {
    const int64_t tiles = std::max<int64_t>(1, (max_k + 63) / 64);
    const int64_t wgs = std::max<int64_t>(1, (max_q * group + 127) / 128) * Hkv * std::max(nseg, 1);
    int64_t want = splits > 0 ? splits : (wgs >= 256 ? 1 : (256 + wgs - 1) / wgs);
    want = std::min(want, tiles);
    int64_t per = (tiles + want - 1) / want;  // tiles per split
    per = std::min<int64_t>(per, fa_chunk_max_split_keys(paged) / 64);
    split_keys = (int)(per * 64);
    nsplit = (int)std::max<int64_t>(1, (tiles + per - 1) / per);
}

void fa_chunk(const DecArgs& a, int D, bool f16, int max_q, hipStream_t st) {
    if (f16) {
        if (D == 128) launch<128, true>(a, max_q, st);
        else if (D == 64) launch<64, true>(a, max_q, st);
        else launch<32, true>(a, max_q, st);
    } else {
        if (D == 128) launch<128, false>(a, max_q, st);
        else if (D == 64) launch<64, false>(a, max_q, st);
        else launch<32, false>(a, max_q, st);
    }
}
}  // namespace sa_launch
