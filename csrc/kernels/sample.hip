// Fused top-k / top-p / temperature sampling for decoding: one launch, one workgroup per row of logits [B, V],
// device operations only (graph-capturable; the step counter is read from device memory).
//
// Semantics (ops/sample.py holds the float64 twin):
//   top-k  keep logits >= the k-th largest logit (tie-mates kept); k <= 0 or k >= V: off
//   top-p  softmax at temperature 1 over what top-k kept; walking the distinct logit values downwards, the cut is the
//          first value whose inclusive cumulative mass exceeds p; keep logits >= cut; p >= 1: off
//   draw   softmax(logit / T) over the kept set, inverse CDF in token-index order with one uniform u in [0, 1): the
//          first kept index whose inclusive cumulative probability exceeds u.  -inf (and NaN) logits are never drawn.
//   u      counter-based: a pure function of (seed, step, row) built from mix32 (flash_attn.h).
//
// No sort.  Both cut values come from an MSB-first radix selection over an order-preserving 32-bit key of the logit:
// 8 bits per pass, a 256-bin LDS histogram of 64-bit integer weights (top-k: 1 per token; top-p: exp(x - max) in
// 2^-40 fixed point).  Integer LDS atomics are order-independent, so the bins, and with them the cuts, are bitwise
// reproducible; the draw sums per-wave partials in a fixed order (fp64) and narrows the token range 16-fold per
// level down to one row of 64, which a single wave scan resolves.  No float atomics anywhere.
// bf16 / fp16 logits need only the 2 / 3 leading passes: their fp32 images have constant low key bits.
// Each histogram is kept in kRep lane-interleaved copies: logits crowd into a few exponent bins, and same-address LDS
// atomics of one wave instruction serialise.
//
// Rows of V <= kMaxResident are staged once in LDS as fp32 (V = 32000: 128000 B + 18.5 KiB of histograms, asked for
// with hipFuncSetAttribute); longer rows are re-read from L2 in every pass (a row is at most 512 KB).
#include "common.h"
#include "flash_attn.h"
#include "launch.h"

namespace sa {
namespace {

typedef unsigned long long u64;
using fa::mix32;

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kBins = 256, kRep = 8;
constexpr int kMaxResident = 32768;
constexpr double kFix = 1099511627776.0;  // 2^40: sum over < 2^22 tokens of weights <= 2^40 stays below 2^63

// dynamic LDS carve (byte offsets, all multiples of 16)
constexpr int kOffHist = 0;                               // u64 [kRep][kBins]
constexpr int kOffBins = kOffHist + kRep * kBins * 8;     // u64 [kBins]
constexpr int kOffSeg = kOffBins + kBins * 8;             // double [kWaves]
constexpr int kOffCnt = kOffSeg + kWaves * 8;             // int [kWaves]
constexpr int kOffRed = kOffCnt + kWaves * 4;             // float [kWaves]
constexpr int kOffSel = kOffRed + kWaves * 4;             // u64 residual target, int bin
constexpr int kOffRow = kOffSel + 16 + 240;               // float [V + 4] (resident rows; image shifted by <= 3)
static_assert(kOffRow % 16 == 0 && kOffRow == 18944, "LDS carve");

// order-preserving key: a > b  <=>  key(a) > key(b) for non-NaN floats (after -0 -> +0)
__device__ __forceinline__ uint32_t f2key(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}
// -0 -> +0 (ties are by value), NaN -> -inf (never drawn)
__device__ __forceinline__ float canon(float x) {
    x = x + 0.0f;
    return x == x ? x : -INFINITY;
}

__device__ __forceinline__ u64 shfl_up64(u64 v, int d) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_up(lo, d, 64);
    hi = __shfl_up(hi, d, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl64(u64 v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ double shfl_up_d(double v, int d) {
    return __longlong_as_double((long long)shfl_up64((u64)__double_as_longlong(v), d));
}

// The global row in 16-byte-aligned chunks of 8 elements (16-byte vector loads) plus a scalar head / tail:
// f8(i0, v) for the chunk starting at token i0, f1(i, x) for edge tokens.  `head` tokens precede the first aligned one.
template <typename T, typename F8, typename F1>
__device__ __forceinline__ void global_row(const T* g, int V, int head, F8 f8, F1 f1) {
    const int tid = threadIdx.x;
    const int nch = (V - head) >> 3;
    if (tid < head) f1(tid, to_f32(g[tid]));
    for (int i = head + 8 * nch + tid; i < V; i += kThreads) f1(i, to_f32(g[i]));
#pragma unroll 2
    for (int c = tid; c < nch; c += kThreads) {
        float v[8];
        V8<T>::ld(g + head + 8 * c, v);
        f8(head + 8 * c, v);
    }
}

// One row: the fp32 LDS image (RES) or global memory, re-read through L2 in every pass.
template <typename T, bool RES>
struct Row {
    const T* g;
    const float* img;  // LDS image, token i at img[i]
    int V, head;
    __device__ __forceinline__ float at(int i) const {
        if constexpr (RES) return img[i];
        else return canon(to_f32(g[i]));
    }
    // f(x) for every token once, in no particular order
    template <typename F>
    __device__ __forceinline__ void each(F f) const {
        if constexpr (RES) {
#pragma unroll 4
            for (int i = threadIdx.x; i < V; i += kThreads) f(img[i]);
        } else {
            global_row<T>(g, V, head,
                          [&](int, const float (&v)[8]) {
#pragma unroll
                              for (int j = 0; j < 8; ++j) f(canon(v[j]));
                          },
                          [&](int, float x) { f(canon(x)); });
        }
    }
};

// The largest key whose inclusive weight from the top exceeds the target: walking keys downwards, the first key K with
// sum of w over {key >= K} > target, where target = target_of(total weight) < total weight.  w(x, key) is a 64-bit
// integer weight.  NPASS leading bytes of the key are resolved; the rest are constant per sign (bf16 / fp16 images).
template <int NPASS, typename RowT, typename TF, typename W>
__device__ uint32_t radix_select(const RowT& row, TF target_of, W w, char* smem) {
    u64* hist = reinterpret_cast<u64*>(smem + kOffHist);
    u64* bins = reinterpret_cast<u64*>(smem + kOffBins);
    u64* sel_t = reinterpret_cast<u64*>(smem + kOffSel);
    int* sel_b = reinterpret_cast<int*>(smem + kOffSel + 8);
    const int tid = threadIdx.x, lane = tid & 63;
    u64* mine = hist + (lane & (kRep - 1)) * kBins;
    uint32_t prefix = 0;
    u64 target = 0;
    for (int pass = 0; pass < NPASS; ++pass) {
        const int shift = 24 - 8 * pass;
        __syncthreads();  // previous users of hist / bins / sel are done
        for (int i = tid; i < kRep * kBins; i += kThreads) hist[i] = 0;
        __syncthreads();
        row.each([&](float x) {
            const uint32_t key = f2key(x);
            if (pass == 0 || (key >> (shift + 8)) == prefix) {
                const u64 wi = w(x, key);
                if (wi) atomicAdd(&mine[(key >> shift) & 0xff], wi);
            }
        });
        __syncthreads();
        if (tid < kBins) {
            u64 s = 0;
#pragma unroll
            for (int r = 0; r < kRep; ++r) s += hist[r * kBins + tid];
            bins[tid] = s;
        }
        __syncthreads();
        if (tid < 64) {
            // lane l owns bins 255 - 4l .. 252 - 4l (descending); inclusive scan of the lane sums over lanes
            u64 b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = bins[255 - 4 * lane - j];
            const u64 own = b[0] + b[1] + b[2] + b[3];
            u64 inc = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u64 o = shfl_up64(inc, d);
                if (lane >= d) inc += o;
            }
            if (pass == 0) target = target_of(shfl64(inc, 63));
            u64 run = inc - own;  // weight strictly above this lane's bins
            int hit = -1;
            u64 above = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (hit < 0 && run + b[j] > target) { hit = j; above = run; }
                run += b[j];
            }
            const u64 m = __ballot(hit >= 0);
            // total weight > target guarantees a hit; the guard keeps a broken precondition from hanging anything
            const int first = m ? __ffsll((long long)m) - 1 : 63;
            if (lane == first) {
                *sel_b = hit >= 0 ? 255 - 4 * lane - hit : 0;
                *sel_t = hit >= 0 ? target - above : 0;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | (uint32_t)*sel_b;
        target = *sel_t;
    }
    if constexpr (NPASS < 4) {
        constexpr int rest = 32 - 8 * NPASS;
        const uint32_t fill = (prefix >> (8 * NPASS - 1)) & 1 ? 0u : ((1u << rest) - 1u);  // positive : negative
        prefix = (prefix << rest) | fill;
    }
    return prefix;
}

template <typename T> struct Passes { static constexpr int n = 4; };
template <> struct Passes<u16> { static constexpr int n = 2; };       // bf16: 16 significant bits
template <> struct Passes<_Float16> { static constexpr int n = 3; };  // fp16 -> fp32: 1 + 8 + 10 bits

struct SampleArgs {
    const void* logits; int64_t ld; int V;
    int64_t* tokens; int* info;
    const int64_t* step; uint32_t seed;
    int top_k; float top_p, inv_t;
};

template <typename T, bool RES>
__global__ void __launch_bounds__(kThreads) sample_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int V = a.V;
    const int64_t r = blockIdx.x;
    const T* g = reinterpret_cast<const T*>(a.logits) + r * a.ld;
    float* red = reinterpret_cast<float*>(smem + kOffRed);
    // tokens before the first 16-byte-aligned one; the LDS image is shifted by `pad` floats so that the aligned
    // chunks of 8 land on 16-byte LDS addresses (ds_write_b128)
    const int head = min(V, (int)(((16 - ((uintptr_t)g & 15)) & 15) / sizeof(T)));
    float* img = reinterpret_cast<float*>(smem + kOffRow) + ((4 - (head & 3)) & 3);
    const Row<T, RES> row{g, img, V, head};
    constexpr int NP = Passes<T>::n;

    // ---- stage + row max
    float mx = -INFINITY;
    global_row<T>(g, V, head,
                  [&](int i0, const float (&v)[8]) {
                      f32x4 lo4, hi4;
#pragma unroll
                      for (int j = 0; j < 4; ++j) {
                          lo4[j] = canon(v[j]);
                          hi4[j] = canon(v[j + 4]);
                          mx = fmaxf(mx, fmaxf(lo4[j], hi4[j]));
                      }
                      if constexpr (RES) {
                          *reinterpret_cast<f32x4*>(img + i0) = lo4;
                          *reinterpret_cast<f32x4*>(img + i0 + 4) = hi4;
                      }
                  },
                  [&](int i, float x) {
                      x = canon(x);
                      if constexpr (RES) img[i] = x;
                      mx = fmaxf(mx, x);
                  });
    mx = block_max(mx, red);  // its barriers also publish the LDS image
    if (mx == -INFINITY) {    // nothing can be drawn (block-uniform)
        if (tid == 0) {
            a.tokens[r] = 0;
            if (a.info) { a.info[2 * r] = 0; a.info[2 * r + 1] = (int)__float_as_uint(-INFINITY); }
        }
        return;
    }

    // ---- cuts
    uint32_t cut = f2key(-INFINITY);
    if (a.top_k > 0 && a.top_k < V) {
        const u64 kt = (u64)(a.top_k - 1);
        cut = radix_select<NP>(row, [kt](u64) { return kt; }, [](float, uint32_t) { return (u64)1; }, smem);
    }
    if (a.top_p < 1.0f) {
        const uint32_t kcut = cut;
        const double p = (double)a.top_p;
        // the first pass's bins also give the total mass Z (the maximum alone contributes 2^40), an integer sum and so
        // the same whatever the order: cum > p Z  <=>  cum > floor(p Z)
        cut = radix_select<NP>(
            row,
            [p](u64 Z) {
                const u64 t = (u64)(p * (double)Z);
                return t < Z ? t : Z - 1;  // p just below 1 after rounding: the cut is the smallest massive value
            },
            [mx, kcut](float x, uint32_t key) { return key >= kcut ? (u64)((double)__expf(x - mx) * kFix) : (u64)0; },
            smem);
    }

    // ---- draw.  Tokens in rows of 64; the 16 waves split the current range of rows, sum their weights (per-wave
    // partials added in wave order: reproducible), the range narrows to the wave whose share holds the target, until
    // one row is left; one wave scan resolves it.  Every pass after the first covers 1/16 of the previous one.
    const float c = a.inv_t * 1.44269504088896340736f;
    auto weight = [&](int i, bool& kept) {
        kept = false;
        if (i >= V) return 0.f;
        const float x = row.at(i);
        kept = f2key(x) >= cut && x > -INFINITY;
        return kept ? exp2f((x - mx) * c) : 0.f;
    };
    double* seg = reinterpret_cast<double*>(smem + kOffSeg);
    int* segc = reinterpret_cast<int*>(smem + kOffCnt);
    int lo = 0, n = (V + 63) >> 6;
    double target = 0.0;
    bool first = true;
    for (;;) {
        const int rpw = (n + kWaves - 1) / kWaves;
        const int r0 = lo + wid * rpw, r1 = min(r0 + rpw, lo + n);
        double acc = 0.0;
        int cnt = 0;
#pragma unroll 4
        for (int rr = r0; rr < r1; ++rr) {
            bool kept;
            acc += (double)weight(rr * 64 + lane, kept);
            cnt += kept;
        }
        acc = wave_sum_d(acc);
        if (first) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        }
        __syncthreads();  // the previous level's readers are done
        if (lane == 0) { seg[wid] = acc; segc[wid] = cnt; }
        __syncthreads();
        if (first) {
            double S = 0.0;
            int kept_n = 0;
            for (int w = 0; w < kWaves; ++w) { S += seg[w]; kept_n += segc[w]; }
            const int64_t step = *a.step;
            uint32_t h = mix32(a.seed + 0x9e3779b9u);
            h = mix32(h ^ (uint32_t)step);
            h = mix32(h + (uint32_t)((uint64_t)step >> 32));
            h = mix32(h ^ ((uint32_t)r * 0x85ebca6bu));
            target = (double)(h >> 8) * (1.0 / 16777216.0) * S;
            if (tid == 0 && a.info) {
                a.info[2 * r] = kept_n;
                a.info[2 * r + 1] = (int)__float_as_uint(key2f(cut));
            }
            first = false;
        }
        // the wave whose share holds the target: first w with prefix(w) > target, else (the target sat on the upper
        // edge: summation-order rounding) the last wave with any weight
        int sel = -1, last = 0;
        double before = 0.0, pre = 0.0, lastpre = 0.0;
        for (int w = 0; w < kWaves; ++w) {
            const double s = seg[w];
            if (s > 0.0) { last = w; lastpre = pre; }
            if (sel < 0 && pre + s > target) { sel = w; before = pre; }
            pre += s;
        }
        if (sel < 0) { sel = last; before = lastpre; }
        target -= before;
        const int end = lo + n;
        lo += sel * rpw;
        n = min(rpw, end - lo);
        if (rpw == 1) break;
    }
    if (wid != 0) return;

    bool kept;
    const double wv = (double)weight(lo * 64 + lane, kept);
    double inc = wv;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = shfl_up_d(inc, d);
        if (lane >= d) inc += o;
    }
    const u64 hm = __ballot(wv > 0.0 && inc > target), pm = __ballot(wv > 0.0);
    int token = lo * 64;
    if (hm) token += __ffsll((long long)hm) - 1;
    else if (pm) token += 63 - __clzll((long long)pm);
    if (lane == 0) a.tokens[r] = min(token, V - 1);
}

template <typename T>
void launch_t(const SampleArgs& a, int64_t B, hipStream_t st) {
    if (a.V <= kMaxResident) {
        const size_t lds = (size_t)kOffRow + ((size_t)a.V + 4) * 4;
        if (lds > 65536) {  // more than 64 KiB of dynamic LDS has to be asked for, once per device and kernel
            static bool asked[64] = {};
            int dev = 0;
            (void)hipGetDevice(&dev);
            if (dev < 0 || dev >= 64 || !asked[dev]) {
                (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_kernel<T, true>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, kOffRow + (kMaxResident + 4) * 4);
                if (dev >= 0 && dev < 64) asked[dev] = true;
            }
        }
        hipLaunchKernelGGL((sample_kernel<T, true>), dim3((unsigned)B), dim3(kThreads), lds, st, a);
    } else {
        hipLaunchKernelGGL((sample_kernel<T, false>), dim3((unsigned)B), dim3(kThreads), (size_t)kOffRow, st, a);
    }
    SA_CHECK_LAUNCH();
}

}  // namespace
}  // namespace sa

namespace sa_launch {
int sample_max_resident() { return sa::kMaxResident; }

void sample(int dtype, const void* logits, int64_t ld, int64_t B, int V, int64_t* tokens, int* info,
            const int64_t* step, uint32_t seed, int top_k, float top_p, float temperature, hipStream_t st) {
    sa::SampleArgs a{logits, ld, V, tokens, info, step, seed, top_k, top_p, 1.0f / temperature};
    if (dtype == DT_F32) sa::launch_t<float>(a, B, st);
    else if (dtype == DT_BF16) sa::launch_t<sa::u16>(a, B, st);
    else sa::launch_t<sa::f16>(a, B, st);
}
}  // namespace sa_launch
