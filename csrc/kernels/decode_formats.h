// Activation and weight-format traits shared by the MFMA weight-streaming decode kernels (skinny.hip, wide.hip).
#pragma once
#include "common.h"

namespace sa {

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

}  // namespace sa
