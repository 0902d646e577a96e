// Device helpers shared by the implicit-GEMM convolutions (conv3x3.hip, gen_conv.hip): the 32-byte [pixel][channel-chunk]
// record, one MFMA step over a chunk for float32 / float16 / bfloat16, and the raw bits of a stored element.
#pragma once

#include "gfla_common.h"

namespace gfla {

typedef float cv_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 cv_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 cv_bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kCvRec = 32;        // bytes of one pixel (or one output channel) of one chunk

template <typename T>
constexpr int cv_ck() { return kCvRec / (int)sizeof(T); }

template <typename T>
__device__ __forceinline__ cv_f32x16 cv_mma(uint4 a, uint4 b, cv_f32x16 acc) {
  if constexpr (__is_same(T, float)) {
    const float4 fa = __builtin_bit_cast(float4, a), fb = __builtin_bit_cast(float4, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
  } else if constexpr (__is_same(T, f16_t)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(cv_f16x8, a), __builtin_bit_cast(cv_f16x8, b), acc, 0,
                                                  0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(cv_bf16x8, a), __builtin_bit_cast(cv_bf16x8, b), acc,
                                                   0, 0, 0);
  }
}

template <typename T>
__device__ __forceinline__ uint32_t cv_bits(const T *p) {
  if constexpr (__is_same(T, float)) return __float_as_uint(*p);
  else return p->bits;
}

}  // namespace gfla
