// 2x2 max pooling, stride 2, floor mode (the four pools of VGG19, external_function.py:323-444): an odd last row or column
// is dropped and its gradient is zero.  Forward: one thread per output element, the winner's stored bits are copied.
// Backward: one thread per INPUT element; it finds the winner of its window again from the saved pool input (no index
// tensor) and writes g or 0, so every element of dX is written exactly once: no atomics, no memset.  Ties go to the first
// maximum in scan order (row, then column), as F.max_pool2d does; a NaN wins its window, as there.  16-bit values are
// compared after exact widening.
#include "gfla_common.h"

namespace gfla {

// index 0..3 (scan order) of the first maximum of the window whose top-left element is p.  F.max_pool2d's rule: a later
// element replaces the winner if it is larger OR a NaN, so a window with a NaN in it returns NaN (the last one in scan
// order) and routes the gradient there.
template <typename T>
__device__ __forceinline__ int pool_winner(const T *p, int W) {
  float best = (float)Num<T>::ld(p);
  int at = 0;
  const float b = (float)Num<T>::ld(p + 1), c = (float)Num<T>::ld(p + W), d = (float)Num<T>::ld(p + W + 1);
  if (b > best || b != b) { best = b; at = 1; }
  if (c > best || c != c) { best = c; at = 2; }
  if (d > best || d != d) { best = d; at = 3; }
  return at;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void maxpool2x2_fwd_kernel(const T *__restrict__ x, T *__restrict__ y, int64_t total,
                                                                int H, int W, int Ho, int Wo) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int ox = (int)(idx % Wo), oy = (int)((idx / Wo) % Ho);
  const int64_t pl = idx / ((int64_t)Wo * Ho);
  const T *p = x + pl * H * (int64_t)W + (int64_t)(2 * oy) * W + 2 * ox;
  const int at = pool_winner<T>(p, W);
  y[idx] = p[(at >> 1) * W + (at & 1)];
}

template <typename T>
__global__ __launch_bounds__(kBlock) void maxpool2x2_bwd_kernel(const T *__restrict__ x, const T *__restrict__ gy,
                                                                T *__restrict__ gx, int64_t total, int H, int W, int Ho,
                                                                int Wo) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int ix = (int)(idx % W), iy = (int)((idx / W) % H);
  const int64_t pl = idx / ((int64_t)W * H);
  const int ox = ix >> 1, oy = iy >> 1;
  T g;
  __builtin_memset(&g, 0, sizeof(T));
  if (ox < Wo && oy < Ho) {
    const T *p = x + pl * H * (int64_t)W + (int64_t)(2 * oy) * W + 2 * ox;
    if (pool_winner<T>(p, W) == (iy & 1) * 2 + (ix & 1)) g = gy[(pl * Ho + oy) * Wo + ox];
  }
  gx[idx] = g;
}

static int pool_check(int64_t B, int64_t C, int64_t H, int64_t W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return GFLA_ERR_BAD_SHAPE;
  if (H > 0x3fffffffLL || W > 0x3fffffffLL || ceil_div(B * C * H * W, kBlock) > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

template <typename T>
static int maxpool_fwd(const T *x, T *y, int64_t B, int64_t C, int64_t H, int64_t W, gfla_stream_t stream) {
  if (!x || !y) return GFLA_ERR_NULL_POINTER;
  if (int rc = pool_check(B, C, H, W)) return rc;
  const int64_t Ho = H / 2, Wo = W / 2, total = B * C * Ho * Wo;
  if (total == 0) return GFLA_OK;   // H or W of 1: an empty output
  maxpool2x2_fwd_kernel<T><<<dim3((unsigned)ceil_div(total, kBlock)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      x, y, total, (int)H, (int)W, (int)Ho, (int)Wo);
  return launch_status();
}

template <typename T>
static int maxpool_bwd(const T *x, const T *grad_y, T *grad_x, int64_t B, int64_t C, int64_t H, int64_t W,
                       gfla_stream_t stream) {
  const bool empty = H / 2 == 0 || W / 2 == 0;   // nothing to read from grad_y: dX is all zero
  if (!x || !grad_x || (!grad_y && !empty)) return GFLA_ERR_NULL_POINTER;
  if (int rc = pool_check(B, C, H, W)) return rc;
  const int64_t total = B * C * H * W;
  maxpool2x2_bwd_kernel<T><<<dim3((unsigned)ceil_div(total, kBlock)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      x, grad_y, grad_x, total, (int)H, (int)W, (int)(H / 2), (int)(W / 2));
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
#define GFLA_DEF_MAXPOOL(SFX, T, CT)                                                                                    \
  int gfla_maxpool2x2_fwd_##SFX(const T *x, T *y, int64_t B, int64_t C, int64_t H, int64_t W, gfla_stream_t stream) {   \
    return gfla::maxpool_fwd<CT>(reinterpret_cast<const CT *>(x), reinterpret_cast<CT *>(y), B, C, H, W, stream);       \
  }                                                                                                                     \
  int gfla_maxpool2x2_bwd_##SFX(const T *x, const T *grad_y, T *grad_x, int64_t B, int64_t C, int64_t H, int64_t W,     \
                                gfla_stream_t stream) {                                                                 \
    return gfla::maxpool_bwd<CT>(reinterpret_cast<const CT *>(x), reinterpret_cast<const CT *>(grad_y),                 \
                                 reinterpret_cast<CT *>(grad_x), B, C, H, W, stream);                                   \
  }
GFLA_DEF_MAXPOOL(f32, float, float)
GFLA_DEF_MAXPOOL(f16, uint16_t, f16_t)
GFLA_DEF_MAXPOOL(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_MAXPOOL
}
