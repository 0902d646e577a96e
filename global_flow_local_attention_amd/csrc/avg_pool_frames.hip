// AvgPool3d(kernel (3,2,2), stride (1,2,2)) on frames-major activations x (B,L,C,H,W), the pool in front of the shortcut of
// a ResBlock3DEncoder (base_function.py:63), forward and backward.
//
//   p[b,lo,c,i,j] = (1/12) sum over frames lo .. lo + 2 of the 2 x 2 block at (2i, 2j)        (B,L-2,C,H/2,W/2)
//                   one float32 sum, frame ascending and within a frame ((x00 + x01) + x10) + x11 as torch walks it,
//                   times 1/12, rounded to T once; torch's floor: an odd trailing row or column is dropped
//   dx[b,l,c,y,x] = (1/12) sum over lo in [max(0, l - 2), min(l, L - 3)] of g[b,lo,c,y/2,x/2], lo ascending, float32,
//                   rounded once; ZERO in the trailing row / column of an odd H / W
//
// Owner-computes in both directions: every element of the result is written by exactly one lane, no atomics, no clearing
// pass, bit-identical from call to call.  A thread owns NV = 16 / sizeof(T) consecutive elements of a row of the result
// and moves them with one 16-byte store where the addresses allow it -- the row length a multiple of what a thread owns
// and the pointers on 16-byte (the gradient's g: 8-byte) boundaries --, and one element otherwise; the arithmetic per element
// is the same on both routes (include/gfla_hip.h, "Pointer placement").
#include "gfla_common.h"

namespace gfla {

constexpr float kPool12 = 1.f / 12.f;

// the float32 sum times 1/12, rounded to T.  float16: the product is rounded to float32 and that value converted, by this
// one instruction on both routes -- left to the compiler, the element route fuses the product into the conversion
// (v_fma_mixlo_f16) and the 16-byte route converts pairs (v_cvt_pk_f16_f32), and the two differed in the last bit of a
// few results of a 70 x 80 map
template <typename T>
__device__ __forceinline__ T pool_mean(float sum) {
  const float v = sum * kPool12;
  if constexpr (__is_same(T, f16_t)) {
    uint32_t h;
    asm("v_cvt_f16_f32 %0, %1" : "=v"(h) : "v"(v));
    return f16_t::from_bits((uint16_t)h);
  } else {
    return (T)v;
  }
}

// NV outputs per thread; x rows of W elements, y rows of Wo = W / 2
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void avg_pool_frames_fwd_kernel(const T *__restrict__ x, T *__restrict__ y, int L, int C,
                                                                     int H, int W, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2, Lo = L - 2, WV = Wo / NV;
  const int jv = (int)(idx % WV), i = (int)((idx / WV) % Ho), c = (int)((idx / WV / Ho) % C);
  const int64_t n = idx / WV / Ho / C, b = n / Lo;
  const int lo = (int)(n - b * Lo);
  const int64_t plane = (int64_t)H * W;
  float s[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) s[k] = 0.f;
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const T *row = x + ((b * L + lo + f) * C + c) * plane + (int64_t)(2 * i) * W + 2 * jv * NV;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
      if constexpr (NV == 1) {
        s[0] += Num<T>::ld(row + dy * W);
        s[0] += Num<T>::ld(row + dy * W + 1);
      } else {
        const Pack<T, NV> a = *reinterpret_cast<const Pack<T, NV> *>(row + dy * W);
        const Pack<T, NV> c2 = *reinterpret_cast<const Pack<T, NV> *>(row + dy * W + NV);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
          const Pack<T, NV> &src = 2 * k < NV ? a : c2;
          s[k] += Num<T>::ld(&src.v[(2 * k) % NV]);
          s[k] += Num<T>::ld(&src.v[(2 * k) % NV + 1]);
        }
      }
    }
  }
  T *out = y + ((n * C + c) * Ho + i) * (int64_t)Wo + jv * NV;
  if constexpr (NV == 1) {
    out[0] = pool_mean<T>(s[0]);
  } else {
    Pack<T, NV> o;
#pragma unroll
    for (int k = 0; k < NV; ++k) o.v[k] = pool_mean<T>(s[k]);
    *reinterpret_cast<Pack<T, NV> *>(out) = o;
  }
}

// NV elements of dx per thread; g rows of Wo = W / 2
template <typename T, int NV>
__global__ __launch_bounds__(kBlock) void avg_pool_frames_bwd_kernel(const T *__restrict__ g, T *__restrict__ dx, int L, int C,
                                                                     int H, int W, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (idx >= total) return;
  const int Ho = H / 2, Wo = W / 2, Lo = L - 2, WV = W / NV;
  const int xv = (int)(idx % WV), yy = (int)((idx / WV) % H), c = (int)((idx / WV / H) % C);
  const int64_t n = idx / WV / H / C, b = n / L;
  const int l = (int)(n - b * L);
  const int lo0 = l - 2 < 0 ? 0 : l - 2, lo1 = l < Lo - 1 ? l : Lo - 1;
  T *out = dx + ((n * C + c) * H + yy) * (int64_t)W + xv * NV;
  if constexpr (NV == 1) {
    float s = 0.f;
    if (yy < 2 * Ho && xv < 2 * Wo)
      for (int lo = lo0; lo <= lo1; ++lo) s += Num<T>::ld(g + (((b * Lo + lo) * C + c) * Ho + yy / 2) * (int64_t)Wo + xv / 2);
    out[0] = pool_mean<T>(s);
  } else {                                              // W is a multiple of NV: even, no trailing column
    float s[NV / 2];
#pragma unroll
    for (int k = 0; k < NV / 2; ++k) s[k] = 0.f;
    if (yy < 2 * Ho)
      for (int lo = lo0; lo <= lo1; ++lo) {
        const Pack<T, NV / 2> a = *reinterpret_cast<const Pack<T, NV / 2> *>(
            g + (((b * Lo + lo) * C + c) * Ho + yy / 2) * (int64_t)Wo + xv * (NV / 2));
#pragma unroll
        for (int k = 0; k < NV / 2; ++k) s[k] += Num<T>::ld(&a.v[k]);
      }
    Pack<T, NV> o;
#pragma unroll
    for (int k = 0; k < NV; ++k) o.v[k] = pool_mean<T>(s[k / 2]);
    *reinterpret_cast<Pack<T, NV> *>(out) = o;
  }
}

static int pool_frames_check(int64_t B, int64_t L, int64_t C, int64_t H, int64_t W) {
  if (B <= 0 || L <= 0 || C <= 0 || H <= 0 || W <= 0 || L < 3 || H < 2 || W < 2) return GFLA_ERR_BAD_SHAPE;
  if (H > 0x7fffffffLL || W > 0x7fffffffLL || H * W > 0x7fffffffLL || L > 65535 || B * L > 65535 || C > 65536)
    return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

static bool aligned_to(const void *p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

template <typename T>
static int avg_pool_frames_fwd(const T *x, T *y, int64_t B, int64_t L, int64_t C, int64_t H, int64_t W, gfla_stream_t stream) {
  if (!x || !y) return GFLA_ERR_NULL_POINTER;
  const int rc = pool_frames_check(B, L, C, H, W);
  if (rc != GFLA_OK) return rc;
  if (!aligned_to(x, sizeof(T)) || !aligned_to(y, sizeof(T))) return GFLA_ERR_UNSUPPORTED;
  constexpr int NV = 16 / (int)sizeof(T);
  const bool vec = W % (2 * NV) == 0 && aligned_to(x, 16) && aligned_to(y, 16);
  const int64_t total = B * (L - 2) * C * (H / 2) * ((W / 2) / (vec ? NV : 1)), blocks = ceil_div(total, kBlock);
  if (blocks > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) avg_pool_frames_fwd_kernel<T, NV><<<dim3((unsigned)blocks), kBlock, 0, s>>>(x, y, (int)L, (int)C, (int)H, (int)W, total);
  else avg_pool_frames_fwd_kernel<T, 1><<<dim3((unsigned)blocks), kBlock, 0, s>>>(x, y, (int)L, (int)C, (int)H, (int)W, total);
  return launch_status();
}

template <typename T>
static int avg_pool_frames_bwd(const T *g, T *dx, int64_t B, int64_t L, int64_t C, int64_t H, int64_t W, gfla_stream_t stream) {
  if (!g || !dx) return GFLA_ERR_NULL_POINTER;
  const int rc = pool_frames_check(B, L, C, H, W);
  if (rc != GFLA_OK) return rc;
  if (!aligned_to(g, sizeof(T)) || !aligned_to(dx, sizeof(T))) return GFLA_ERR_UNSUPPORTED;
  constexpr int NV = 16 / (int)sizeof(T);
  const bool vec = W % NV == 0 && aligned_to(dx, 16) && aligned_to(g, 8);
  const int64_t total = B * L * C * H * (W / (vec ? NV : 1)), blocks = ceil_div(total, kBlock);
  if (blocks > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) avg_pool_frames_bwd_kernel<T, NV><<<dim3((unsigned)blocks), kBlock, 0, s>>>(g, dx, (int)L, (int)C, (int)H, (int)W, total);
  else avg_pool_frames_bwd_kernel<T, 1><<<dim3((unsigned)blocks), kBlock, 0, s>>>(g, dx, (int)L, (int)C, (int)H, (int)W, total);
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
#define GFLA_DEF_AVG_POOL_FRAMES(SFX, T, CT)                                                                             \
  int gfla_avg_pool_frames_fwd_##SFX(const T *x, T *y, int64_t B, int64_t L, int64_t C, int64_t H, int64_t W,            \
                                     gfla_stream_t stream) {                                                             \
    return gfla::avg_pool_frames_fwd<CT>(reinterpret_cast<const CT *>(x), reinterpret_cast<CT *>(y), B, L, C, H, W,      \
                                         stream);                                                                        \
  }                                                                                                                      \
  int gfla_avg_pool_frames_bwd_##SFX(const T *grad_y, T *grad_x, int64_t B, int64_t L, int64_t C, int64_t H, int64_t W,  \
                                     gfla_stream_t stream) {                                                             \
    return gfla::avg_pool_frames_bwd<CT>(reinterpret_cast<const CT *>(grad_y), reinterpret_cast<CT *>(grad_x), B, L, C,  \
                                         H, W, stream);                                                                  \
  }
GFLA_DEF_AVG_POOL_FRAMES(f32, float, float)
GFLA_DEF_AVG_POOL_FRAMES(f16, uint16_t, f16_t)
GFLA_DEF_AVG_POOL_FRAMES(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_AVG_POOL_FRAMES
}
