// Image inputs on the device, gfx950 (include/gfla_image.h): Pillow's nearest-neighbour affine transform fused with
// ToTensor + Normalize, and Pillow's 8-bit bilinear / bicubic resize, byte for byte.
//
// affine_images is two launches.  The first, one small workgroup per sample, reads the sample's matrix and writes its
// record into the workspace: the branch (Pillow's ImagingScaleAffine, its affine_fixed, or poisoned), the six 16.16
// fixed-point coefficients, and for the scale branch xin[W] and yin[H], each made by ONE lane with the W (H) double
// additions in Pillow's order -- the running sum is part of the result -- and converted by all.  The second is normalize_images' kernel
// (csrc/pose_inputs.hip) with a gather in front: a workgroup takes 1024 consecutive output pixels of one sample, every thread
// finds the source pixel of four of them -- two table reads or two integer multiply-adds, the branch being uniform over the
// workgroup -- and puts its C bytes (or the fill) into LDS, interleaved; then each channel's span of the plane is stored
// through the 256-entry table of ((v / 255) - mean) / std like any span (store_span): elements up to the first 16-byte
// boundary, 16-byte packs, elements after the last one.  A poisoned sample runs the same stores through a table of NaN.
// Consecutive lanes gather consecutive output pixels, whose sources are neighbours along a line of the source image: byte
// loads that share cache lines, from an image the size of the output's smallest plane.
// resize_pass is one output byte per thread: up to ksize byte loads `inner` apart (lanes side by side), int32 coefficients
// that the whole wave shares, a 32-bit accumulator.
#include "gfla_common.h"
#include "span_store.h"

namespace gfla {

constexpr int kAffPix = 1024;                  // output pixels per workgroup: 4 KB of uint8 at C = 4
constexpr int kAffRecord = 8;                  // int32 per sample in front of its tables: mode, a0 .. a5, unused
constexpr int kAffTableThreads = 128;          // two waves: one makes xin, the other yin
constexpr int kAffChain = 512;                 // running sums per axis staged in LDS at a time: 8 KB
constexpr int64_t kAffMaxSide = 32768;
constexpr double kAffLimit = 32767.0;
constexpr int64_t kImgMaxGrid = 2147483647;
constexpr int64_t kResizeMaxTaps = 4096;
enum { kAffScale = 0, kAffFixed = 1, kAffPoisoned = 2 };

// ---- the per-sample records ----------------------------------------------------------------------------------------
__device__ __forceinline__ int affine_fix(double v) {
#pragma clang fp contract(off)
  return (int)floor(v * 65536.0 + 0.5);
}

__global__ __launch_bounds__(kAffTableThreads) void affine_tables_kernel(const double *__restrict__ inverse,
                                                                         int32_t *__restrict__ tables, int H, int W) {
#pragma clang fp contract(off)
  const double *m = inverse + 6 * (int64_t)blockIdx.x;
  int32_t *rec = tables + (int64_t)blockIdx.x * (kAffRecord + W + H);
  const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
  bool bad = false;
  for (int e = 0; e < 6; ++e) bad = bad || !__builtin_isfinite(m[e]);
  for (int corner = 0; corner < 4; ++corner) {
    const double x = (corner & 1) ? (double)W : 0.0, y = (corner & 2) ? (double)H : 0.0;
    const double u = x * m0 + y * m1 + m2, v = x * m3 + y * m4 + m5;
    bad = bad || !(fabs(u) < kAffLimit) || !(fabs(v) < kAffLimit);
  }
  const int mode = bad ? kAffPoisoned : (m1 == 0.0 && m3 == 0.0) ? kAffScale : kAffFixed;
  const int tid = threadIdx.x;
  if (tid < kAffRecord) {
    int v = 0;
    if (tid == 0) v = mode;
    if (mode == kAffFixed) {
      if (tid == 1) v = affine_fix(m0);
      if (tid == 2) v = affine_fix(m1);
      if (tid == 3) v = affine_fix(m2 + m0 * 0.5 + m1 * 0.5);
      if (tid == 4) v = affine_fix(m3);
      if (tid == 5) v = affine_fix(m4);
      if (tid == 6) v = affine_fix(m5 + m3 * 0.5 + m4 * 0.5);
    }
    rec[tid] = v;
  }
  if (mode != kAffScale) return;                     // the whole workgroup: the barriers below are uniform
  // One lane per axis (lane 0 of each wave) makes the running sums, n additions one after another, kAffChain at a time
  // into LDS: nothing but the addition and an LDS write sits in the serial loop.  All threads then turn them into table
  // entries (|o| stays below 32767 + |step|: the corners bound it).
  __shared__ double chain[2][kAffChain];
  const int axis = tid >> 6;
  const double step = axis ? m4 : m0;
  double o = (axis ? m5 : m2) + step * 0.5;
  for (int base = 0; base < max(W, H); base += kAffChain) {
    if ((tid & 63) == 0) {
      const int n = min(kAffChain, (axis ? H : W) - base);
      for (int i = 0; i < n; ++i) {
        chain[axis][i] = o;
        o += step;
      }
    }
    __syncthreads();
    for (int a = 0; a < 2; ++a) {
      const int n = min(kAffChain, (a ? H : W) - base);
      int32_t *table = rec + kAffRecord + (a ? W : 0) + base;
      for (int i = tid; i < n; i += kAffTableThreads) {
        const double v = chain[a][i];
        table[i] = v < 0.0 ? -1 : (int)v;
      }
    }
    __syncthreads();
  }
}

// ---- the gather ----------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void affine_images_kernel(const uint8_t *__restrict__ images,
                                                               const int32_t *__restrict__ tables, T *__restrict__ out, int H,
                                                               int W, int C, int chunks, NormCoef coef, uint32_t fill) {
  __shared__ uint4 raw[kAffPix * 4 / 16];            // the chosen bytes, interleaved like a source pixel
  __shared__ float lut[4 * 256];
  const int64_t b = blockIdx.x / chunks;
  const int P = H * W;
  const int p0 = (int)(blockIdx.x - b * chunks) * kAffPix;
  const int npix = min(kAffPix, P - p0);
  const int tid = threadIdx.x;
  const int32_t *rec = tables + b * (kAffRecord + W + H);
  const int mode = rec[0];
  uint8_t *bytes = reinterpret_cast<uint8_t *>(raw);
  if (mode == kAffPoisoned) {
    for (int c = 0; c < C; ++c) lut[c * 256 + tid] = __builtin_nanf("");
    for (int i = tid; i < npix * C; i += kBlock) bytes[i] = 0;
  } else {
    norm_lut_fill(lut, C, coef);
    const uint32_t a0 = (uint32_t)rec[1], a1 = (uint32_t)rec[2], a2 = (uint32_t)rec[3];
    const uint32_t a3 = (uint32_t)rec[4], a4 = (uint32_t)rec[5], a5 = (uint32_t)rec[6];
    const int32_t *tx = rec + kAffRecord, *ty = tx + W;
    const uint8_t *src = images + b * P * C;
    for (int i = tid; i < npix; i += kBlock) {
      const int p = p0 + i;
      const int y = p / W, x = p - y * W;
      int xin, yin;
      if (mode == kAffScale) {
        xin = tx[x];
        yin = ty[y];
      } else {                                       // the sums fit an int32 (|coordinate| < 32767), the terms wrap
        xin = (int32_t)(a2 + a0 * (uint32_t)x + a1 * (uint32_t)y) >> 16;
        yin = (int32_t)(a5 + a3 * (uint32_t)x + a4 * (uint32_t)y) >> 16;
      }
      const bool inside = xin >= 0 && xin < W && yin >= 0 && yin < H;
      const uint8_t *s = src + ((int64_t)(inside ? yin : 0) * W + (inside ? xin : 0)) * C;
      for (int c = 0; c < C; ++c) bytes[i * C + c] = inside ? s[c] : (uint8_t)(fill >> (8 * c));
    }
  }
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    NormGen gen;
    gen.px = bytes + c;
    gen.lut = lut + c * 256;
    gen.C = C;
    store_span(out + ((b * C + c) * (int64_t)P + p0), npix, gen);
  }
}

static int affine_shape_status(int64_t B, int64_t H, int64_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return GFLA_ERR_BAD_SHAPE;
  if (H > kAffMaxSide || W > kAffMaxSide || H > kImgMaxGrid / W) return GFLA_ERR_UNSUPPORTED;
  if (B > kImgMaxGrid / ceil_div(H * W, kAffPix)) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

template <typename T>
static int affine_images(const uint8_t *images, const double *inverse, T *out, void *workspace, int64_t B, int64_t H,
                         int64_t W, int64_t C, const double *fill, const double *mean, const double *std,
                         gfla_stream_t stream) {
  if (images == nullptr || inverse == nullptr || out == nullptr || workspace == nullptr || fill == nullptr ||
      mean == nullptr || std == nullptr)
    return GFLA_ERR_NULL_POINTER;
  if (C < 1 || C > 4) return GFLA_ERR_BAD_SHAPE;
  const int shape = affine_shape_status(B, H, W);
  if (shape == GFLA_ERR_BAD_SHAPE) return shape;
  NormCoef coef = {};
  uint32_t fills = 0;
  for (int c = 0; c < C; ++c) {
    coef.mean[c] = (float)mean[c];
    coef.std[c] = (float)std[c];
    if (!__builtin_isfinite(coef.mean[c]) || !__builtin_isfinite(coef.std[c]) || coef.std[c] == 0.f)
      return GFLA_ERR_BAD_SHAPE;
    if (!(fill[c] >= 0.0 && fill[c] <= 255.0) || fill[c] != (double)(int)fill[c]) return GFLA_ERR_BAD_SHAPE;
    fills |= (uint32_t)(int)fill[c] << (8 * c);
  }
  if (shape != GFLA_OK) return shape;
  const int64_t chunks = ceil_div(H * W, kAffPix);
  hipLaunchKernelGGL(affine_tables_kernel, dim3((unsigned)B), dim3(kAffTableThreads), 0, static_cast<hipStream_t>(stream),
                     inverse, static_cast<int32_t *>(workspace), (int)H, (int)W);
  hipLaunchKernelGGL(affine_images_kernel<T>, dim3((unsigned)(B * chunks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), images, static_cast<const int32_t *>(workspace), out, (int)H, (int)W,
                     (int)C, (int)chunks, coef, fills);
  return launch_status();
}

// ---- one axis of the resize ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void resize_pass_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                             const int32_t *__restrict__ coeffs,
                                                             const int32_t *__restrict__ bounds, int in_len, int out_len,
                                                             int inner, int ksize, int total) {
  const int64_t at = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (at >= total) return;
  const int e = (int)at;
  const int row = e / inner, i = e - row * inner;
  const int o = row / out_len, j = row - o * out_len;
  const int first = clampi(bounds[2 * j], 0, in_len - 1);
  const int count = min(min(bounds[2 * j + 1], ksize), in_len - first);
  const uint8_t *s = src + ((int64_t)o * in_len + first) * inner + i;
  const int32_t *k = coeffs + (int64_t)j * ksize;
  uint32_t acc = 1u << 21;                           // wraps like Pillow's int where a table is not Pillow's
  for (int q = 0; q < count; ++q) acc += (uint32_t)s[(int64_t)q * inner] * (uint32_t)k[q];
  dst[e] = (uint8_t)clampi((int32_t)acc >> 22, 0, 255);
}

static int resize_pass(const uint8_t *src, uint8_t *dst, const int32_t *coeffs, const int32_t *bounds, int64_t outer,
                       int64_t in_len, int64_t out_len, int64_t inner, int64_t ksize, gfla_stream_t stream) {
  if (src == nullptr || dst == nullptr || coeffs == nullptr || bounds == nullptr) return GFLA_ERR_NULL_POINTER;
  if (outer <= 0 || in_len <= 0 || out_len <= 0 || inner <= 0 || ksize <= 0) return GFLA_ERR_BAD_SHAPE;
  if (ksize > kResizeMaxTaps || outer > kImgMaxGrid / inner) return GFLA_ERR_UNSUPPORTED;
  if (outer * inner > kImgMaxGrid / in_len || outer * inner > kImgMaxGrid / out_len) return GFLA_ERR_UNSUPPORTED;
  const int64_t total = outer * inner * out_len;
  hipLaunchKernelGGL(resize_pass_kernel, dim3((unsigned)ceil_div(total, kBlock)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), src, dst, coeffs, bounds, (int)in_len, (int)out_len, (int)inner,
                     (int)ksize, (int)total);
  return launch_status();
}

}  // namespace gfla

using namespace gfla;

extern "C" int64_t gfla_affine_images_workspace_bytes(int64_t B, int64_t H, int64_t W) {
  const int shape = affine_shape_status(B, H, W);
  return shape != GFLA_OK ? shape : B * (kAffRecord + W + H) * (int64_t)sizeof(int32_t);
}

#define GFLA_DEF_AFFINE(SFX, S)                                                                                          \
  extern "C" int gfla_affine_images_##SFX(const uint8_t *images, const double *inverse, S *out, void *workspace, int64_t B, \
                                          int64_t H, int64_t W, int64_t C, const double *fill, const double *mean,        \
                                          const double *std, gfla_stream_t stream) {                                     \
    return affine_images(images, inverse, as<elem_##SFX>(out), workspace, B, H, W, C, fill, mean, std, stream);          \
  }
GFLA_DEF_AFFINE(f32, float)
GFLA_DEF_AFFINE(f16, uint16_t)
GFLA_DEF_AFFINE(bf16, uint16_t)
#undef GFLA_DEF_AFFINE

extern "C" int gfla_resize_pass_u8(const uint8_t *src, uint8_t *dst, const int32_t *coeffs, const int32_t *bounds,
                                   int64_t outer, int64_t in_len, int64_t out_len, int64_t inner, int64_t ksize,
                                   gfla_stream_t stream) {
  return resize_pass(src, dst, coeffs, bounds, outer, in_len, out_len, inner, ksize, stream);
}
