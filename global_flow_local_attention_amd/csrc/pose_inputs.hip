// Pose inputs on the device, gfx950 (include/gfla_pose.h): key points -> Gaussian heat maps, heat maps -> key points,
// interleaved uint8 images -> normalised planes.
//
// pose_maps is a pure store stream: B J H W elements out, B J 2 + B 9 doubles in.  The squared distance is an integer
// and the exponential factorises, so a workgroup -- one (b, j, band of kPoseBand rows) -- evaluates W + kPoseBand
// one-axis exponentials in double into LDS and every element is one double multiplication rounded to float32 once.  A
// band of whole rows is one contiguous span of the output, so it is stored like any span (store_span): elements up to
// the first 16-byte boundary, 16-byte packs, elements after the last one.  Missing joints and poisoned ones run the same
// stores with factors of 0 and NaN.  The stream is as fast as its instruction count per element allows (a wave64
// instruction takes four cycles): a thread divides once, steps from pack to pack by a precomputed (rows, columns), and a
// pack inside one row at a multiple of its width is V LDS loads at constant offsets times one row factor.
// pose_cords is one workgroup per plane: 16-byte loads, a (value, lowest index) pair per thread, a wave reduction and
// four pairs through LDS.
// normalize_images stages 1024 interleaved pixels in LDS with 16-byte loads, at the byte phase of their address, and
// writes each channel's span through a 256-entry table of ((v / 255) - mean) / std, one entry per thread.
#include "gfla_common.h"
#include "span_store.h"

namespace gfla {

constexpr int kPoseBand = 32;                  // rows per workgroup
constexpr int64_t kPoseMaxW = 4096;            // ex[W] (skewed: + W / 32) + ey[kPoseBand] doubles in LDS: 34 KB
constexpr double kPoseClamp = 1073741824.0;    // 2^30
constexpr int kNormPix = 1024;                 // pixels per workgroup: 4 KB of uint8 at C = 4
constexpr int64_t kMaxGrid = 2147483647;

// ---- key points -> heat maps ---------------------------------------------------------------------------------------
// ex lives in LDS skewed by one double per 32: the lanes of a wave, whose columns are V apart, then read from 32 different
// banks, and the V columns of a pack that starts at a multiple of V stay consecutive
__device__ __forceinline__ int pose_ex_slot(int i) { return i + (i >> 5); }

template <int V>
struct PoseGen {
  const double *ex, *ey;
  int W, drow, dcol;                                 // kBlock * V elements as whole rows and columns
  int row, col;
  __device__ __forceinline__ void seek(int k) {
    row = k / W;
    col = k - row * W;
  }
  __device__ __forceinline__ void jump(int) {
    row += drow;
    col += dcol;
    if (col >= W) {
      col -= W;
      ++row;
    }
  }
  __device__ __forceinline__ float next() {
    const float v = (float)(ex[pose_ex_slot(col)] * ey[row]);      // one rounding to float32, denormals kept
    if (++col == W) {
      col = 0;
      ++row;
    }
    return v;
  }
  template <typename T>
  __device__ __forceinline__ void pack(Pack<T, V> &q) {
    if ((col & (V - 1)) == 0 && col + V <= W) {      // within one row, at a multiple of V: V loads at constant offsets
      const double *e = ex + pose_ex_slot(col);
      const double y = ey[row];
#pragma unroll
      for (int i = 0; i < V; ++i) q.v[i] = Num<T>::from((float)(e[i] * y));
    } else {
      const int r = row, c = col;
      for (int i = 0; i < V; ++i) q.v[i] = Num<T>::from(next());
      row = r;
      col = c;
    }
  }
};

// the centre (c0: row, c1: column) of one joint; returns 0: a Gaussian, 1: missing, 2: poisoned
__device__ __forceinline__ int pose_centre(const double *__restrict__ cord, const double *__restrict__ a, int affine_stride,
                                           double H, double W, double H0, double W0, int64_t &c0, int64_t &c1) {
#pragma clang fp contract(off)
  const double y = cord[0], x = cord[1];
  if (y == -1.0 || x == -1.0) return 1;
  bool bad = !__builtin_isfinite(y) || !__builtin_isfinite(x);
  const double p0 = (y / H0) * H, p1 = (x / W0) * W;
  double r0 = p1, r1 = p0;                           // r0: column, r1: row
  if (a != nullptr) {
    for (int e = 0; e < affine_stride; ++e) bad = bad || !__builtin_isfinite(a[e]);
    r0 = a[0] * p1 + a[1] * p0 + a[2];
    r1 = a[3] * p1 + a[4] * p0 + a[5];
  }
  if (bad || r0 != r0 || r1 != r1) return 2;
  c0 = (int64_t)fmin(fmax(trunc(r1), -kPoseClamp), kPoseClamp);
  c1 = (int64_t)fmin(fmax(trunc(r0), -kPoseClamp), kPoseClamp);
  return 0;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void pose_maps_kernel(const double *__restrict__ cords,
                                                           const double *__restrict__ affine, int affine_stride,
                                                           T *__restrict__ out, int J, int H, int W, int bands, double H0,
                                                           double W0, double two_sigma_sq) {
  constexpr int V = 16 / (int)sizeof(T);
  extern __shared__ double pose_fac[];               // ex (skewed), ey[rows of this band]
  const int ey0 = pose_ex_slot(W - 1) + 1;
  const int64_t bj = blockIdx.x / bands;
  const int band = (int)(blockIdx.x - bj * bands);
  const int row0 = band * kPoseBand;
  const int rows = min(kPoseBand, H - row0);
  const int tid = threadIdx.x;
  int64_t c0 = 0, c1 = 0;
  const int kind = pose_centre(cords + 2 * bj, affine == nullptr ? nullptr : affine + (bj / J) * affine_stride,
                               affine_stride, (double)H, (double)W, H0, W0, c0, c1);
  for (int i = tid; i < W + rows; i += kBlock) {
    double v = 0.0;
    if (kind == 2) {
      v = __builtin_nan("");
    } else if (kind == 0) {
      const int64_t d = i < W ? (int64_t)i - c1 : (int64_t)(row0 + i - W) - c0;
      v = exp(-(double)(d * d) / two_sigma_sq);
    }
    pose_fac[i < W ? pose_ex_slot(i) : ey0 + i - W] = v;
  }
  __syncthreads();
  PoseGen<V> gen;
  gen.ex = pose_fac;
  gen.ey = pose_fac + ey0;
  gen.W = W;
  gen.drow = (kBlock * V) / W;
  gen.dcol = (kBlock * V) - gen.drow * W;
  store_span(out + (bj * H + row0) * W, rows * W, gen);
}

template <typename T>
static int pose_maps(const double *cords, const double *affine, int64_t affine_stride, T *out, int64_t B, int64_t J,
                     int64_t H, int64_t W, int64_t H0, int64_t W0, double two_sigma_sq, gfla_stream_t stream) {
  if (cords == nullptr || out == nullptr) return GFLA_ERR_NULL_POINTER;
  if (B <= 0 || J <= 0 || H <= 0 || W <= 0 || H0 <= 0 || W0 <= 0) return GFLA_ERR_BAD_SHAPE;
  if (!(two_sigma_sq > 0) || !(two_sigma_sq <= 1.7976931348623157e308)) return GFLA_ERR_BAD_SHAPE;
  if (affine != nullptr && affine_stride != 6 && affine_stride != 9) return GFLA_ERR_BAD_SHAPE;
  if (W > kPoseMaxW || H > kMaxGrid || J > kMaxGrid) return GFLA_ERR_UNSUPPORTED;
  const int64_t bands = ceil_div(H, kPoseBand);
  if (B > kMaxGrid / J || B * J > kMaxGrid / bands) return GFLA_ERR_UNSUPPORTED;
  const size_t lds = (size_t)(W + ((W - 1) >> 5) + kPoseBand) * sizeof(double);     // pose_ex_slot(W - 1) + 1 for ex
  hipLaunchKernelGGL(pose_maps_kernel<T>, dim3((unsigned)(B * J * bands)), dim3(kBlock), lds,
                     static_cast<hipStream_t>(stream), cords, affine, (int)affine_stride, out, (int)J, (int)H, (int)W,
                     (int)bands, (double)H0, (double)W0, two_sigma_sq);
  return launch_status();
}

// ---- heat maps -> key points ---------------------------------------------------------------------------------------
struct Peak {
  float v;
  int at, nan;
  __device__ __forceinline__ void take(float x, int i) {
    nan |= x != x;
    if (x > v || (x == v && i < at)) {               // float comparison: -0 == +0; a NaN never wins
      v = x;
      at = i;
    }
  }
};

template <typename T>
__global__ __launch_bounds__(kBlock) void pose_cords_kernel(const T *__restrict__ maps, int64_t *__restrict__ out, int n,
                                                            int W, float threshold) {
  constexpr int V = 16 / (int)sizeof(T);
  const T *src = maps + (int64_t)blockIdx.x * n;
  const int tid = threadIdx.x;
  Peak p;
  p.v = -__builtin_inff();
  p.at = 2147483647;
  p.nan = 0;
  int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u)) & 15u) / sizeof(T));
  if (head > n) head = n;
  if (tid < head) p.take(Num<T>::ld(src + tid), tid);
  const int nv = (n - head) / V;
  for (int v = tid; v < nv; v += kBlock) {
    const int k = head + v * V;
    const Pack<T, V> q = *reinterpret_cast<const Pack<T, V> *>(src + k);
#pragma unroll
    for (int e = 0; e < V; ++e) p.take(Num<T>::ld(&q.v[e]), k + e);
  }
  const int done = head + nv * V;
  if (tid < n - done) p.take(Num<T>::ld(src + done + tid), done + tid);

  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_xor(p.v, off);
    const int oat = __shfl_xor(p.at, off);
    p.nan |= __shfl_xor(p.nan, off);
    if (ov > p.v || (ov == p.v && oat < p.at)) {
      p.v = ov;
      p.at = oat;
    }
  }
  __shared__ float wave_v[kBlock / 64];
  __shared__ int wave_at[kBlock / 64], wave_nan[kBlock / 64];
  if ((tid & 63) == 0) {
    wave_v[tid >> 6] = p.v;
    wave_at[tid >> 6] = p.at;
    wave_nan[tid >> 6] = p.nan;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kBlock / 64; ++w) {
      p.nan |= wave_nan[w];
      if (wave_v[w] > p.v || (wave_v[w] == p.v && wave_at[w] < p.at)) {
        p.v = wave_v[w];
        p.at = wave_at[w];
      }
    }
    const bool hit = !p.nan && p.v > threshold;
    out[2 * (int64_t)blockIdx.x] = hit ? p.at / W : -1;
    out[2 * (int64_t)blockIdx.x + 1] = hit ? p.at % W : -1;
  }
}

template <typename T>
static int pose_cords(const T *maps, int64_t *out, int64_t planes, int64_t H, int64_t W, double threshold,
                      gfla_stream_t stream) {
  if (maps == nullptr || out == nullptr) return GFLA_ERR_NULL_POINTER;
  if (planes <= 0 || H <= 0 || W <= 0 || threshold != threshold) return GFLA_ERR_BAD_SHAPE;
  if (planes > kMaxGrid || H > kMaxGrid / W) return GFLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pose_cords_kernel<T>, dim3((unsigned)planes), dim3(kBlock), 0, static_cast<hipStream_t>(stream), maps,
                     out, (int)(H * W), (int)W, (float)threshold);
  return launch_status();
}

// ---- uint8 images -> network input ---------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void normalize_images_kernel(const uint8_t *__restrict__ images, T *__restrict__ out,
                                                                  int64_t P, int C, int chunks, NormCoef coef) {
  __shared__ uint4 raw[kNormPix * 4 / 16 + 2];       // the pixels at the byte phase of their address
  __shared__ float lut[4 * 256];
  const int64_t b = blockIdx.x / chunks;
  const int64_t p0 = (int64_t)(blockIdx.x - b * chunks) * kNormPix;
  const int npix = (int)min((int64_t)kNormPix, P - p0);
  const int nbytes = npix * C;
  const int tid = threadIdx.x;
  norm_lut_fill(lut, C, coef);
  const uint8_t *src = images + (b * P + p0) * C;
  uint8_t *bytes = reinterpret_cast<uint8_t *>(raw);
  const int phase = (int)(reinterpret_cast<uintptr_t>(src) & 15u);
  int head = (16 - phase) & 15;
  if (head > nbytes) head = nbytes;
  if (tid < head) bytes[phase + tid] = src[tid];
  const int nv = (nbytes - head) / 16;
  for (int v = tid; v < nv; v += kBlock)
    raw[(phase + head) / 16 + v] = *reinterpret_cast<const uint4 *>(src + head + 16 * v);
  const int done = head + nv * 16;
  if (tid < nbytes - done) bytes[phase + done + tid] = src[done + tid];
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    NormGen gen;
    gen.px = bytes + phase + c;
    gen.lut = lut + c * 256;
    gen.C = C;
    store_span(out + ((b * C + c) * P + p0), npix, gen);
  }
}

template <typename T>
static int normalize_images(const uint8_t *images, T *out, int64_t B, int64_t H, int64_t W, int64_t C, const double *mean,
                            const double *std, gfla_stream_t stream) {
  if (images == nullptr || out == nullptr || mean == nullptr || std == nullptr) return GFLA_ERR_NULL_POINTER;
  if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4) return GFLA_ERR_BAD_SHAPE;
  NormCoef coef = {};
  for (int c = 0; c < C; ++c) {
    coef.mean[c] = (float)mean[c];
    coef.std[c] = (float)std[c];
    if (!__builtin_isfinite(coef.mean[c]) || !__builtin_isfinite(coef.std[c]) || coef.std[c] == 0.f)
      return GFLA_ERR_BAD_SHAPE;
  }
  if (H > kMaxGrid / W) return GFLA_ERR_UNSUPPORTED;
  const int64_t P = H * W, chunks = ceil_div(P, kNormPix);
  if (B > kMaxGrid / chunks) return GFLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(normalize_images_kernel<T>, dim3((unsigned)(B * chunks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), images, out, P, (int)C, (int)chunks, coef);
  return launch_status();
}

}  // namespace gfla

using namespace gfla;

extern "C" int64_t gfla_pose_maps_band_rows(void) { return kPoseBand; }

#define GFLA_DEF_POSE(SFX, S)                                                                                           \
  extern "C" int gfla_pose_maps_##SFX(const double *cords, const double *affine, int64_t affine_stride, S *out, int64_t B, \
                                      int64_t J, int64_t H, int64_t W, int64_t H0, int64_t W0, double two_sigma_sq,      \
                                      gfla_stream_t stream) {                                                           \
    return pose_maps(cords, affine, affine_stride, as<elem_##SFX>(out), B, J, H, W, H0, W0, two_sigma_sq, stream);      \
  }                                                                                                                     \
  extern "C" int gfla_pose_cords_##SFX(const S *maps, int64_t *out, int64_t planes, int64_t H, int64_t W,                \
                                       double threshold, gfla_stream_t stream) {                                        \
    return pose_cords(as<elem_##SFX>(maps), out, planes, H, W, threshold, stream);                                      \
  }                                                                                                                     \
  extern "C" int gfla_normalize_images_##SFX(const uint8_t *images, S *out, int64_t B, int64_t H, int64_t W, int64_t C, \
                                             const double *mean, const double *std, gfla_stream_t stream) {             \
    return normalize_images(images, as<elem_##SFX>(out), B, H, W, C, mean, std, stream);                                \
  }
GFLA_DEF_POSE(f32, float)
GFLA_DEF_POSE(f16, uint16_t)
GFLA_DEF_POSE(bf16, uint16_t)
#undef GFLA_DEF_POSE
