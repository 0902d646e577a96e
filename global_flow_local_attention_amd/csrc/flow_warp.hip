// Bilinear flow warp (the reference's three grid_sample warps), gfx950.
//
// For an output position (x, y) of an H x W flow and an Hs x Ws source the sampling position, in source PIXELS, is
//   ix = (x + gx flow_x) mx ,   iy = (y + gy flow_y) my
// and out[b,c,y,x] is the bilinear interpolation of source[b,c] at (ix, iy) with zero padding: a corner outside the map
// contributes 0.  This is grid_sample(mode="bilinear", padding_mode="zeros", align_corners=True) without the normalised
// grid: with align_corners=True a grid value g maps to the pixel (g + 1) / 2 * (size - 1), so the reference's formulas
// reduce to
//   "correctness"  external_function.py:309-319   grid = 2 x/(w-1) - 1 + 2 flow_x / w  (y alike with h)
//                  ix = x + flow_x (w-1)/w,  iy = y + flow_y (h-1)/h          gx = (w-1)/w  gy = (h-1)/h  mx = my = 1
//   "block"        base_function.py:495-506       grid = 2 (x + flow_x)/(w-1) - 1,  2 (y + flow_y)/(w-1) - 1: BOTH axes
//                  are divided by w - 1 (kept as the reference has it)
//                  ix = x + flow_x,  iy = (y + flow_y) (h-1)/(w-1)            gx = gy = 1   mx = 1  my = (h-1)/(w-1)
//   "pixel"        poseflownet_model.py:86-103    grid = 2 (x + flow_x)/(w-1) - 1,  2 (y + flow_y)/(h-1) - 1
//                  ix = x + flow_x,  iy = y + flow_y                          gx = gy = mx = my = 1
// The kernels take the four scalars, not a name.
//
// Layout.  The op is bandwidth-bound: four gathers per output element, and the C channels of a position share one set
// of weights and corner offsets.  Lanes run along the flattened output positions (64 consecutive positions per wave: the
// flow loads, the gradient loads and the output stores are whole 256-byte lines, the gathers are as local as the flow is
// smooth); position, floor, weights, the four in-plane offsets and their in-range flags are computed once per lane; the
// waves of a workgroup share the 64 positions and split the channels.
//   forward        workgroup = 64 positions x a group of channels (kWarpCG), wave w takes channels w, w + 4, ...
//   d/d flow       workgroup = 64 positions x ALL channels: every wave sums its channels in ascending order, the partial
//                  sums meet in the LDS and wave 0 adds them in wave order and stores: one writer per element, no atomics,
//                  bit-identical from call to call (the number of waves is a function of the shape only)
//   d/d source     the forward's grid; every in-range corner receives weight x gradient through a float atomic into a
//                  buffer of the flow's precision that the entry point zero-fills itself.  The one output of the op that
//                  is not bit-reproducible; it is launched only when grad_source is given.
// The source is read as stored (float16 / bfloat16 widen exactly at the load).  Every address is formed from CLAMPED
// corner coordinates, so it lies inside the plane wherever the flow points (NaN included); an out-of-range corner's value
// is replaced by 0 after the load, and it receives no atomic.
//
// Precision.  The position, its floor and the two fractions are formed once per lane in float64 from the flow as stored
// and the scalars as given (a float32 position of 32-64 px carries 2e-6 px of rounding, which d/d flow_x sees through
// its dependence on the y fraction, and the forward through both).  The fractions are then rounded to the flow's
// precision (float32; float64 for f64), and the weights and the forward's interpolation run in it; the output is rounded
// once at the store.  d/d flow keeps the fractions, the differences of corner values, the products and the sum over
// channels in float64 for every storage type (two fused multiply-adds per channel next to four gathers), so a 32-bit
// result is rounded once.
#include "gfla_common.h"

namespace gfla {

constexpr int kWarpCG = 32;          // channels per forward / source-gradient workgroup (8 per wave)
constexpr int kWarpMaxWaves = 16;    // d/d flow: waves per workgroup
constexpr int64_t kWarpMaxPlane = 0x7fffffffLL;   // H W and Hs Ws: in-plane offsets are 32-bit

struct WarpTaps {
  int off[4];      // (y0,x0) (y0,x0+1) (y0+1,x0) (y0+1,x0+1): clamped, always inside the plane
  bool in[4];
  double ax, ay;   // fractions along x / y
};

// floor of a position as an int in [-2, size]: -2 and `size` stand for "both corners out of range" (NaN goes to -2)
__device__ __forceinline__ int warp_floor_index(double f, int size) {
  return !(f >= -2.0) ? -2 : (f > (double)size ? size : (int)f);
}

__device__ __forceinline__ WarpTaps warp_taps(double fx, double fy, int x, int y, int Hs, int Ws, double gx, double gy,
                                              double mx, double my) {
  WarpTaps t;
  const double ix = ((double)x + gx * fx) * mx, iy = ((double)y + gy * fy) * my;
  const double x0f = floor(ix), y0f = floor(iy);
  t.ax = ix - x0f;
  t.ay = iy - y0f;
  const int x0 = warp_floor_index(x0f, Ws), y0 = warp_floor_index(y0f, Hs);
  const bool xin0 = (unsigned)x0 < (unsigned)Ws, xin1 = (unsigned)(x0 + 1) < (unsigned)Ws;
  const bool yin0 = (unsigned)y0 < (unsigned)Hs, yin1 = (unsigned)(y0 + 1) < (unsigned)Hs;
  const int xa = clampi(x0, 0, Ws - 1), xb = clampi(x0 + 1, 0, Ws - 1);
  const int ya = clampi(y0, 0, Hs - 1) * Ws, yb = clampi(y0 + 1, 0, Hs - 1) * Ws;
  t.off[0] = ya + xa; t.off[1] = ya + xb; t.off[2] = yb + xa; t.off[3] = yb + xb;
  t.in[0] = yin0 & xin0; t.in[1] = yin0 & xin1; t.in[2] = yin1 & xin0; t.in[3] = yin1 & xin1;
  return t;
}

// blockIdx.x = (b * ngroups + group) * nblk + position block
struct WarpBlock {
  int b, c0, c1, p;
  bool active;
};
__device__ __forceinline__ WarpBlock warp_block(int C, int HW, int nblk, int ngroups) {
  WarpBlock w;
  int bid = blockIdx.x;
  const int blk = bid % nblk;
  bid /= nblk;
  const int g = bid % ngroups;
  w.b = bid / ngroups;
  w.c0 = g * kWarpCG;
  w.c1 = min(C, w.c0 + kWarpCG);
  w.p = blk * 64 + (int)(threadIdx.x & 63);
  w.active = w.p < HW;
  if (!w.active) w.p = HW - 1;
  return w;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void flow_warp_fwd_kernel(const T *__restrict__ src,
                                                               const typename Num<T>::acc *__restrict__ flow,
                                                               typename Num<T>::acc *__restrict__ out, int C, int Hs,
                                                               int Ws, int H, int W, int nblk, int ngroups, double gx,
                                                               double gy, double mx, double my) {
  using A = typename Num<T>::acc;
  const int HW = H * W;
  const WarpBlock wb = warp_block(C, HW, nblk, ngroups);
  if (!wb.active) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int y = wb.p / W, x = wb.p - y * W;
  const A *fl = flow + (int64_t)wb.b * 2 * HW;
  const WarpTaps t = warp_taps(fl[wb.p], fl[HW + wb.p], x, y, Hs, Ws, gx, gy, mx, my);
  const A ax = (A)t.ax, ay = (A)t.ay;
  const A w00 = (1 - ax) * (1 - ay), w01 = ax * (1 - ay), w10 = (1 - ax) * ay, w11 = ax * ay;
  const int64_t splane = (int64_t)Hs * Ws;
#pragma unroll 2
  for (int c = wb.c0 + wave; c < wb.c1; c += kBlock / 64) {
    const T *pl = src + ((int64_t)wb.b * C + c) * splane;
    const A v00 = Num<T>::ld(pl + t.off[0]), v01 = Num<T>::ld(pl + t.off[1]);
    const A v10 = Num<T>::ld(pl + t.off[2]), v11 = Num<T>::ld(pl + t.off[3]);
    A s = w00 * (t.in[0] ? v00 : (A)0);
    s += w01 * (t.in[1] ? v01 : (A)0);
    s += w10 * (t.in[2] ? v10 : (A)0);
    s += w11 * (t.in[3] ? v11 : (A)0);
    out[((int64_t)wb.b * C + c) * HW + wb.p] = s;
  }
}

// blockIdx.x = b * nblk + position block; blockDim.x = 64 * nw
template <typename T>
__global__ __launch_bounds__(64 * kWarpMaxWaves) void flow_warp_bwd_flow_kernel(
    const T *__restrict__ src, const typename Num<T>::acc *__restrict__ flow,
    const typename Num<T>::acc *__restrict__ grad_out, typename Num<T>::acc *__restrict__ grad_flow, int C, int Hs, int Ws,
    int H, int W, int nblk, double gx, double gy, double mx, double my) {
  using A = typename Num<T>::acc;
  __shared__ double red[2][kWarpMaxWaves - 1][64];
  const int HW = H * W;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nw = blockDim.x >> 6;
  const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
  const int pl = blk * 64 + lane;
  const bool active = pl < HW;
  const int p = active ? pl : HW - 1;
  const int y = p / W, x = p - y * W;
  const A *fl = flow + (int64_t)b * 2 * HW;
  const WarpTaps t = warp_taps(fl[p], fl[HW + p], x, y, Hs, Ws, gx, gy, mx, my);
  const double ax = t.ax, ay = t.ay;
  const int64_t splane = (int64_t)Hs * Ws;
  double sx = 0, sy = 0;
#pragma unroll 2
  for (int c = wave; c < C; c += nw) {
    const T *sp = src + ((int64_t)b * C + c) * splane;
    const double v00 = t.in[0] ? (double)Num<T>::ld(sp + t.off[0]) : 0.0;
    const double v01 = t.in[1] ? (double)Num<T>::ld(sp + t.off[1]) : 0.0;
    const double v10 = t.in[2] ? (double)Num<T>::ld(sp + t.off[2]) : 0.0;
    const double v11 = t.in[3] ? (double)Num<T>::ld(sp + t.off[3]) : 0.0;
    const double g = grad_out[((int64_t)b * C + c) * HW + p];
    sx += g * ((1 - ay) * (v01 - v00) + ay * (v11 - v10));
    sy += g * ((1 - ax) * (v10 - v00) + ax * (v11 - v01));
  }
  if (wave > 0) {
    red[0][wave - 1][lane] = sx;
    red[1][wave - 1][lane] = sy;
  }
  __syncthreads();
  if (wave == 0 && active) {
    for (int w = 1; w < nw; ++w) {
      sx += red[0][w - 1][lane];
      sy += red[1][w - 1][lane];
    }
    A *gf = grad_flow + (int64_t)b * 2 * HW;
    gf[p] = (A)(sx * (gx * mx));
    gf[HW + p] = (A)(sy * (gy * my));
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void flow_warp_bwd_src_kernel(const typename Num<T>::acc *__restrict__ flow,
                                                                   const typename Num<T>::acc *__restrict__ grad_out,
                                                                   typename Num<T>::acc *__restrict__ grad_src, int C,
                                                                   int Hs, int Ws, int H, int W, int nblk, int ngroups,
                                                                   double gx, double gy, double mx, double my) {
  using A = typename Num<T>::acc;
  const int HW = H * W;
  const WarpBlock wb = warp_block(C, HW, nblk, ngroups);
  if (!wb.active) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int y = wb.p / W, x = wb.p - y * W;
  const A *fl = flow + (int64_t)wb.b * 2 * HW;
  const WarpTaps t = warp_taps(fl[wb.p], fl[HW + wb.p], x, y, Hs, Ws, gx, gy, mx, my);
  const A ax = (A)t.ax, ay = (A)t.ay;
  const A w[4] = {(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay};
  const int64_t splane = (int64_t)Hs * Ws;
  for (int c = wb.c0 + wave; c < wb.c1; c += kBlock / 64) {
    const A g = grad_out[((int64_t)wb.b * C + c) * HW + wb.p];
    A *pl = grad_src + ((int64_t)wb.b * C + c) * splane;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (t.in[k]) atomic_add(pl + t.off[k], w[k] * g);
  }
}

static int warp_check(int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W) {
  if (B <= 0 || C <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return GFLA_ERR_BAD_SHAPE;
  // 32-bit in-plane offsets and a one-dimensional grid
  if (Hs > kWarpMaxPlane / Ws || H > kWarpMaxPlane / W || C > kWarpMaxPlane) return GFLA_ERR_UNSUPPORTED;
  const int64_t nblk = ceil_div(H * W, 64);
  if (B > kWarpMaxPlane / nblk || B * nblk > kWarpMaxPlane / ceil_div(C, kWarpCG)) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

// waves of a d/d flow workgroup: a function of the shape only.  Few workgroups (small maps): more waves each, so that the
// channel loop of a position is spread over the CU; never more waves than channels.
static int warp_flow_waves(int64_t workgroups, int64_t C) {
  int nw = workgroups >= 16 * kNumCU ? 4 : (workgroups >= 4 * kNumCU ? 8 : kWarpMaxWaves);
  while (nw > 1 && nw > C) nw >>= 1;
  return nw;
}

template <typename T>
static int warp_fwd(const T *source, const typename Num<T>::acc *flow, typename Num<T>::acc *out, int64_t B, int64_t C,
                    int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                    gfla_stream_t stream) {
  if (!source || !flow || !out) return GFLA_ERR_NULL_POINTER;
  if (int rc = warp_check(B, C, Hs, Ws, H, W)) return rc;
  const int64_t nblk = ceil_div(H * W, 64), ngroups = ceil_div(C, kWarpCG);
  flow_warp_fwd_kernel<T><<<dim3((unsigned)(B * ngroups * nblk)), kBlock, 0, static_cast<hipStream_t>(stream)>>>(
      source, flow, out, (int)C, (int)Hs, (int)Ws, (int)H, (int)W, (int)nblk, (int)ngroups, gx, gy, mx, my);
  return launch_status();
}

template <typename T>
static int warp_bwd(const T *source, const typename Num<T>::acc *flow, const typename Num<T>::acc *grad_out,
                    typename Num<T>::acc *grad_source, typename Num<T>::acc *grad_flow, int64_t B, int64_t C, int64_t Hs,
                    int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my, gfla_stream_t stream) {
  using A = typename Num<T>::acc;
  if (!source || !flow || !grad_out) return GFLA_ERR_NULL_POINTER;
  if (int rc = warp_check(B, C, Hs, Ws, H, W)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nblk = ceil_div(H * W, 64), ngroups = ceil_div(C, kWarpCG);
  if (grad_flow) {
    const int nw = warp_flow_waves(B * nblk, C);
    flow_warp_bwd_flow_kernel<T><<<dim3((unsigned)(B * nblk)), 64 * nw, 0, st>>>(
        source, flow, grad_out, grad_flow, (int)C, (int)Hs, (int)Ws, (int)H, (int)W, (int)nblk, gx, gy, mx, my);
  }
  if (grad_source) {
    if (hipMemsetAsync(grad_source, 0, (size_t)(B * C * Hs * Ws) * sizeof(A), st) != hipSuccess) return GFLA_ERR_LAUNCH;
    flow_warp_bwd_src_kernel<T><<<dim3((unsigned)(B * ngroups * nblk)), kBlock, 0, st>>>(
        flow, grad_out, grad_source, (int)C, (int)Hs, (int)Ws, (int)H, (int)W, (int)nblk, (int)ngroups, gx, gy, mx, my);
  }
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int gfla_flow_warp_fwd_f32(const float *source, const float *flow, float *out, int64_t B, int64_t C, int64_t Hs, int64_t Ws,
                           int64_t H, int64_t W, double gx, double gy, double mx, double my, gfla_stream_t stream) {
  return gfla::warp_fwd<float>(source, flow, out, B, C, Hs, Ws, H, W, gx, gy, mx, my, stream);
}
int gfla_flow_warp_fwd_f64(const double *source, const double *flow, double *out, int64_t B, int64_t C, int64_t Hs,
                           int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                           gfla_stream_t stream) {
  return gfla::warp_fwd<double>(source, flow, out, B, C, Hs, Ws, H, W, gx, gy, mx, my, stream);
}
int gfla_flow_warp_fwd_f16(const uint16_t *source, const float *flow, float *out, int64_t B, int64_t C, int64_t Hs,
                           int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                           gfla_stream_t stream) {
  return gfla::warp_fwd<f16_t>(reinterpret_cast<const f16_t *>(source), flow, out, B, C, Hs, Ws, H, W, gx, gy, mx, my,
                               stream);
}
int gfla_flow_warp_fwd_bf16(const uint16_t *source, const float *flow, float *out, int64_t B, int64_t C, int64_t Hs,
                            int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                            gfla_stream_t stream) {
  return gfla::warp_fwd<bf16_t>(reinterpret_cast<const bf16_t *>(source), flow, out, B, C, Hs, Ws, H, W, gx, gy, mx, my,
                                stream);
}

int gfla_flow_warp_bwd_f32(const float *source, const float *flow, const float *grad_out, float *grad_source,
                           float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                           double gy, double mx, double my, gfla_stream_t stream) {
  return gfla::warp_bwd<float>(source, flow, grad_out, grad_source, grad_flow, B, C, Hs, Ws, H, W, gx, gy, mx, my, stream);
}
int gfla_flow_warp_bwd_f64(const double *source, const double *flow, const double *grad_out, double *grad_source,
                           double *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                           double gy, double mx, double my, gfla_stream_t stream) {
  return gfla::warp_bwd<double>(source, flow, grad_out, grad_source, grad_flow, B, C, Hs, Ws, H, W, gx, gy, mx, my, stream);
}
int gfla_flow_warp_bwd_f16(const uint16_t *source, const float *flow, const float *grad_out, float *grad_source,
                           float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                           double gy, double mx, double my, gfla_stream_t stream) {
  return gfla::warp_bwd<f16_t>(reinterpret_cast<const f16_t *>(source), flow, grad_out, grad_source, grad_flow, B, C, Hs,
                               Ws, H, W, gx, gy, mx, my, stream);
}
int gfla_flow_warp_bwd_bf16(const uint16_t *source, const float *flow, const float *grad_out, float *grad_source,
                            float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                            double gy, double mx, double my, gfla_stream_t stream) {
  return gfla::warp_bwd<bf16_t>(reinterpret_cast<const bf16_t *>(source), flow, grad_out, grad_source, grad_flow, B, C, Hs,
                                Ws, H, W, gx, gy, mx, my, stream);
}
}
