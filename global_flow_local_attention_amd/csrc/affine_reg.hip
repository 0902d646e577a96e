// Affine regularisation loss of a flow field (AffineRegularizationLoss, external_function.py:31-77), gfx950.
//
// The reference evaluates, per axis of the sampling grid u = flow + pixel coordinates,
//   loss_axis = mean over (b, valid k x k windows) of  u^T M u ,   M = K^T K,  K = A (A^T A)^-1 A^T - I,  A = [row, col, 1]
// K = P - I with P the projector on the affine functions of the window, so M = I - P, M A = 0, and the coordinate part
// of u (a column of A plus a constant) is annihilated exactly:
//   u^T M u = f^T M f = |f - P f|^2            f = the k x k flow patch of one axis: no grid, no coordinates
// P f is the least-squares plane a + bx*dx + by*dy through the window, dx, dy in {-(k-1)/2 .. (k-1)/2}:
//   a = mean(f),  bx = sum(dx f) / s,  by = sum(dy f) / s,  s = k^2 (k^2 - 1) / 12
// The window's first element is subtracted from f before the fit (constants are annihilated too), so every number that
// is squared or cancelled is a local variation of the flow, not its magnitude.  With r = f - a - bx dx - by dy:
//   loss       = 1/(B L) sum_b sum_axis sum_windows sum_j r_j^2                       L = (H-k+1)(W-k+1)
//   dloss/df_p = 2/(B L) sum over the windows that contain p of r_window[position of p]         (M symmetric, M f = r)
//
// One workgroup owns a kTH x kTW tile of one (b, axis) plane.  It loads the tile plus its halo into the LDS (widened to the
// arithmetic type at the load: the flow is read as stored, float16 / bfloat16 included), fits every window it needs once
// (lane = window), and then
//   forward:  sums r^2 over the windows whose origin lies in the tile (each window has one owner), reduces the workgroup's
//             sum in a fixed tree and writes it to its own slot of the workspace; a one-workgroup kernel adds the slots in
//             a fixed order and writes the loss;
//   backward: every pixel of the tile gathers its residual from the <= k^2 windows that contain it (owner computes),
//             scales by 2 grad_loss / (B L) and stores once in the storage type.
// No atomics: loss and gradient are bit-identical from call to call.  The fit is k^2-wide per window rather than separable
// box sums: the whole loss is ~150 MFLOP at the training batch, the launches are what it costs.
//
// Precision.  The tile is kept as loaded (float32 for f32 / f16 / bf16 flows, float64 for f64); the differences d = f - f[0],
// the sums of the fit, the residuals and every reduction after them are float64 for all storage types, so the only
// rounding of a 16- or 32-bit result is the final store.  Float32 is not enough where the flow is nearly affine over a
// window: the plane is rounded at 6e-8 of the window's linear trend, the residuals are the curvature, 100x smaller, and the
// gradient is an alternating sum of k^2 residuals, smaller again.  Measured on a 0.5 px field over a 200 x 300 map, k = 5
// (DESIGN.md section 5): 3.9e-5 of the largest gradient entry with a float32 fit, 1.5e-5 with float32 differences and a
// float64 fit (f - f[0] is inexact where the two differ in exponent) -- both over the project's float32 bar of 1e-5.
// The float64 part is ~6 k^2 operations per window.
#include "gfla_common.h"

namespace gfla {

constexpr int kTH = 16, kTW = 32;            // pixels of a tile (rows x columns); 256 threads = 2 pixels each
constexpr int kAffineMinK = 2, kAffineMaxK = 7;
constexpr int64_t kAffineMaxDim = 16384;     // H, W: keeps every index in 32 bits

// GRAD = false: the windows whose origin is in the tile; true: every window that contains a pixel of the tile
template <int K, bool GRAD>
struct AffineTile {
  static constexpr int back = GRAD ? K - 1 : 0;
  static constexpr int WY = kTH + back, WX = kTW + back;         // window origins
  static constexpr int FY = WY + K - 1, FX = WX + K - 1;         // flow rows / columns under them
};

// Least-squares plane through the K x K window at `f` (row stride `ld`), after subtracting its first element; returns
// sum r^2.  a = mean(f - f[0]); bx, by the slopes along rows / columns.
template <typename A, int K>
__device__ __forceinline__ double affine_fit(const A *f, int ld, double &a, double &bx, double &by) {
  constexpr double c = (K - 1) / 2.0, inv_n = 1.0 / (K * K), inv_s = 12.0 / (K * K * (K * K - 1));
  const double f0 = f[0];
  double s0 = 0, sy = 0, sx = 0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double row = 0, ramp = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double d = (double)f[i * ld + j] - f0;
      row += d;
      ramp += (j - c) * d;
    }
    s0 += row;
    sy += (i - c) * row;
    sx += ramp;
  }
  a = s0 * inv_n;
  by = sy * inv_s;
  bx = sx * inv_s;
  double ss = 0;
#pragma unroll
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const double r = ((double)f[i * ld + j] - f0) - a - by * (i - c) - bx * (j - c);
      ss += r * r;
    }
  }
  return ss;
}

// Loads the flow under the tile's windows into `fl` (row stride FX).  Returns false when the tile owns no window.
template <typename T, int K, bool GRAD>
__device__ __forceinline__ bool affine_load(const T *__restrict__ plane, int H, int W, int ty0, int tx0,
                                            typename Num<T>::acc *fl, int &wy0, int &wx0, int &nwy, int &nwx) {
  using G = AffineTile<K, GRAD>;
  wy0 = max(ty0 - G::back, 0);
  wx0 = max(tx0 - G::back, 0);
  nwy = min(ty0 + kTH - 1, H - K) - wy0 + 1;
  nwx = min(tx0 + kTW - 1, W - K) - wx0 + 1;
  if (nwy <= 0 || nwx <= 0) return false;
  const int fy = nwy + K - 1, fx = nwx + K - 1;              // <= FY, FX; rows wy0 .. wy0 + fy - 1 <= H - 1
  for (int i = threadIdx.x; i < fy * fx; i += kBlock) {
    const int y = i / fx, x = i - y * fx;
    fl[y * G::FX + x] = Num<T>::ld(plane + (int64_t)(wy0 + y) * W + (wx0 + x));
  }
  return true;
}

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void affine_reg_fwd_kernel(const T *__restrict__ flow, double *__restrict__ partial,
                                                                int H, int W, int tiles_x) {
  using A = typename Num<T>::acc;
  using G = AffineTile<K, false>;
  __shared__ A fl[G::FY * G::FX];
  __shared__ double red[kBlock];
  const int ty0 = (blockIdx.x / tiles_x) * kTH, tx0 = (blockIdx.x % tiles_x) * kTW;
  const T *plane = flow + (int64_t)blockIdx.y * H * W;
  int wy0, wx0, nwy, nwx;
  double sum = 0;
  if (affine_load<T, K, false>(plane, H, W, ty0, tx0, fl, wy0, wx0, nwy, nwx)) {
    __syncthreads();
    for (int w = threadIdx.x; w < nwy * nwx; w += kBlock) {
      const int y = w / nwx, x = w - y * nwx;
      double a, bx, by;
      sum += affine_fit<A, K>(fl + y * G::FX + x, G::FX, a, bx, by);
    }
  }
  red[threadIdx.x] = sum;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
}

// loss = scale * sum(partial[0..n)), one workgroup, fixed order
template <typename A>
__global__ __launch_bounds__(kBlock) void affine_reg_sum_kernel(const double *__restrict__ partial, int64_t n, double scale,
                                                                A *__restrict__ loss) {
  __shared__ double red[kBlock];
  double s = 0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) s += partial[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (A)(red[0] * scale);
}

template <typename T, int K>
__global__ __launch_bounds__(kBlock) void affine_reg_bwd_kernel(const T *__restrict__ flow,
                                                                const typename Num<T>::acc *__restrict__ grad_loss,
                                                                T *__restrict__ grad_flow, int H, int W, int tiles_x,
                                                                double two_over_bl) {
  using A = typename Num<T>::acc;
  using G = AffineTile<K, true>;
  constexpr double c = (K - 1) / 2.0;
  __shared__ A fl[G::FY * G::FX];
  __shared__ double fit[3][G::WY * G::WX];
  const int ty0 = (blockIdx.x / tiles_x) * kTH, tx0 = (blockIdx.x % tiles_x) * kTW;
  const int64_t plane_at = (int64_t)blockIdx.y * H * W;
  int wy0, wx0, nwy, nwx;
  affine_load<T, K, true>(flow + plane_at, H, W, ty0, tx0, fl, wy0, wx0, nwy, nwx);   // ty0 <= H - 1: never empty
  __syncthreads();
  for (int w = threadIdx.x; w < nwy * nwx; w += kBlock) {
    const int y = w / nwx, x = w - y * nwx;
    double a, bx, by;
    affine_fit<A, K>(fl + y * G::FX + x, G::FX, a, bx, by);
    fit[0][y * G::WX + x] = a;
    fit[1][y * G::WX + x] = bx;
    fit[2][y * G::WX + x] = by;
  }
  __syncthreads();
  const double scale = (double)*grad_loss * two_over_bl;
  for (int p = threadIdx.x; p < kTH * kTW; p += kBlock) {
    const int py = ty0 + p / kTW, px = tx0 + p % kTW;
    if (py >= H || px >= W) continue;
    const double fp = fl[(py - wy0) * G::FX + (px - wx0)];
    // windows (wy, wx) with wy <= py <= wy + K - 1, 0 <= wy <= H - K (and the same along x): all fitted above
    const int ya = max(py - K + 1, 0), yb = min(py, H - K), xa = max(px - K + 1, 0), xb = min(px, W - K);
    double g = 0;
    for (int wy = ya; wy <= yb; ++wy) {
      const double dy = (py - wy) - c;
      for (int wx = xa; wx <= xb; ++wx) {
        const int at = (wy - wy0) * G::WX + (wx - wx0);
        const double d = fp - (double)fl[(wy - wy0) * G::FX + (wx - wx0)];   // minus the window's first element
        g += d - fit[0][at] - fit[2][at] * dy - fit[1][at] * ((px - wx) - c);
      }
    }
    grad_flow[plane_at + (int64_t)py * W + px] = (T)(A)(g * scale);
  }
}

static int affine_check(int64_t B, int64_t H, int64_t W, int k) {
  if (B <= 0 || H <= 0 || W <= 0) return GFLA_ERR_BAD_SHAPE;
  if (k < kAffineMinK || k > kAffineMaxK) return GFLA_ERR_UNSUPPORTED;    // k = 1: A^T A is singular, there is no projector
  if (H < k || W < k) return GFLA_ERR_BAD_SHAPE;
  if (H > kAffineMaxDim || W > kAffineMaxDim || 2 * B > 65535) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

static int64_t affine_tiles(int64_t H, int64_t W) { return ceil_div(H, kTH) * ceil_div(W, kTW); }

template <typename T>
static int affine_fwd(const T *flow, void *workspace, typename Num<T>::acc *loss, int64_t B, int64_t H, int64_t W, int k,
                      gfla_stream_t stream) {
  if (!flow || !workspace || !loss) return GFLA_ERR_NULL_POINTER;
  if (int rc = affine_check(B, H, W, k)) return rc;
  const dim3 grid((unsigned)affine_tiles(H, W), (unsigned)(2 * B));
  const int tiles_x = (int)ceil_div(W, kTW);
  double *partial = static_cast<double *>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
#define GFLA_AFFINE_FWD(K_) \
  case K_: affine_reg_fwd_kernel<T, K_><<<grid, kBlock, 0, st>>>(flow, partial, (int)H, (int)W, tiles_x); break;
    GFLA_AFFINE_FWD(2) GFLA_AFFINE_FWD(3) GFLA_AFFINE_FWD(4) GFLA_AFFINE_FWD(5) GFLA_AFFINE_FWD(6) GFLA_AFFINE_FWD(7)
#undef GFLA_AFFINE_FWD
  }
  const double scale = 1.0 / ((double)B * (double)((H - k + 1) * (W - k + 1)));
  affine_reg_sum_kernel<typename Num<T>::acc><<<1, kBlock, 0, st>>>(partial, (int64_t)grid.x * grid.y, scale, loss);
  return launch_status();
}

template <typename T>
static int affine_bwd(const T *flow, const typename Num<T>::acc *grad_loss, T *grad_flow, int64_t B, int64_t H, int64_t W,
                      int k, gfla_stream_t stream) {
  if (!flow || !grad_loss || !grad_flow) return GFLA_ERR_NULL_POINTER;
  if (int rc = affine_check(B, H, W, k)) return rc;
  const dim3 grid((unsigned)affine_tiles(H, W), (unsigned)(2 * B));
  const int tiles_x = (int)ceil_div(W, kTW);
  const double scale = 2.0 / ((double)B * (double)((H - k + 1) * (W - k + 1)));
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (k) {
#define GFLA_AFFINE_BWD(K_) \
  case K_: affine_reg_bwd_kernel<T, K_><<<grid, kBlock, 0, st>>>(flow, grad_loss, grad_flow, (int)H, (int)W, tiles_x, scale); break;
    GFLA_AFFINE_BWD(2) GFLA_AFFINE_BWD(3) GFLA_AFFINE_BWD(4) GFLA_AFFINE_BWD(5) GFLA_AFFINE_BWD(6) GFLA_AFFINE_BWD(7)
#undef GFLA_AFFINE_BWD
  }
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_affine_reg_workspace_bytes(int64_t B, int64_t H, int64_t W, int k) {
  if (int rc = gfla::affine_check(B, H, W, k)) return rc;
  return 2 * B * gfla::affine_tiles(H, W) * (int64_t)sizeof(double);
}

int gfla_affine_reg_fwd_f32(const float *flow, void *workspace, float *loss, int64_t B, int64_t H, int64_t W, int k,
                            gfla_stream_t stream) {
  return gfla::affine_fwd<float>(flow, workspace, loss, B, H, W, k, stream);
}
int gfla_affine_reg_fwd_f64(const double *flow, void *workspace, double *loss, int64_t B, int64_t H, int64_t W, int k,
                            gfla_stream_t stream) {
  return gfla::affine_fwd<double>(flow, workspace, loss, B, H, W, k, stream);
}
int gfla_affine_reg_fwd_f16(const uint16_t *flow, void *workspace, float *loss, int64_t B, int64_t H, int64_t W, int k,
                            gfla_stream_t stream) {
  return gfla::affine_fwd<f16_t>(reinterpret_cast<const f16_t *>(flow), workspace, loss, B, H, W, k, stream);
}
int gfla_affine_reg_fwd_bf16(const uint16_t *flow, void *workspace, float *loss, int64_t B, int64_t H, int64_t W, int k,
                             gfla_stream_t stream) {
  return gfla::affine_fwd<bf16_t>(reinterpret_cast<const bf16_t *>(flow), workspace, loss, B, H, W, k, stream);
}

int gfla_affine_reg_bwd_f32(const float *flow, const float *grad_loss, void *workspace, float *grad_flow, int64_t B,
                            int64_t H, int64_t W, int k, gfla_stream_t stream) {
  return gfla::affine_bwd<float>(flow, grad_loss, grad_flow, B, H, W, k, stream);
}
int gfla_affine_reg_bwd_f64(const double *flow, const double *grad_loss, void *workspace, double *grad_flow, int64_t B,
                            int64_t H, int64_t W, int k, gfla_stream_t stream) {
  return gfla::affine_bwd<double>(flow, grad_loss, grad_flow, B, H, W, k, stream);
}
int gfla_affine_reg_bwd_f16(const uint16_t *flow, const float *grad_loss, void *workspace, uint16_t *grad_flow, int64_t B,
                            int64_t H, int64_t W, int k, gfla_stream_t stream) {
  return gfla::affine_bwd<f16_t>(reinterpret_cast<const f16_t *>(flow), grad_loss, reinterpret_cast<f16_t *>(grad_flow), B,
                                 H, W, k, stream);
}
int gfla_affine_reg_bwd_bf16(const uint16_t *flow, const float *grad_loss, void *workspace, uint16_t *grad_flow, int64_t B,
                             int64_t H, int64_t W, int k, gfla_stream_t stream) {
  return gfla::affine_bwd<bf16_t>(reinterpret_cast<const bf16_t *>(flow), grad_loss, reinterpret_cast<bf16_t *>(grad_flow),
                                  B, H, W, k, stream);
}
}
