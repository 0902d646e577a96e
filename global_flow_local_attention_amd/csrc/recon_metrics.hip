// Reconstruction metrics on the device, gfx950 (include/gfla_metrics.h): the generator's output as bytes, and SSIM with a
// uniform and with a Gaussian window, PSNR, L1 and MAE of byte images.
//
// images_to_uint8: a workgroup takes 1024 consecutive pixels of one sample, reads that span of each of the C planes (lanes
// side by side), puts the bytes into LDS interleaved like a pixel, and stores the span of the (B, H, W, C) output like any
// span (store_span): bytes up to the first 16-byte boundary, 16-byte packs, bytes after the last one.
//
// recon_metrics is up to four launches on one stream, the first three independent of each other but for R:
//   pixel sums      grid (chunks, B): a workgroup walks 16 KB pieces of one image pair, 16 bytes per thread and piece, and
//                   leaves sum |d|, sum d d, sum (a + b) as doubles and min / max of pred in the workspace.
//   uniform SSIM    one workgroup per (image, channel, band of kSsimBand output rows, strip of T - (win - 1) output
//                   columns), T = 256 threads, or 1024 for windows over 129.  A thread owns one INPUT column of the strip and
//                   keeps the five window sums of that column over the last `win` rows in registers: the entering row's
//                   byte is added, the leaving one's subtracted, both read from the image (the rows of a band stay in L2,
//                   and the next row's four bytes are fetched before the current row is worked on).  Per output row the five
//                   column sums are prefix-summed across the strip -- a wave scan, the waves' totals through LDS -- and a
//                   window's sum is the difference of two prefixes, in wrapping 32-bit arithmetic, which is exact because
//                   the window's own sum fits 32 bits.  The cost per position does not depend on the window.  S is one
//                   double division of exact integers (but for C1 N^2 and C2 N (N - 1), rounded once on the host).
//   Gaussian SSIM   the same grid with T = 256 and 11 taps: a thread keeps its column's last 11 byte pairs in registers,
//                   weighs the five moments with the taps in order, hands them over through LDS, and the thread of an
//                   output column weighs 11 neighbours.  R comes from the pixel launch's min / max.
//   finish          one wave per image adds the workgroups' partial sums in a fixed order and applies the last formulas.
// Every sum has a fixed order (per thread in row order, then a tree over the workgroup, then a strided sum and a tree over
// the partials), nothing is atomic, and no index depends on the batch: an image's numbers are the same bits anywhere.
#include "gfla_common.h"
#include "span_store.h"

namespace gfla {

constexpr int kU8Pix = 1024;                   // pixels per workgroup of images_to_uint8: 4 KB of bytes at C = 4
constexpr int kPixPiece = 16384;               // bytes of one image a workgroup of the pixel sums takes at a time
constexpr int kPixMaxChunks = 64;              // workgroups per image at most: the partials one finishing wave adds
constexpr int kSsimBand = 32;                  // output rows per workgroup of both SSIM kernels
constexpr int kSsimWide = 129;                 // windows above this run 1024 threads: at least 770 output columns per strip
constexpr int kGaussTaps = GFLA_METRICS_TAPS;
constexpr int64_t kMetMaxSide = 32768;
constexpr int64_t kMetMaxGrid = 2147483647;

template <>
struct Num<uint8_t> {
  static __device__ __forceinline__ uint8_t from(uint8_t v) { return v; }
};

// ---- images_to_uint8 -----------------------------------------------------------------------------------------------
__device__ __forceinline__ uint8_t to_byte(float x, float bytes) {
#pragma clang fp contract(off)
  const float t = ((x + 1.f) / 2.f) * bytes;
  if (!(t >= 0.f)) return 0;                         // negative, or NaN
  if (t >= 256.f) return 255;
  return (uint8_t)(int)t;
}

struct ByteGen {
  const uint8_t *src;
  int at;
  __device__ __forceinline__ void seek(int k) { at = k; }
  __device__ __forceinline__ void jump(int m) { at += m; }
  __device__ __forceinline__ uint8_t next() { return src[at++]; }
  template <int V>
  __device__ __forceinline__ void pack(Pack<uint8_t, V> &q) const {
#pragma unroll
    for (int i = 0; i < V; ++i) q.v[i] = src[at + i];
  }
};

template <typename T>
__global__ __launch_bounds__(kBlock) void images_to_uint8_kernel(const T *__restrict__ x, uint8_t *__restrict__ out, int P,
                                                                 int C, int chunks, float bytes) {
  __shared__ uint8_t staged[kU8Pix * 4];
  const int64_t b = blockIdx.x / chunks;
  const int p0 = (int)(blockIdx.x - b * chunks) * kU8Pix;
  const int npix = min(kU8Pix, P - p0);
  for (int c = 0; c < C; ++c) {
    const T *plane = x + (b * C + c) * (int64_t)P + p0;
    for (int i = threadIdx.x; i < npix; i += kBlock) staged[i * C + c] = to_byte(Num<T>::ld(plane + i), bytes);
  }
  __syncthreads();
  ByteGen gen;
  gen.src = staged;
  store_span(out + (b * P + p0) * C, npix * C, gen);
}

template <typename T>
static int images_to_uint8(const T *x, uint8_t *out, int64_t B, int64_t C, int64_t H, int64_t W, double bytes,
                           gfla_stream_t stream) {
  if (x == nullptr || out == nullptr) return GFLA_ERR_NULL_POINTER;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !__builtin_isfinite((float)bytes)) return GFLA_ERR_BAD_SHAPE;
  if (C > 4 || H > kMetMaxSide || W > kMetMaxSide || H * W > kMetMaxGrid / C) return GFLA_ERR_UNSUPPORTED;
  const int64_t chunks = ceil_div(H * W, kU8Pix);
  if (B > kMetMaxGrid / chunks) return GFLA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(images_to_uint8_kernel<T>, dim3((unsigned)(B * chunks)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), x, out, (int)(H * W), (int)C, (int)chunks, (float)bytes);
  return launch_status();
}

// ---- sums in a fixed order -----------------------------------------------------------------------------------------
// the sum of v over the T threads of a workgroup, a tree through LDS: the same order in every call (all threads call it)
template <int T>
__device__ __forceinline__ double block_sum(double v, double *tree) {
  const int tid = threadIdx.x;
  __syncthreads();                                   // whoever read `tree` last is done
  tree[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = T / 2; s > 0; s >>= 1) {
    if (tid < s) tree[tid] = tree[tid] + tree[tid + s];
    __syncthreads();
  }
  return tree[0];
}

// the sum of n doubles `stride` apart by one wave: lane l adds l, l + 64, ... in turn, then a tree over the lanes
__device__ __forceinline__ double wave_sum_strided(const double *p, int64_t n, int64_t stride) {
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 64) v = v + p[i * stride];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = v + __shfl_down(v, d, 64);
  return __shfl(v, 0, 64);
}

// ---- the pixel sums ------------------------------------------------------------------------------------------------
struct MetricsPlan {
  int64_t chunks;                                    // pixel-sum workgroups per image
  int64_t strips_u, bands_u, strips_g, bands_g;      // per (image, channel) of the two SSIM kernels; 0: not asked for
  int threads_u;
  int64_t pix_at, ssim_at, gauss_at, doubles;        // offsets into the workspace, in doubles
};

// 16 bytes at p, or the `count` < 16 there are: dwords where p allows them (the same branch for the whole launch)
__device__ __forceinline__ void load_bytes(const uint8_t *p, int count, uint32_t (&w)[4]) {
  if (count == 16 && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = reinterpret_cast<const uint32_t *>(p)[i];
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < count) w[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
}

__device__ __forceinline__ double unit_value(uint32_t byte) {
#pragma clang fp contract(off)
  return (double)((float)byte / 255.f);
}

__global__ __launch_bounds__(kBlock) void pixel_sums_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt,
                                                            double *__restrict__ partial, int n, int chunks) {
#pragma clang fp contract(off)
  __shared__ double tree[kBlock];
  __shared__ uint32_t lows[kBlock], highs[kBlock];
  const int64_t b = blockIdx.y;
  const uint8_t *p = pred + b * n, *g = gt + b * n;
  const int tid = threadIdx.x;
  double s_abs = 0.0, s_sq = 0.0, s_sum = 0.0;
  uint32_t low = 255, high = 0;
  for (int64_t piece = blockIdx.x; piece * kPixPiece < n; piece += chunks) {
    for (int k = 0; k < kPixPiece / (16 * kBlock); ++k) {
      const int64_t at = piece * kPixPiece + (k * kBlock + tid) * 16;
      if (at >= n) break;
      const int count = (int)min((int64_t)16, n - at);
      uint32_t wp[4], wg[4];
      load_bytes(p + at, count, wp);
      load_bytes(g + at, count, wg);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (i >= count) break;
        const uint32_t y = (wp[i >> 2] >> (8 * (i & 3))) & 255u, x = (wg[i >> 2] >> (8 * (i & 3))) & 255u;
        const double a = unit_value(x), v = unit_value(y), d = a - v;
        s_abs = s_abs + fabs(d);
        s_sq = s_sq + d * d;
        s_sum = s_sum + (a + v);
        low = min(low, y);
        high = max(high, y);
      }
    }
  }
  double *mine = partial + (b * chunks + blockIdx.x) * 4;
  const double t_abs = block_sum<kBlock>(s_abs, tree), t_sq = block_sum<kBlock>(s_sq, tree);
  const double t_sum = block_sum<kBlock>(s_sum, tree);
  lows[tid] = low;
  highs[tid] = high;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (tid < s) {
      lows[tid] = min(lows[tid], lows[tid + s]);
      highs[tid] = max(highs[tid], highs[tid + s]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    mine[0] = t_abs;
    mine[1] = t_sq;
    mine[2] = t_sum;
    uint32_t *mm = reinterpret_cast<uint32_t *>(mine + 3);
    mm[0] = lows[0];
    mm[1] = highs[0];
  }
}

// ---- S -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double ssim_value(double ux, double uy, double vx, double vy, double vxy, double c1, double c2) {
#pragma clang fp contract(off)
  const double a1 = 2.0 * ux * uy + c1, a2 = 2.0 * vxy + c2;
  const double b1 = ux * ux + uy * uy + c1, b2 = vx + vy + c2;
  return (a1 * a2) / (b1 * b2);
}

// where the workgroup's tile lies: image b, channel c, output rows y0 .. y0 + rows - 1, output columns x0 .. x0 + cols - 1
struct Tile {
  int64_t b;
  int c, y0, rows, x0, cols;
};

__device__ __forceinline__ Tile tile_of(int H, int W, int C, int win, int strips, int bands, int strip_width) {
  Tile t;
  int64_t at = blockIdx.x;
  const int strip = (int)(at % strips);
  at /= strips;
  const int band = (int)(at % bands);
  at /= bands;
  t.c = (int)(at % C);
  t.b = at / C;
  t.y0 = band * kSsimBand;
  t.rows = min(kSsimBand, H - win + 1 - t.y0);
  t.x0 = strip * strip_width;
  t.cols = min(strip_width, W - win + 1 - t.x0);
  return t;
}

// ---- SSIM with a uniform window ------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wave_scan(uint32_t v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t below = __shfl_up(v, d, 64);
    if (lane >= d) v += below;
  }
  return v;
}

template <int T>
__global__ __launch_bounds__(T) void ssim_uniform_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt,
                                                         double *__restrict__ partial, int H, int W, int C, int win,
                                                         int strips, int bands, double c1, double c2) {
#pragma clang fp contract(off)
  constexpr int kWaves = T / 64;
  __shared__ uint32_t totals[5][kWaves];
  __shared__ uint32_t prefix[5][T + 1];              // prefix[k][i]: the sum of the first i columns' k-th sums
  __shared__ double tree[T];
  const Tile t = tile_of(H, W, C, win, strips, bands, T - (win - 1));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool has_column = tid < t.cols + win - 1, has_output = tid < t.cols;
  const int64_t image = t.b * H * W * C + t.c;
  // byte (row, this thread's column) of the channel; a thread without a column reads the strip's first one and drops it
  const int64_t column = image + (int64_t)(t.x0 + (has_column ? tid : 0)) * C;
  const int64_t row_step = (int64_t)W * C;
  const uint8_t *px = gt + column, *py = pred + column;
  if (tid < 5) prefix[tid][0] = 0;
  uint32_t sum[5] = {0, 0, 0, 0, 0};                 // x, y, x x, y y, x y over the rows in the window
  const int64_t N = (int64_t)win * win;
  const int steps = t.rows + win - 1;
  double acc = 0.0;
  uint32_t nx = px[t.y0 * row_step], ny = py[t.y0 * row_step], ox = 0, oy = 0;
  for (int r = 0; r < steps; ++r) {
    const uint32_t x = nx, y = ny, lx = ox, ly = oy;
    if (r + 1 < steps) {                             // the next step's bytes, in flight while this one is worked on
      const int64_t next = (t.y0 + r + 1) * row_step;
      nx = px[next];
      ny = py[next];
      if (r + 1 >= win) {
        ox = px[next - win * row_step];
        oy = py[next - win * row_step];
      }
    }
    if (has_column) {
      sum[0] += x - lx;
      sum[1] += y - ly;
      sum[2] += x * x - lx * lx;
      sum[3] += y * y - ly * ly;
      sum[4] += x * y - lx * ly;
    }
    if (r < win - 1) continue;                       // uniform: the window is not full yet
    uint32_t incl[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      incl[k] = wave_scan(sum[k], lane);
      if (lane == 63) totals[k][wave] = incl[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      for (int w = 0; w < wave; ++w) incl[k] += totals[k][w];
      prefix[k][tid + 1] = incl[k];
    }
    __syncthreads();
    if (has_output) {
      int64_t s[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) s[k] = (int64_t)(uint32_t)(prefix[k][tid + win] - prefix[k][tid]);
      const double sx = (double)s[0], sy = (double)s[1];
      const double nxx = (double)(N * s[2] - s[0] * s[0]), nyy = (double)(N * s[3] - s[1] * s[1]);
      const double nxy = (double)(N * s[4] - s[0] * s[1]);
      // ux, uy scaled by N and the covariances by N (N - 1), c1 and c2 with them: exact integers but for c1, c2
      acc = acc + ssim_value(sx, sy, nxx, nyy, nxy, c1, c2);
    }
  }
  const double total = block_sum<T>(acc, tree);
  if (tid == 0) partial[blockIdx.x] = total;
}

// ---- SSIM with Gaussian weights ------------------------------------------------------------------------------------
struct GaussTaps {
  double t[kGaussTaps];
};

__global__ __launch_bounds__(kBlock) void ssim_gauss_kernel(const uint8_t *__restrict__ pred, const uint8_t *__restrict__ gt,
                                                            const double *__restrict__ pixel_partial,
                                                            double *__restrict__ partial, int H, int W, int C, int strips,
                                                            int bands, int chunks, GaussTaps taps) {
#pragma clang fp contract(off)
  constexpr int win = kGaussTaps;
  __shared__ double moments[5][kBlock];
  __shared__ double tree[kBlock];
  const Tile t = tile_of(H, W, C, win, strips, bands, kBlock - (win - 1));
  const int tid = threadIdx.x;
  const bool has_column = tid < t.cols + win - 1, has_output = tid < t.cols;
  uint32_t low = 255, high = 0;                      // of the whole prediction, from the pixel launch
  for (int j = 0; j < chunks; ++j) {
    const uint32_t *mm = reinterpret_cast<const uint32_t *>(pixel_partial + (t.b * chunks + j) * 4 + 3);
    low = min(low, mm[0]);
    high = max(high, mm[1]);
  }
  const double R = (double)(int)(high - low);
  const double c1 = (0.01 * R) * (0.01 * R), c2 = (0.03 * R) * (0.03 * R);
  const int64_t image = t.b * H * W * C + t.c;
  const int64_t column = image + (int64_t)(t.x0 + (has_column ? tid : 0)) * C;
  const int64_t row_step = (int64_t)W * C;
  const uint8_t *px = gt + column, *py = pred + column;
  uint32_t ring[win];                                // x | y << 8 of the last 11 rows, oldest first
#pragma unroll
  for (int i = 0; i < win; ++i) ring[i] = 0;
  const int steps = t.rows + win - 1;
  double acc = 0.0;
  uint32_t next_pair = (uint32_t)px[t.y0 * row_step] | (uint32_t)py[t.y0 * row_step] << 8;
  for (int r = 0; r < steps; ++r) {
#pragma unroll
    for (int i = 0; i + 1 < win; ++i) ring[i] = ring[i + 1];
    ring[win - 1] = next_pair;
    if (r + 1 < steps) {
      const int64_t next = (t.y0 + r + 1) * row_step;
      next_pair = (uint32_t)px[next] | (uint32_t)py[next] << 8;
    }
    if (r < win - 1) continue;
    double m[5];
#pragma unroll
    for (int i = 0; i < win; ++i) {
      const uint32_t x = ring[i] & 255u, y = ring[i] >> 8;
      const double v[5] = {(double)x, (double)y, (double)(x * x), (double)(y * y), (double)(x * y)};
#pragma unroll
      for (int k = 0; k < 5; ++k) m[k] = i == 0 ? taps.t[0] * v[k] : m[k] + taps.t[i] * v[k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) moments[k][tid] = m[k];
    __syncthreads();
    if (has_output) {
      double u[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        u[k] = taps.t[0] * moments[k][tid];
#pragma unroll
        for (int i = 1; i < win; ++i) u[k] = u[k] + taps.t[i] * moments[k][tid + i];
      }
      const double vx = u[2] - u[0] * u[0], vy = u[3] - u[1] * u[1], vxy = u[4] - u[0] * u[1];
      acc = acc + ssim_value(u[0], u[1], vx, vy, vxy, c1, c2);
    }
    __syncthreads();
  }
  const double total = block_sum<kBlock>(acc, tree);
  if (tid == 0) partial[blockIdx.x] = total;
}

// ---- the last formulas ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void metrics_finish_kernel(const double *__restrict__ ws, double *__restrict__ out, int B,
                                                            int H, int W, int C, int win, int flags, MetricsPlan plan) {
#pragma clang fp contract(off)
  const int64_t b = blockIdx.x;
  if (flags & 1) {
    const int64_t per = plan.strips_u * plan.bands_u;
    const double positions = (double)((int64_t)(H - win + 1) * (W - win + 1));
    double mean = 0.0;
    for (int c = 0; c < C; ++c) mean = mean + wave_sum_strided(ws + plan.ssim_at + (b * C + c) * per, per, 1) / positions;
    if (threadIdx.x == 0) out[b] = mean / (double)C;
  }
  if (flags & 2) {
    const int64_t per = plan.strips_g * plan.bands_g;
    const double positions = (double)((int64_t)(H - kGaussTaps + 1) * (W - kGaussTaps + 1));
    double mean = 0.0;
    for (int c = 0; c < C; ++c) mean = mean + wave_sum_strided(ws + plan.gauss_at + (b * C + c) * per, per, 1) / positions;
    if (threadIdx.x == 0) out[(int64_t)B + b] = mean / (double)C;
  }
  if (flags & 4) {
    const double *mine = ws + plan.pix_at + b * plan.chunks * 4;
    const double n = (double)((int64_t)H * W * C);
    const double s_abs = wave_sum_strided(mine, plan.chunks, 4), s_sq = wave_sum_strided(mine + 1, plan.chunks, 4);
    const double s_sum = wave_sum_strided(mine + 2, plan.chunks, 4);
    if (threadIdx.x == 0) {
      out[2 * (int64_t)B + b] = 10.0 * log10(1.0 / (s_sq / n));
      out[3 * (int64_t)B + b] = s_abs / n;
      out[4 * (int64_t)B + b] = s_abs / s_sum;
    }
  }
}

// ---- the host side -------------------------------------------------------------------------------------------------
static int uniform_threads(int64_t win) { return win > kSsimWide ? 1024 : kBlock; }

// what is launched, and where its partial sums go; flags as in gfla_recon_metrics
static int metrics_plan(int64_t B, int64_t H, int64_t W, int64_t C, int64_t win, int flags, MetricsPlan *plan) {
  if (B <= 0 || H <= 0 || W <= 0 || C < 1 || C > 4 || flags < 1 || flags > 7) return GFLA_ERR_BAD_SHAPE;
  if ((flags & 1) && (win < 3 || win > 255 || win % 2 == 0 || H < win || W < win)) return GFLA_ERR_BAD_SHAPE;
  if ((flags & 2) && (H < kGaussTaps || W < kGaussTaps)) return GFLA_ERR_BAD_SHAPE;
  if (H > kMetMaxSide || W > kMetMaxSide || H * W > kMetMaxGrid / C) return GFLA_ERR_UNSUPPORTED;
  MetricsPlan p = {};
  p.chunks = min(ceil_div(H * W * C, kPixPiece), (int64_t)kPixMaxChunks);
  p.threads_u = uniform_threads(win);
  if (flags & 1) {
    p.strips_u = ceil_div(W - win + 1, p.threads_u - (win - 1));
    p.bands_u = ceil_div(H - win + 1, kSsimBand);
  }
  if (flags & 2) {
    p.strips_g = ceil_div(W - kGaussTaps + 1, kBlock - (kGaussTaps - 1));
    p.bands_g = ceil_div(H - kGaussTaps + 1, kSsimBand);
  }
  // B <= 65535 images per launch of the pixel sums (grid y), and every SSIM grid within 2^31 - 1
  if (B > 65535 || B * C > kMetMaxGrid / max(max(p.strips_u * p.bands_u, p.strips_g * p.bands_g), (int64_t)1))
    return GFLA_ERR_UNSUPPORTED;
  p.pix_at = 0;
  p.ssim_at = p.pix_at + B * p.chunks * 4;
  p.gauss_at = p.ssim_at + B * C * p.strips_u * p.bands_u;
  p.doubles = p.gauss_at + B * C * p.strips_g * p.bands_g;
  *plan = p;
  return GFLA_OK;
}

static int recon_metrics(const uint8_t *pred, const uint8_t *gt, double *out, void *workspace, int64_t B, int64_t H,
                         int64_t W, int64_t C, int64_t win, int flags, const double *taps, gfla_stream_t stream) {
  if (pred == nullptr || gt == nullptr || out == nullptr || workspace == nullptr) return GFLA_ERR_NULL_POINTER;
  if (flags >= 1 && flags <= 7 && (flags & 2) && taps == nullptr) return GFLA_ERR_NULL_POINTER;
  MetricsPlan plan;
  const int status = metrics_plan(B, H, W, C, win, flags, &plan);
  if (status != GFLA_OK) return status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  double *ws = static_cast<double *>(workspace);
  if (flags & 6)                                     // the Gaussian window needs the prediction's range
    hipLaunchKernelGGL(pixel_sums_kernel, dim3((unsigned)plan.chunks, (unsigned)B), dim3(kBlock), 0, s, pred, gt,
                       ws + plan.pix_at, (int)(H * W * C), (int)plan.chunks);
  if (flags & 1) {
    const double N = (double)(win * win);
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double c1 = C1 * (N * N), c2 = C2 * (N * (N - 1.0));
    const dim3 grid((unsigned)(B * C * plan.strips_u * plan.bands_u));
    if (plan.threads_u == 1024)
      hipLaunchKernelGGL(ssim_uniform_kernel<1024>, grid, dim3(1024), 0, s, pred, gt, ws + plan.ssim_at, (int)H, (int)W,
                         (int)C, (int)win, (int)plan.strips_u, (int)plan.bands_u, c1, c2);
    else
      hipLaunchKernelGGL(ssim_uniform_kernel<kBlock>, grid, dim3(kBlock), 0, s, pred, gt, ws + plan.ssim_at, (int)H, (int)W,
                         (int)C, (int)win, (int)plan.strips_u, (int)plan.bands_u, c1, c2);
  }
  if (flags & 2) {
    GaussTaps t;
    for (int i = 0; i < kGaussTaps; ++i) t.t[i] = taps[i];
    hipLaunchKernelGGL(ssim_gauss_kernel, dim3((unsigned)(B * C * plan.strips_g * plan.bands_g)), dim3(kBlock), 0, s, pred,
                       gt, ws + plan.pix_at, ws + plan.gauss_at, (int)H, (int)W, (int)C, (int)plan.strips_g,
                       (int)plan.bands_g, (int)plan.chunks, t);
  }
  hipLaunchKernelGGL(metrics_finish_kernel, dim3((unsigned)B), dim3(64), 0, s, ws, out, (int)B, (int)H, (int)W, (int)C,
                     (int)win, flags, plan);
  return launch_status();
}

}  // namespace gfla

using namespace gfla;

#define GFLA_DEF_TO_UINT8(SFX, S)                                                                                        \
  extern "C" int gfla_images_to_uint8_##SFX(const S *x, uint8_t *out, int64_t B, int64_t C, int64_t H, int64_t W,        \
                                            double bytes, gfla_stream_t stream) {                                        \
    return images_to_uint8(as<elem_##SFX>(x), out, B, C, H, W, bytes, stream);                                           \
  }
GFLA_DEF_TO_UINT8(f32, float)
GFLA_DEF_TO_UINT8(f16, uint16_t)
GFLA_DEF_TO_UINT8(bf16, uint16_t)
#undef GFLA_DEF_TO_UINT8

extern "C" int64_t gfla_recon_metrics_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t win_size,
                                                      int flags) {
  MetricsPlan plan;
  const int status = metrics_plan(B, H, W, C, win_size, flags, &plan);
  return status != GFLA_OK ? status : plan.doubles * (int64_t)sizeof(double);
}

extern "C" int gfla_recon_metrics(const uint8_t *pred, const uint8_t *gt, double *out, void *workspace, int64_t B, int64_t H,
                                  int64_t W, int64_t C, int64_t win_size, int flags, const double *taps,
                                  gfla_stream_t stream) {
  return recon_metrics(pred, gt, out, workspace, B, H, W, C, win_size, flags, taps, stream);
}

extern "C" int gfla_recon_metrics_geometry(int64_t win_size, int64_t *out) {
  if (out == nullptr) return GFLA_ERR_NULL_POINTER;
  if (win_size < 3 || win_size > 255 || win_size % 2 == 0) return GFLA_ERR_BAD_SHAPE;
  out[0] = uniform_threads(win_size) - (win_size - 1);
  out[1] = kSsimBand;
  out[2] = kBlock - (kGaussTaps - 1);
  out[3] = kSsimBand;
  out[4] = kPixPiece;
  return GFLA_OK;
}
