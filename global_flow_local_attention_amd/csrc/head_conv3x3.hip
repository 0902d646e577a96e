// Narrow 3x3 convolution heads (Cout <= 8) with fused surroundings, forward and backward, gfx950.
//
//   a   = pre_act ? leaky_relu(x, slope) : x                      (x == 0 takes the slope side in the backward)
//   s   = conv3x3(pad(a), w) + bias                               pad: zeros | reflect (one pixel), stride 1, output H x W
//   y_c = post_c(s_c),  post_c in {identity, tanh, sigmoid}       two 8-bit masks, one bit per OUTPUT channel
// Channels [0, C0) go to y0 (B,C0,H,W) and [C0, Cout) to y1 (B,Cout-C0,H,W): a flow field and its mask come out of one
// launch as two contiguous tensors.  With so few output channels the op is one streaming pass over x: 9 Cin Cout MACs per
// pixel against Cin loaded values, on the vector ALUs (a 32-wide MFMA tile would be 3/32 full).  Weights are uniform
// over a wave and are read through uniform (scalar) loads; sums are float32, a 16-bit result is rounded once.
//
// Forward (hc_fwd_kernel).  A workgroup owns a tile of TW x TH pixels with its one-pixel halo and walks Cin in chunks of
// four channels.  The tile is staged to LDS as float32 with the pre-activation applied and the padding resolved (reflect
// is an index map, -1 -> 1, H -> H-2; a zero-padded position is a stored zero): neither the activated nor the padded map
// exists in memory.  Which element of a plane each thread stages is the same for every channel and is worked out once;
// a chunk travels through registers, all its loads issued before the first is used and the next chunk's loads in flight
// while this one is multiplied.
// A thread owns 4 x 2 pixels: per channel it reads 4 rows x 6 columns from LDS (one 16-byte and one 8-byte read per row)
// for 72 Cout FMAs, and keeps its 8 Cout sums in registers.
//
// Backward, d x (hc_bwd_x_kernel), owner-computes, no atomics.  g'_c = g_c post_c'(y_c) from the saved outputs is staged
// once per tile (with halo, zero outside the image).  The thread of a strip of PX pixels in one row holds, for every
// output channel, the three rows x (PX + 2) columns of g' that reach it -- they are the same for every input channel --
// and then walks its share of Cin: 9 Cout PX FMAs, times the pre-activation's slope at the stored x, one store.
// Reflect padding: output q reads the padded position q + d, which is the image position m(q + d).  The positions that
// map onto row p are p itself, the ring row -1 when p == 1 and the ring row H when p == H - 2 (for H == 2 both ring rows
// fold onto opposite rows); ring row -1 is reached from output row 0 with d = -1 only, ring row H from row H - 1 with
// d = +1 only.  So the row slot of tap d = -1 (g' row p + 1) also takes g' row 0 when p == 1, and the slot of d = +1
// takes row H - 1 when p == H - 2; the slots belong to one pixel row (PY = 1), so this is done in registers once.
// Columns likewise, per pixel, as two extra FMAs per row slot for the pixels in columns 1 and W - 2.
//
// Backward, d w and d bias (hc_bwd_w_kernel + hc_bwd_w_sum_kernel).  dW[co][ci][tap] = sum over pixels of
// g'_co[p] a_ci[p + tap].  Lanes are INPUT CHANNELS: a thread owns the 9 Cout sums of its channel (and the Cout bias
// sums), a wave walks one output row of a stage of 4 rows x 32 columns with a sliding 3 x 3 window over a (staged to LDS
// as [channel][6 x 34], pitch 205: conflict-free for lanes = channels, a recomputed from x with the padding), g' is
// read as a wave-wide broadcast.  There is no cross-lane reduction at all; the four waves of a workgroup are added in
// wave order once, at the end of the workgroup's slab (a band of rows of one image).  Per-slab partials go to the
// workspace and a second launch adds them in a fixed order (16 segments of slabs, then the segments): no atomics, no
// memset, bit-identical from call to call.
#include <algorithm>

#include "gfla_common.h"

namespace gfla {

constexpr int kHcMaxCout = 8;
constexpr int kHcChunk = 4;        // forward: input channels staged per round
constexpr int kHcStage = 11;       // forward / d x: tile elements (halo included) a thread stages per channel, at most
constexpr int kHcWLanes = 64;      // d w: input channels per workgroup (one per lane)
constexpr int kHcWRows = 4, kHcWCols = 32;                                   // d w: output pixels per stage
constexpr int kHcWPlane = (kHcWRows + 2) * (kHcWCols + 2);                   // 204 staged values per channel
constexpr int kHcWPitch = kHcWPlane + 1;                                     // odd: lanes = channels hit 64 banks
constexpr int64_t kHcWantSlabs = 1024;

// image offset of padded position (gy, gx), or -1 for a zero (zero padding, or beyond the one-pixel ring)
__device__ __forceinline__ int hc_src(int gy, int gx, int H, int W, int reflect) {
  if (reflect) {
    gy = gy < 0 ? -gy : gy;
    gy = gy >= H ? 2 * H - 2 - gy : gy;
    gx = gx < 0 ? -gx : gx;
    gx = gx >= W ? 2 * W - 2 - gx : gx;
  }
  return (gy < 0 || gy >= H || gx < 0 || gx >= W) ? -1 : gy * W + gx;
}

__device__ __forceinline__ int hc_post_mode(int co, unsigned tanh_mask, unsigned sig_mask) {
  return ((tanh_mask >> co) & 1u) ? 1 : ((sig_mask >> co) & 1u) ? 2 : 0;
}

// upstream gradient through the post-activation, from the saved output
template <typename T>
__device__ __forceinline__ float hc_gprime(const T *g, const T *y, int64_t at, int mode) {
  const float gv = Num<T>::ld(g + at);
  if (mode == 0) return gv;
  const float yv = Num<T>::ld(y + at);
  return mode == 1 ? gv * (1.0f - yv * yv) : gv * (yv * (1.0f - yv));
}

// N contiguous values of a row: one vector access where the host found every strip whole and aligned
template <typename T, int N>
__device__ __forceinline__ void hc_load_strip(const T *p, bool vec, int valid, float (&v)[N]) {
  if (vec) {
    const Pack<T, N> pk = *reinterpret_cast<const Pack<T, N> *>(p);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = Num<T>::ld(&pk.v[i]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = i < valid ? Num<T>::ld(p + i) : 0.0f;
  }
}

template <typename T, int N>
__device__ __forceinline__ void hc_store_strip(T *p, bool vec, int valid, const float (&v)[N]) {
  if (vec) {
    Pack<T, N> pk;
#pragma unroll
    for (int i = 0; i < N; ++i) pk.v[i] = Num<T>::from(v[i]);
    *reinterpret_cast<Pack<T, N> *>(p) = pk;
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i)
      if (i < valid) p[i] = Num<T>::from(v[i]);
  }
}

struct HcGeo {
  int H, W, Cin, C0;
  int tw, lg, th, ntx, nty;     // tile width, log2 of the strips per tile row, tile height, tiles per plane
  int reflect, pre_act;
  float slope;
  unsigned tanh_mask, sig_mask;
};

// ---- forward ---------------------------------------------------------------------------------------------------------
template <typename T, int COUT>
__global__ void __launch_bounds__(256)
hc_fwd_kernel(const T *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, T *__restrict__ y0,
              T *__restrict__ y1, HcGeo g, int vec) {
  extern __shared__ float4 hc_lds4[];
  float *lds = reinterpret_cast<float *>(hc_lds4);
  const int tid = threadIdx.x, nth = blockDim.x;
  int blk = blockIdx.x;
  const int txi = blk % g.ntx;
  blk /= g.ntx;
  const int tyi = blk % g.nty;
  const int b = blk / g.nty;
  const int H = g.H, W = g.W, HW = H * W, Cin = g.Cin;
  const int x0 = txi * g.tw, r0 = tyi * g.th;
  const int rows = g.th + 2, cols = g.tw + 2, pitch = g.tw + 4, plane = rows * pitch;

  int goff[kHcStage], loff[kHcStage];
#pragma unroll
  for (int k = 0; k < kHcStage; ++k) {
    const int e = tid + k * nth;
    const int r = e / cols, c = e - r * cols;
    loff[k] = e < rows * cols ? r * pitch + c : -1;
    goff[k] = hc_src(r0 - 1 + r, x0 - 1 + c, H, W, g.reflect);
  }
  const int tx = tid & ((1 << g.lg) - 1), ty = tid >> g.lg;
  float acc[COUT][2][4];
#pragma unroll
  for (int co = 0; co < COUT; ++co)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[co][i >> 2][i & 3] = 0.0f;

  const T *xb = x + (int64_t)b * Cin * HW;
  // the chunk's values travel through registers: every load of a chunk is issued before the first is used, and the next
  // chunk's loads are in flight while this one is multiplied.  Addresses are clamped instead of branched around (a zero
  // position reads element 0, a channel beyond Cin reads the last one) and the value is chosen afterwards.
  T v[kHcStage][kHcChunk];
#pragma unroll
  for (int k = 0; k < kHcStage; ++k)
#pragma unroll
    for (int c = 0; c < kHcChunk; ++c) v[k][c] = xb[(int64_t)min(c, Cin - 1) * HW + max(goff[k], 0)];
  for (int ci0 = 0; ci0 < Cin; ci0 += kHcChunk) {
    const int cn = min(kHcChunk, Cin - ci0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kHcStage; ++k) {
      if (loff[k] < 0) continue;
#pragma unroll
      for (int c = 0; c < kHcChunk; ++c) {
        float a = goff[k] >= 0 ? Num<T>::ld(&v[k][c]) : 0.0f;
        if (g.pre_act) a = a > 0.0f ? a : a * g.slope;
        lds[c * plane + loff[k]] = a;
      }
    }
    __syncthreads();
    if (ci0 + kHcChunk < Cin) {
#pragma unroll
      for (int k = 0; k < kHcStage; ++k)
#pragma unroll
        for (int c = 0; c < kHcChunk; ++c)
          v[k][c] = xb[(int64_t)min(ci0 + kHcChunk + c, Cin - 1) * HW + max(goff[k], 0)];
    }
    for (int c = 0; c < cn; ++c) {
      const float *t = lds + c * plane + (2 * ty) * pitch + 4 * tx;
      float a[4][6];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 p = *reinterpret_cast<const float4 *>(t + j * pitch);
        const float2 q = *reinterpret_cast<const float2 *>(t + j * pitch + 4);
        a[j][0] = p.x, a[j][1] = p.y, a[j][2] = p.z, a[j][3] = p.w, a[j][4] = q.x, a[j][5] = q.y;
      }
#pragma unroll
      for (int co = 0; co < COUT; ++co) {
        const float *wp = w + ((int64_t)co * Cin + (ci0 + c)) * 9;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float wv = wp[ky * 3 + kx];
#pragma unroll
            for (int py = 0; py < 2; ++py)
#pragma unroll
              for (int px = 0; px < 4; ++px) acc[co][py][px] = fmaf(wv, a[py + ky][px + kx], acc[co][py][px]);
          }
      }
    }
  }

  const int gx = x0 + 4 * tx;
  if (gx >= W) return;
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    const float bv = bias ? bias[co] : 0.0f;
    const int mode = hc_post_mode(co, g.tanh_mask, g.sig_mask);
    const bool first = co < g.C0;
    T *dst = (first ? y0 + ((int64_t)b * g.C0 + co) * HW : y1 + ((int64_t)b * (COUT - g.C0) + (co - g.C0)) * HW);
#pragma unroll
    for (int py = 0; py < 2; ++py) {
      const int gy = r0 + 2 * ty + py;
      if (gy >= H) continue;
      float v[4];
#pragma unroll
      for (int px = 0; px < 4; ++px) {
        const float s = acc[co][py][px] + bv;
        v[px] = mode == 0 ? s : mode == 1 ? tanhf(s) : 1.0f / (1.0f + expf(-s));
      }
      hc_store_strip<T, 4>(dst + (int64_t)gy * W + gx, vec != 0, W - gx, v);
    }
  }
}

// ---- backward: d x ---------------------------------------------------------------------------------------------------
template <typename T, int COUT, int PX>
__global__ void __launch_bounds__(256)
hc_bwd_x_kernel(const T *__restrict__ x, const float *__restrict__ w, const T *__restrict__ y0, const T *__restrict__ y1,
                const T *__restrict__ g0, const T *__restrict__ g1, T *__restrict__ dx, HcGeo g, int ci_per, int vec) {
  extern __shared__ float4 hc_lds4[];
  float *lds = reinterpret_cast<float *>(hc_lds4);
  const int tid = threadIdx.x, nth = blockDim.x;
  int blk = blockIdx.x;
  const int txi = blk % g.ntx;
  blk /= g.ntx;
  const int tyi = blk % g.nty;
  const int b = blk / g.nty;
  const int H = g.H, W = g.W, HW = H * W, Cin = g.Cin;
  const int x0 = txi * g.tw, r0 = tyi * g.th;
  const int rows = g.th + 2, cols = g.tw + 2, plane = rows * cols;

  // g' of the tile and its halo, zero outside the image (whatever the padding mode: the ring holds no output)
#pragma unroll
  for (int k = 0; k < kHcStage; ++k) {
    const int e = tid + k * nth;
    if (e >= plane) break;
    const int r = e / cols, c = e - r * cols;
    const int at = hc_src(r0 - 1 + r, x0 - 1 + c, H, W, 0);
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      const bool first = co < g.C0;
      const T *gp = first ? g0 : g1;
      const T *yp = first ? y0 : y1;
      const int64_t base = first ? ((int64_t)b * g.C0 + co) * HW : ((int64_t)b * (COUT - g.C0) + (co - g.C0)) * HW;
      float v = 0.0f;
      if (gp && at >= 0) v = hc_gprime<T>(gp, yp, base + at, hc_post_mode(co, g.tanh_mask, g.sig_mask));
      lds[co * plane + e] = v;
    }
  }
  __syncthreads();

  const int tx = tid & ((1 << g.lg) - 1), ty = tid >> g.lg;
  const int gx = x0 + PX * tx, gy = r0 + ty;
  if (gx >= W || gy >= H) return;
  // S[co][ky][i]: the row of g' that tap row ky reaches (ky = 0: row gy + 1, ky = 2: row gy - 1), columns gx - 1 + i
  float S[COUT][3][PX + 2];
#pragma unroll
  for (int co = 0; co < COUT; ++co)
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int i = 0; i < PX + 2; ++i) S[co][ky][i] = lds[co * plane + (ty + 2 - ky) * cols + PX * tx + i];
  if (g.reflect) {
    if (gy == 1) {          // ring row -1: output row 0 through tap row 0
#pragma unroll
      for (int co = 0; co < COUT; ++co)
#pragma unroll
        for (int i = 0; i < PX + 2; ++i) S[co][0][i] += lds[co * plane + ty * cols + PX * tx + i];
    }
    if (gy == H - 2) {      // ring row H: output row H - 1 through tap row 2
#pragma unroll
      for (int co = 0; co < COUT; ++co)
#pragma unroll
        for (int i = 0; i < PX + 2; ++i) S[co][2][i] += lds[co * plane + (ty + 2) * cols + PX * tx + i];
    }
  }
  const bool edge = g.reflect && (gx <= 1 || (gx <= W - 2 && W - 2 < gx + PX));
  const int ci_lo = blockIdx.y * ci_per, ci_hi = min(Cin, ci_lo + ci_per);
  const int64_t row = (int64_t)gy * W + gx;
  for (int ci = ci_lo; ci < ci_hi; ++ci) {
    float acc[PX];
#pragma unroll
    for (int p = 0; p < PX; ++p) acc[p] = 0.0f;
#pragma unroll
    for (int co = 0; co < COUT; ++co) {
      const float *wp = w + ((int64_t)co * Cin + ci) * 9;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const float wv = wp[ky * 3 + kx];
#pragma unroll
          for (int p = 0; p < PX; ++p) acc[p] = fmaf(wv, S[co][ky][p + 2 - kx], acc[p]);
        }
    }
    if (edge) {
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        if (gx + p == 1) {          // ring column -1: output column 0 through tap column 0
#pragma unroll
          for (int co = 0; co < COUT; ++co)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) acc[p] = fmaf(w[((int64_t)co * Cin + ci) * 9 + ky * 3], S[co][ky][p], acc[p]);
        }
        if (gx + p == W - 2) {      // ring column W: output column W - 1 through tap column 2
#pragma unroll
          for (int co = 0; co < COUT; ++co)
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
              acc[p] = fmaf(w[((int64_t)co * Cin + ci) * 9 + ky * 3 + 2], S[co][ky][p + 2], acc[p]);
        }
      }
    }
    const int64_t at = ((int64_t)b * Cin + ci) * HW + row;
    if (g.pre_act) {
      float xv[PX];
      hc_load_strip<T, PX>(x + at, vec != 0, W - gx, xv);
#pragma unroll
      for (int p = 0; p < PX; ++p) acc[p] = xv[p] > 0.0f ? acc[p] : acc[p] * g.slope;
    }
    hc_store_strip<T, PX>(dx + at, vec != 0, W - gx, acc);
  }
}

// ---- backward: d w, d bias -------------------------------------------------------------------------------------------
template <typename T, int COUT>
__global__ void __launch_bounds__(256)
hc_bwd_w_kernel(const T *__restrict__ x, const T *__restrict__ y0, const T *__restrict__ y1, const T *__restrict__ g0,
                const T *__restrict__ g1, float *__restrict__ partial, float *__restrict__ partial_b, HcGeo g, int band,
                int nband) {
  __shared__ float A[kHcWLanes * kHcWPitch];
  __shared__ float G[COUT * kHcWRows * kHcWCols];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slab = blockIdx.x, b = slab / nband;
  const int r_lo = (slab - b * nband) * band, r_hi = min(g.H, r_lo + band);
  const int H = g.H, W = g.W, HW = H * W, Cin = g.Cin;
  const int c_lo = blockIdx.y * kHcWLanes, cn = min(kHcWLanes, Cin - c_lo);
  const T *xb = x + ((int64_t)b * Cin + c_lo) * HW;
  float acc[COUT][9], gb[COUT];
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    gb[co] = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[co][k] = 0.0f;
  }
  const int sr = tid / (kHcWCols + 2), sc = tid - sr * (kHcWCols + 2);     // the staged position of this thread
  for (int row0 = r_lo; row0 < r_hi; row0 += kHcWRows) {
    for (int col0 = 0; col0 < W; col0 += kHcWCols) {
      __syncthreads();
      if (tid < kHcWPlane) {
        const int at = hc_src(row0 - 1 + sr, col0 - 1 + sc, H, W, g.reflect);
        for (int j0 = 0; j0 < cn; j0 += 8) {       // eight loads in flight, then their eight stores
          T v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = xb[(int64_t)min(j0 + j, cn - 1) * HW + max(at, 0)];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float a = at >= 0 ? Num<T>::ld(&v[j]) : 0.0f;
            if (g.pre_act) a = a > 0.0f ? a : a * g.slope;
            if (j0 + j < cn) A[(j0 + j) * kHcWPitch + tid] = a;
          }
        }
      }
      if (tid < kHcWRows * kHcWCols) {
        const int gy = row0 + (tid >> 5), gx = col0 + (tid & 31);
        const bool in = gy < r_hi && gx < W;
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
          const bool first = co < g.C0;
          const T *gp = first ? g0 : g1;
          const T *yp = first ? y0 : y1;
          const int64_t base = first ? ((int64_t)b * g.C0 + co) * HW : ((int64_t)b * (COUT - g.C0) + (co - g.C0)) * HW;
          float v = 0.0f;
          if (gp && in) v = hc_gprime<T>(gp, yp, base + (int64_t)gy * W + gx, hc_post_mode(co, g.tanh_mask, g.sig_mask));
          G[co * (kHcWRows * kHcWCols) + tid] = v;
        }
      }
      __syncthreads();
      if (row0 + wave < r_hi && lane < cn) {
        const float *ap = A + lane * kHcWPitch + wave * (kHcWCols + 2);
        const float *gp = G + wave * kHcWCols;
        const int cmax = min(kHcWCols, W - col0);
        float a[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) a[r][1] = ap[r * (kHcWCols + 2)], a[r][2] = ap[r * (kHcWCols + 2) + 1];
#pragma unroll 6
        for (int c = 0; c < cmax; ++c) {
#pragma unroll
          for (int r = 0; r < 3; ++r) a[r][0] = a[r][1], a[r][1] = a[r][2], a[r][2] = ap[r * (kHcWCols + 2) + c + 2];
#pragma unroll
          for (int co = 0; co < COUT; ++co) {
            const float gv = gp[co * (kHcWRows * kHcWCols) + c];
            gb[co] += gv;
#pragma unroll
            for (int k = 0; k < 9; ++k) acc[co][k] = fmaf(gv, a[k / 3][k % 3], acc[co][k]);
          }
        }
      }
    }
  }
  // the four waves in wave order, one output channel per round (A is free now)
#pragma unroll
  for (int co = 0; co < COUT; ++co) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k) A[(wave * 10 + k) * 64 + lane] = acc[co][k];
    A[(wave * 10 + 9) * 64 + lane] = gb[co];
    __syncthreads();
    if (wave == 0 && lane < cn) {
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        float s = A[k * 64 + lane];
#pragma unroll
        for (int v = 1; v < 4; ++v) s += A[(v * 10 + k) * 64 + lane];
        if (k < 9)
          partial[(((int64_t)slab * COUT + co) * 9 + k) * Cin + c_lo + lane] = s;
        else if (blockIdx.y == 0 && lane == 0)
          partial_b[(int64_t)slab * COUT + co] = s;
      }
    }
  }
}

// partials in a fixed order: a workgroup owns 16 outputs (in the partials' own layout [co][tap][ci], then the Cout bias
// sums) and cuts the slabs into 16 contiguous segments; thread (segment, output) adds its segment in slab order, eight
// loads in flight, and the segment sums are added in segment order.  dW is written as (Cout,Cin,3,3).
__global__ void __launch_bounds__(256)
hc_bwd_w_sum_kernel(const float *__restrict__ partial, const float *__restrict__ partial_b, float *__restrict__ dw,
                    float *__restrict__ db, int nslab, int Cout, int Cin) {
  __shared__ float part[16][17];
  const int n = Cout * 9 * Cin;
  const int o = threadIdx.x & 15, seg = threadIdx.x >> 4;
  const int j = blockIdx.x * 16 + o;
  const int per = (nslab + 15) / 16, t0 = seg * per, t1 = min(nslab, t0 + per);
  const bool is_w = j < n, is_b = !is_w && j < n + Cout;
  const float *src = is_w ? partial + j : partial_b + (j - n);
  const int64_t stride = is_w ? n : Cout;
  float s = 0.0f;
  if ((is_w && dw) || (is_b && db)) {
    int t = t0;
    for (; t + 8 <= t1; t += 8) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = src[(int64_t)(t + i) * stride];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; t < t1; ++t) s += src[(int64_t)t * stride];
  }
  part[seg][o] = s;
  __syncthreads();
  if (seg != 0) return;
  s = part[0][o];
#pragma unroll
  for (int i = 1; i < 16; ++i) s += part[i][o];
  if (is_w && dw) {
    const int ci = j % Cin, k = (j / Cin) % 9, co = j / (9 * Cin);
    dw[((int64_t)co * Cin + ci) * 9 + k] = s;
  } else if (is_b && db) {
    db[j - n] = s;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct HcTile {
  int tw, th, threads, lg, ntx, nty;
};

// the (tile width, workgroup size) that pads the plane least; a thread owns px x py pixels
static HcTile hc_pick_tile(int64_t H, int64_t W, int px, int py) {
  HcTile best = {};
  int64_t best_area = -1;
  for (int threads = 256; threads >= 64; threads /= 2)
    for (int tw = 64; tw >= 8; tw /= 2) {
      const int strips = tw / px, th = threads / strips * py;
      const int64_t area = ceil_div(W, tw) * tw * ceil_div(H, th) * th;
      if (best_area < 0 || area < best_area) {
        int lg = 0;
        while ((1 << lg) < strips) ++lg;
        best = {tw, th, threads, lg, (int)ceil_div(W, tw), (int)ceil_div(H, th)};
        best_area = area;
      }
    }
  return best;
}

struct HcBands {
  int64_t band, nband, nslab;
};
static HcBands hc_bands(int64_t B, int64_t H) {
  HcBands p;
  p.band = std::max<int64_t>(kHcWRows, kHcWRows * ceil_div(B * H, kHcWRows * kHcWantSlabs));
  p.nband = ceil_div(H, p.band);
  p.nslab = B * p.nband;
  return p;
}

static int hc_check(int64_t B, int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int tanh_mask,
                    int sig_mask) {
  if (B < 1 || Cin < 1 || Cout < 1 || Cout > kHcMaxCout || C0 < 1 || C0 > Cout || H < 1 || W < 1) return GFLA_ERR_BAD_SHAPE;
  if (pad_mode != 0 && pad_mode != 1) return GFLA_ERR_BAD_SHAPE;
  if (pad_mode == 1 && (H < 2 || W < 2)) return GFLA_ERR_BAD_SHAPE;
  const int all = (1 << Cout) - 1;
  if (tanh_mask < 0 || sig_mask < 0 || (tanh_mask & ~all) || (sig_mask & ~all) || (tanh_mask & sig_mask))
    return GFLA_ERR_BAD_SHAPE;
  if (H * W > 0x7fffffffLL || Cin > 0x7fffffffLL / 9 / kHcMaxCout || B > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

static HcGeo hc_geo(const HcTile &t, int64_t Cin, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act,
                    double slope, int tanh_mask, int sig_mask) {
  HcGeo g;
  g.H = (int)H, g.W = (int)W, g.Cin = (int)Cin, g.C0 = (int)C0;
  g.tw = t.tw, g.lg = t.lg, g.th = t.th, g.ntx = t.ntx, g.nty = t.nty;
  g.reflect = pad_mode, g.pre_act = pre_act ? 1 : 0, g.slope = (float)slope;
  g.tanh_mask = (unsigned)tanh_mask, g.sig_mask = (unsigned)sig_mask;
  return g;
}

template <typename T>
static bool hc_strips_whole(int64_t W, int px, const void *a, const void *b) {
  const uintptr_t m = (uintptr_t)(px * sizeof(T)) - 1;
  return W % px == 0 && !(reinterpret_cast<uintptr_t>(a) & m) && !(reinterpret_cast<uintptr_t>(b) & m);
}

#define GFLA_HC_COUT(VAL, ...)                 \
  switch (VAL) {                               \
    case 1: { constexpr int COUT = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int COUT = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int COUT = 3; __VA_ARGS__; } break; \
    case 4: { constexpr int COUT = 4; __VA_ARGS__; } break; \
    case 5: { constexpr int COUT = 5; __VA_ARGS__; } break; \
    case 6: { constexpr int COUT = 6; __VA_ARGS__; } break; \
    case 7: { constexpr int COUT = 7; __VA_ARGS__; } break; \
    case 8: { constexpr int COUT = 8; __VA_ARGS__; } break; \
  }

template <typename T>
static int hc_fwd(const T *x, const float *w, const float *bias, T *y0, T *y1, int64_t B, int64_t Cin, int64_t Cout,
                  int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act, double slope, int tanh_mask, int sig_mask,
                  gfla_stream_t stream) {
  if (!x || !w || !y0) return GFLA_ERR_NULL_POINTER;
  if (int rc = hc_check(B, Cin, Cout, C0, H, W, pad_mode, tanh_mask, sig_mask)) return rc;
  if (C0 < Cout && !y1) return GFLA_ERR_NULL_POINTER;
  const HcTile t = hc_pick_tile(H, W, 4, 2);
  const int64_t nwg = B * t.ntx * t.nty;
  if (nwg > 0x7fffffffLL || ceil_div((int64_t)(t.th + 2) * (t.tw + 2), t.threads) > kHcStage) return GFLA_ERR_UNSUPPORTED;
  const HcGeo g = hc_geo(t, Cin, C0, H, W, pad_mode, pre_act, slope, tanh_mask, sig_mask);
  const size_t lds = (size_t)kHcChunk * (t.th + 2) * (t.tw + 4) * sizeof(float);
  const int vec = hc_strips_whole<T>(W, 4, y0, C0 < Cout ? y1 : y0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  GFLA_HC_COUT((int)Cout, hc_fwd_kernel<T, COUT><<<dim3((unsigned)nwg), t.threads, lds, st>>>(x, w, bias, y0, y1, g, vec))
  return launch_status();
}

template <typename T>
static int hc_bwd(const T *x, const float *w, const T *y0, const T *y1, const T *g0, const T *g1, T *dx, float *dw,
                  float *db, void *workspace, int64_t B, int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W,
                  int pad_mode, int pre_act, double slope, int tanh_mask, int sig_mask, gfla_stream_t stream) {
  if (!x || !w || !y0) return GFLA_ERR_NULL_POINTER;
  if (int rc = hc_check(B, Cin, Cout, C0, H, W, pad_mode, tanh_mask, sig_mask)) return rc;
  if (C0 < Cout && !y1) return GFLA_ERR_NULL_POINTER;
  if ((dw || db) && !workspace) return GFLA_ERR_NULL_POINTER;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int px = Cout <= 4 ? 4 : 2;
  const HcTile t = hc_pick_tile(H, W, px, 1);
  const int64_t tiles = B * t.ntx * t.nty;
  const HcBands bands = hc_bands(B, H);
  const int64_t cgroups = ceil_div(Cin, kHcWLanes);
  if (tiles > 0x7fffffffLL || ceil_div((int64_t)(t.th + 2) * (t.tw + 2), t.threads) > kHcStage || cgroups > 65535 ||
      bands.nslab > 0x7fffffffLL)
    return GFLA_ERR_UNSUPPORTED;
  if (dx) {
    // few tiles: split Cin over workgroups too (each stages g' again, Cout / Cin of the traffic)
    int64_t split = std::min<int64_t>(std::min<int64_t>(ceil_div(4 * kNumCU, tiles), ceil_div(Cin, 8)), 65535);
    const int64_t ci_per = ceil_div(Cin, std::max<int64_t>(split, 1));
    split = ceil_div(Cin, ci_per);
    const HcGeo g = hc_geo(t, Cin, C0, H, W, pad_mode, pre_act, slope, tanh_mask, sig_mask);
    const size_t lds = (size_t)Cout * (t.th + 2) * (t.tw + 2) * sizeof(float);
    const dim3 grid((unsigned)tiles, (unsigned)split);
    if (px == 4) {
      const int vec = hc_strips_whole<T>(W, 4, x, dx);
      GFLA_HC_COUT((int)Cout, hc_bwd_x_kernel<T, (COUT <= 4 ? COUT : 1), 4><<<grid, t.threads, lds, st>>>(
                                  x, w, y0, y1, g0, g1, dx, g, (int)ci_per, vec))
    } else {
      const int vec = hc_strips_whole<T>(W, 2, x, dx);
      GFLA_HC_COUT((int)Cout, hc_bwd_x_kernel<T, (COUT > 4 ? COUT : 8), 2><<<grid, t.threads, lds, st>>>(
                                  x, w, y0, y1, g0, g1, dx, g, (int)ci_per, vec))
    }
  }
  if (dw || db) {
    const HcTile none = {};
    const HcGeo g = hc_geo(none, Cin, C0, H, W, pad_mode, pre_act, slope, tanh_mask, sig_mask);
    float *partial = static_cast<float *>(workspace);
    float *partial_b = partial + bands.nslab * Cout * 9 * Cin;
    const dim3 grid((unsigned)bands.nslab, (unsigned)cgroups);
    GFLA_HC_COUT((int)Cout, hc_bwd_w_kernel<T, COUT><<<grid, 256, 0, st>>>(x, y0, y1, g0, g1, partial, partial_b, g,
                                                                        (int)bands.band, (int)bands.nband))
    const int64_t n = Cout * 9 * Cin + Cout;
    hc_bwd_w_sum_kernel<<<dim3((unsigned)ceil_div(n, 16)), kBlock, 0, st>>>(partial, partial_b, dw, db, (int)bands.nslab,
                                                                              (int)Cout, (int)Cin);
  }
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_head_conv3x3_workspace_bytes(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int elem_size) {
  if (elem_size != 2 && elem_size != 4) return GFLA_ERR_BAD_SHAPE;
  if (int rc = gfla::hc_check(B, Cin, Cout, Cout, H, W, 0, 0, 0)) return rc;
  const gfla::HcBands p = gfla::hc_bands(B, H);
  if (p.nslab > 0x7fffffffLL) return GFLA_ERR_UNSUPPORTED;
  return p.nslab * (Cout * 9 * Cin + Cout) * (int64_t)sizeof(float);
}

int gfla_head_conv3x3_geometry(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int is_backward, int64_t *out) {
  if (!out) return GFLA_ERR_NULL_POINTER;
  if (int rc = gfla::hc_check(B, Cin, Cout, Cout, H, W, 0, 0, 0)) return rc;
  const gfla::HcTile t = is_backward ? gfla::hc_pick_tile(H, W, Cout <= 4 ? 4 : 2, 1) : gfla::hc_pick_tile(H, W, 4, 2);
  const gfla::HcBands p = gfla::hc_bands(B, H);
  out[0] = t.tw, out[1] = t.th, out[2] = t.threads, out[3] = (int64_t)t.ntx * t.nty;
  out[4] = p.band, out[5] = p.nslab, out[6] = gfla::ceil_div(Cin, gfla::kHcWLanes);
  return GFLA_OK;
}

#define GFLA_DEF_HEAD_CONV(SFX, ABI_T, T)                                                                                    \
  int gfla_head_conv3x3_fwd_##SFX(const ABI_T *x, const float *w, const float *bias, ABI_T *y0, ABI_T *y1, int64_t B,        \
                                  int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act,   \
                                  double pre_slope, int tanh_mask, int sigmoid_mask, gfla_stream_t stream) {                 \
    return gfla::hc_fwd<T>(reinterpret_cast<const T *>(x), w, bias, reinterpret_cast<T *>(y0), reinterpret_cast<T *>(y1), B, \
                           Cin, Cout, C0, H, W, pad_mode, pre_act, pre_slope, tanh_mask, sigmoid_mask, stream);              \
  }                                                                                                                          \
  int gfla_head_conv3x3_bwd_##SFX(const ABI_T *x, const float *w, const ABI_T *y0, const ABI_T *y1, const ABI_T *grad_y0,    \
                                  const ABI_T *grad_y1, ABI_T *grad_x, float *grad_w, float *grad_b, void *workspace,        \
                                  int64_t B, int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode,      \
                                  int pre_act, double pre_slope, int tanh_mask, int sigmoid_mask, gfla_stream_t stream) {    \
    return gfla::hc_bwd<T>(reinterpret_cast<const T *>(x), w, reinterpret_cast<const T *>(y0),                               \
                           reinterpret_cast<const T *>(y1), reinterpret_cast<const T *>(grad_y0),                            \
                           reinterpret_cast<const T *>(grad_y1), reinterpret_cast<T *>(grad_x), grad_w, grad_b, workspace,   \
                           B, Cin, Cout, C0, H, W, pad_mode, pre_act, pre_slope, tanh_mask, sigmoid_mask, stream);           \
  }
GFLA_DEF_HEAD_CONV(f32, float, float)
GFLA_DEF_HEAD_CONV(f16, uint16_t, f16_t)
GFLA_DEF_HEAD_CONV(bf16, uint16_t, bf16_t)
#undef GFLA_DEF_HEAD_CONV
}
