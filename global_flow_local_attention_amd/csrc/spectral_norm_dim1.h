// The batched spectral norm's table record, and the passes of a matrix normalised along dim 1 (csrc/spectral_norm.hip;
// include/gfla_spectral_norm.h: the gfla_spectral_norm_mixed_* entry points).
//
// torch normalises an nn.ConvTranspose2d along dim 1: a weight stored (Cin, R, inner) -- R = Cout, inner = kh kw -- is the
// R x K matrix, K = Cin inner, whose element (r, c) lies at ((c / inner) R + r) inner + c % inner.  Such a matrix (a record
// of 9 words with [8] = inner > 0) goes through the launches of spectral_norm.hip, each workgroup taking the branch of its
// matrix, and every pass streams the weight in storage order, consecutive lanes at consecutive addresses:
//   column sums   slice = one slab W[ci] of R inner contiguous floats, read front to back by the whole workgroup.  A
//                 thread adds element o = r inner + j into its own LDS bin of tap j (no two threads share a bin, so the
//                 bins need no barrier while they fill); a wave then adds the 256 bins of a tap: four per lane in thread
//                 order, xor butterfly.  inner sums per slab.  Never a walk at stride inner.
//   row dots      slice = max(1, 64 / inner) rows: in every slab their floats are one contiguous run, one lane per float;
//                 wave w takes the slabs ci = w, w + 4, ...  Lane (row, tap) keeps one accumulator over its slabs; one
//                 thread per row then adds the waves' values in wave order, taps ascending.  Never a walk at stride
//                 R inner by neighbouring lanes.
//   scale         sigma = u . s and the buffers as for dim 0, then W / sigma element-wise in storage order.
// <G, W> is element-wise as well; grad_w maps a storage offset back to (r, c) (sn_bwd_apply_kernel).
//
// Sums: float64, on the float32 weight.  The bins and the per-row sums above are serial where the dim-0 passes have a
// butterfly, and sigma = u . (W v) cancels when u and v are not yet singular vectors (an eval-mode forward on fresh
// buffers).  So t, s and both norms stay float64 between the passes (`wide`: t at the K-vector's offset, s at the
// R-vector's, the offsets of the float32 vector arrays); float32 are the weight, the buffers u and v -- each entry rounded
// once from its float64 value -- and sigma, rounded once.  FP64 FMA runs at the FP32 rate's half on this part and the
// passes are bound by the weight's bytes.  The order of every sum depends on (R, K, inner) alone.
#ifndef GFLA_SPECTRAL_NORM_DIM1_H_
#define GFLA_SPECTRAL_NORM_DIM1_H_

#include "gfla_common.h"

namespace gfla {

constexpr int kSnMaxInner = 25;      // dim 1: taps per (Cin, Cout) pair; the column sums keep inner x kBlock float64 LDS bins
constexpr int kSnWords0 = 8;         // int64 per record of the dim-0 entry points
constexpr int kSnWords = 9;          // ... of the mixed ones: [8] = inner, 0 for a matrix read as stored
constexpr int kSnElems = 4096;       // elements per workgroup of the element-wise passes

struct SnRec {
  int64_t w, u, v, R, K, elem_off, k_off, r_off, inner;
};

__device__ __forceinline__ SnRec sn_rec(const int64_t *__restrict__ table, int words, int i) {
  const int64_t *p = table + (int64_t)i * words;
  return SnRec{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], words > kSnWords0 ? p[8] : 0};
}

// rows per workgroup of the dim-1 row dots: their floats in one slab fill at most one wave
__host__ __device__ __forceinline__ int sn_rows1(int inner) { return inner >= 64 ? 1 : 64 / inner; }

__device__ __forceinline__ double sn_wave_sum64(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the same value in every thread; lds: kBlock / 64 doubles
__device__ __forceinline__ double sn_block_sum64(double v, double *lds) {
  v = sn_wave_sum64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = lds[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) total += lds[w];
  return total;
}

// max(||x||_2, eps) of n doubles, the same bits in every workgroup that asks; a NaN norm stays NaN
__device__ __forceinline__ double sn_denominator64(const double *x, int n, float eps, double *lds) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) acc += x[i] * x[i];
  const double norm = sqrt(sn_block_sum64(acc, lds));
  return norm < (double)eps ? (double)eps : norm;
}

// t = W^T u over the slab W[blockIdx.x] of a dim-1 matrix
__device__ __forceinline__ void sn_colsum_dim1(const SnRec &rec, double *__restrict__ wide, int from_s, float eps) {
  extern __shared__ __attribute__((aligned(16))) double sn_bins[];     // inner x kBlock
  __shared__ double red[kBlock / 64];
  const int R = (int)rec.R, inner = (int)rec.inner;
  const int ci = blockIdx.x;
  if (ci >= (int)rec.K / inner) return;
  const double *s = wide + rec.r_off;
  const float *ubuf = reinterpret_cast<const float *>(rec.u);
  const double den = from_s ? sn_denominator64(s, R, eps, red) : 1.0;
  const int slab = R * inner;                                          // R K <= 2^31 - 1
  const float *W = reinterpret_cast<const float *>(rec.w) + (int64_t)ci * slab;
  for (int j = 0; j < inner; ++j) sn_bins[j * kBlock + threadIdx.x] = 0.0;
  for (int o = threadIdx.x; o < slab; o += kBlock) {
    const int r = o / inner, j = o - r * inner;
    const double ur = from_s ? s[r] / den : (double)ubuf[r];
    sn_bins[j * kBlock + threadIdx.x] += (double)W[o] * ur;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = wave; j < inner; j += kBlock / 64) {
    double acc = sn_bins[j * kBlock + lane];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) acc += sn_bins[j * kBlock + w * 64 + lane];
    acc = sn_wave_sum64(acc);
    if (lane == 0) wide[rec.k_off + ci * inner + j] = acc;
  }
}

// s = W v over the rows [blockIdx.x rows, + rows) of a dim-1 matrix.  from_t: v = t / max(||t||, eps), written to the
// module's buffer (and `saved`) by slice 0; else the buffer
__device__ __forceinline__ void sn_rowdot_dim1(const SnRec &rec, double *__restrict__ wide, float *__restrict__ saved,
                                               int from_t, float eps) {
  __shared__ double part[kBlock / 64][64];
  __shared__ double red[kBlock / 64];
  const int R = (int)rec.R, K = (int)rec.K, inner = (int)rec.inner;
  const int rows = sn_rows1(inner), r0 = blockIdx.x * rows;
  if (r0 >= R) return;
  const float *W = reinterpret_cast<const float *>(rec.w);
  const double *t = wide + rec.k_off;
  float *vbuf = reinterpret_cast<float *>(rec.v);
  const double den = from_t ? sn_denominator64(t, K, eps, red) : 1.0;
  if (from_t && blockIdx.x == 0) {
    for (int c = threadIdx.x; c < K; c += kBlock) {
      const float vc = (float)(t[c] / den);
      vbuf[c] = vc;
      if (saved != nullptr) saved[rec.k_off + c] = vc;
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rl = lane / inner, j = lane - rl * inner;
  const int slab = R * inner, cin = K / inner;
  double acc = 0.0;
  if (rl < rows && r0 + rl < R) {
    const float *run = W + (int64_t)r0 * inner + lane;                 // = (r0 + rl) inner + j of slab 0
    for (int ci = wave; ci < cin; ci += kBlock / 64) {
      const double vc = from_t ? t[ci * inner + j] / den : (double)vbuf[ci * inner + j];
      acc += (double)run[(int64_t)ci * slab] * vc;
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  const int mine = threadIdx.x;
  if (mine < rows && r0 + mine < R) {
    double total = 0.0;
    for (int w = 0; w < kBlock / 64; ++w)
      for (int jj = 0; jj < inner; ++jj) total += part[w][mine * inner + jj];
    wide[rec.r_off + r0 + mine] = total;
  }
}

// sigma = u . s, W_sn = W / sigma over the elements [blockIdx.x kSnElems, + kSnElems) of a dim-1 matrix's storage.  from_s:
// u = s / max(||s||, eps), written to the module's buffer (and `saved`) by slice 0; else u is the buffer and slice 0 only
// copies u and v to `saved`.  As sn_scale_kernel does for dim 0, on the float64 s.
__device__ __forceinline__ void sn_scale_dim1(const SnRec &rec, int matrix, const double *__restrict__ wide,
                                              float *__restrict__ w_sn, float *__restrict__ sigma_out,
                                              float *__restrict__ saved, int from_s, float eps) {
  __shared__ double red[kBlock / 64];
  const int R = (int)rec.R, K = (int)rec.K;
  const int64_t total = rec.R * rec.K;
  const int64_t e0 = (int64_t)blockIdx.x * kSnElems;
  if (e0 >= total) return;
  const float *W = reinterpret_cast<const float *>(rec.w);
  const double *s = wide + rec.r_off;
  float *ubuf = reinterpret_cast<float *>(rec.u);
  const double den = from_s ? sn_denominator64(s, R, eps, red) : 1.0;
  double acc = 0.0;
  for (int r = threadIdx.x; r < R; r += kBlock) acc += (from_s ? s[r] / den : (double)ubuf[r]) * s[r];
  const float sigma = (float)sn_block_sum64(acc, red);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) sigma_out[matrix] = sigma;
    for (int r = threadIdx.x; r < R; r += kBlock) {
      const float ur = from_s ? (float)(s[r] / den) : ubuf[r];
      if (from_s) ubuf[r] = ur;
      if (saved != nullptr) saved[rec.r_off + r] = ur;
    }
    if (!from_s && saved != nullptr) {
      const float *vbuf = reinterpret_cast<const float *>(rec.v);
      for (int c = threadIdx.x; c < K; c += kBlock) saved[rec.k_off + c] = vbuf[c];
    }
  }
  float *out = w_sn + rec.elem_off;
  const bool vec = ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
#pragma unroll
  for (int j = 0; j < kSnElems / (4 * kBlock); ++j) {
    const int64_t e = e0 + (int64_t)(j * kBlock + threadIdx.x) * 4;
    if (e >= total) break;
    if (vec && e + 4 <= total) {
      float4 w = *reinterpret_cast<const float4 *>(W + e);
      w.x /= sigma, w.y /= sigma, w.z /= sigma, w.w /= sigma;
      *reinterpret_cast<float4 *>(out + e) = w;
    } else {
      for (int64_t i = e; i < e + 4 && i < total; ++i) out[i] = W[i] / sigma;
    }
  }
}

}  // namespace gfla

#endif  // GFLA_SPECTRAL_NORM_DIM1_H_
