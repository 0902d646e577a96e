// Spectral normalisation of a batch of weight matrices, forward and backward, gfx950 (include/gfla_spectral_norm.h).
//
// torch's hook runs, per convolution and per forward, three gemv, two normalisations, a dot and a division: about ten
// launches on a matrix of a few thousand to 262,144 floats.  Here the whole batch of a network is a fixed number of
// launches, each over (matrix, slice):
//   sn_colsum_kernel    t[c] = sum_r W[r][c] u[r]       slice = 64 columns; the four waves take a quarter of the rows each
//   sn_rowdot_kernel    s[r] = sum_c W[r][c] v[c]       slice = 4 rows, one wave per row
//   sn_scale_kernel     sigma = u . s, W_sn = W / sigma slice = 4096 elements
// The vector a launch multiplies with is either a buffer of the module (u of the first iteration; u and v in eval mode) or
// the normalised output of the launch before it: t and s stay in scratch as computed, and every workgroup that needs
// v = t / max(||t||, eps) or u = s / max(||s||, eps) recomputes the norm from the whole vector (a few thousand floats out
// of L2) in the same fixed order.  So no workgroup reads a u or v that another workgroup of its launch writes: v is written
// (buffer and saved copy) by slice 0 of the row dots, which read t; u by slice 0 of the scale pass, which reads s.
//
// Sums: float32.  A thread adds its strided share in ascending order, a wave combines by xor butterfly, the waves' values
// are added in wave order.  The order depends on (R, K) alone: bit-identical from call to call, alone or in a batch.
// No atomics.
//
// A matrix normalised along dim 1 (nn.ConvTranspose2d; a 9-word record with inner > 0) runs in the same launches: its
// workgroups take sn_colsum_dim1 / sn_rowdot_dim1 / sn_scale_dim1 (spectral_norm_dim1.h, with the record and the layout).
#include <algorithm>

#include "spectral_norm_dim1.h"

namespace gfla {

constexpr int kSnCols = 64;          // columns per workgroup of the column sums
constexpr int kSnRows = 4;           // rows per workgroup of the row dots (one wave each)
constexpr int64_t kSnMaxDim = (int64_t)1 << 24;
constexpr int64_t kSnMaxElems = 2147483647;
constexpr int64_t kSnMaxBatch = 65535;

__device__ __forceinline__ float sn_wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// the same value in every thread; lds: kBlock / 64 floats
__device__ __forceinline__ float sn_block_sum(float v, float *lds) {
  v = sn_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  float total = lds[0];
#pragma unroll
  for (int w = 1; w < kBlock / 64; ++w) total += lds[w];
  return total;
}

// max(||x||_2, eps) of a vector of n floats, the same bits in every workgroup that asks.  A NaN norm stays NaN, as
// F.normalize's clamp_min keeps it (fmaxf would hand back eps, and a vector with one NaN entry would keep its others)
__device__ __forceinline__ float sn_denominator(const float *x, int n, float eps, float *lds) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += kBlock) acc += x[i] * x[i];
  const float norm = sqrtf(sn_block_sum(acc, lds));
  return norm < eps ? eps : norm;
}

// t = W^T u.  from_s: u = s / max(||s||, eps) of the iteration before, else the module's buffer.
__global__ __launch_bounds__(kBlock) void sn_colsum_kernel(const int64_t *__restrict__ table, int words, double *__restrict__ wide,
                                                           float *__restrict__ scratch, int from_s, float eps) {
  __shared__ float red[kBlock / 64];
  __shared__ float part[kBlock / 64][kSnCols];
  const SnRec rec = sn_rec(table, words, blockIdx.y);
  if (rec.inner > 0) return sn_colsum_dim1(rec, wide, from_s, eps);
  const int R = (int)rec.R, K = (int)rec.K;
  const int c0 = blockIdx.x * kSnCols;
  if (c0 >= K) return;
  const float *W = reinterpret_cast<const float *>(rec.w);
  const float *s = scratch + rec.r_off;
  const float *u = from_s ? s : reinterpret_cast<const float *>(rec.u);
  const float den = from_s ? sn_denominator(s, R, eps, red) : 1.f;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = c0 + lane;
  float acc = 0.f;
  if (c < K) {
    for (int r = wave; r < R; r += kBlock / 64) {
      const float ur = from_s ? u[r] / den : u[r];
      acc += W[(int64_t)r * K + c] * ur;
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && c < K) {
    float total = part[0][lane];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) total += part[w][lane];
    scratch[rec.k_off + c] = total;
  }
}

// s = W v.  from_t: v = t / max(||t||, eps), written to the module's buffer (and `saved`) by slice 0; else the buffer.
__global__ __launch_bounds__(kBlock) void sn_rowdot_kernel(const int64_t *__restrict__ table, int words, double *__restrict__ wide,
                                                           float *__restrict__ scratch, float *__restrict__ saved, int from_t, float eps) {
  __shared__ float red[kBlock / 64];
  const SnRec rec = sn_rec(table, words, blockIdx.y);
  if (rec.inner > 0) return sn_rowdot_dim1(rec, wide, saved, from_t, eps);
  const int R = (int)rec.R, K = (int)rec.K;
  const int r0 = blockIdx.x * kSnRows;
  if (r0 >= R) return;
  const float *W = reinterpret_cast<const float *>(rec.w);
  const float *t = scratch + rec.k_off;
  float *vbuf = reinterpret_cast<float *>(rec.v);
  const float *v = from_t ? t : vbuf;
  const float den = from_t ? sn_denominator(t, K, eps, red) : 1.f;
  if (from_t && blockIdx.x == 0) {
    for (int c = threadIdx.x; c < K; c += kBlock) {
      const float vc = t[c] / den;
      vbuf[c] = vc;
      if (saved != nullptr) saved[rec.k_off + c] = vc;
    }
  }
  const int lane = threadIdx.x & 63, r = r0 + (threadIdx.x >> 6);
  if (r >= R) return;                              // whole waves; no barrier below
  const float *row = W + (int64_t)r * K;
  float acc = 0.f;
  for (int c = lane; c < K; c += 64) {
    const float vc = from_t ? v[c] / den : v[c];
    acc += row[c] * vc;
  }
  acc = sn_wave_sum(acc);
  if (lane == 0) scratch[rec.r_off + r] = acc;
}

// sigma = u . s, W_sn = W / sigma.  from_s: u = s / max(||s||, eps), written to the module's buffer (and `saved`) by slice
// 0; else u is the buffer and slice 0 only copies u and v to `saved`.
__global__ __launch_bounds__(kBlock) void sn_scale_kernel(const int64_t *__restrict__ table, int words, const double *__restrict__ wide,
                                                          const float *__restrict__ scratch, float *__restrict__ w_sn,
                                                          float *__restrict__ sigma_out, float *__restrict__ saved, int from_s, float eps) {
  __shared__ float red[kBlock / 64];
  const SnRec rec = sn_rec(table, words, blockIdx.y);
  if (rec.inner > 0) return sn_scale_dim1(rec, blockIdx.y, wide, w_sn, sigma_out, saved, from_s, eps);
  const int R = (int)rec.R, K = (int)rec.K;
  const int64_t total = rec.R * rec.K;
  const int64_t e0 = (int64_t)blockIdx.x * kSnElems;
  if (e0 >= total) return;
  const float *W = reinterpret_cast<const float *>(rec.w);
  const float *s = scratch + rec.r_off;
  float *ubuf = reinterpret_cast<float *>(rec.u);
  const float den = from_s ? sn_denominator(s, R, eps, red) : 1.f;
  float acc = 0.f;
  for (int r = threadIdx.x; r < R; r += kBlock) {
    const float ur = from_s ? s[r] / den : ubuf[r];
    acc += ur * s[r];
  }
  const float sigma = sn_block_sum(acc, red);
  if (blockIdx.x == 0) {
    if (threadIdx.x == 0) sigma_out[blockIdx.y] = sigma;
    for (int r = threadIdx.x; r < R; r += kBlock) {
      const float ur = from_s ? s[r] / den : ubuf[r];
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

// partial[matrix][slice] = sum over the slice's elements of G W
__global__ __launch_bounds__(kBlock) void sn_bwd_dot_kernel(const int64_t *__restrict__ table, int words, const float *__restrict__ grad_sn,
                                                            float *__restrict__ partial, int max_slices) {
  __shared__ float red[kBlock / 64];
  const SnRec rec = sn_rec(table, words, blockIdx.y);
  const int64_t total = rec.R * rec.K;
  const int64_t e0 = (int64_t)blockIdx.x * kSnElems;
  if (e0 >= total) return;
  const float *W = reinterpret_cast<const float *>(rec.w);
  const float *G = grad_sn + rec.elem_off;
  const bool vec = ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(G)) & 15) == 0;
  float acc = 0.f;
#pragma unroll
  for (int j = 0; j < kSnElems / (4 * kBlock); ++j) {
    const int64_t e = e0 + (int64_t)(j * kBlock + threadIdx.x) * 4;
    if (e >= total) break;
    // The pointers decide how a group of four is LOADED, never how it is added.  Left to the compiler the float4 branch
    // became v_pk_mul_f32 + v_add_f32 (every product rounded) and the scalar branch v_fmac_f32 (fused), so <G, W>, and
    // with it c and grad_w, changed in the last bit with the phase of W.  A whole group rounds its products, the ragged
    // last group of a matrix is fused: what an aligned call has always computed.
    if (e + 4 <= total) {
      float g[4], w[4];
      if (vec) {
        const float4 w4 = *reinterpret_cast<const float4 *>(W + e);
        const float4 g4 = *reinterpret_cast<const float4 *>(G + e);
        g[0] = g4.x, g[1] = g4.y, g[2] = g4.z, g[3] = g4.w;
        w[0] = w4.x, w[1] = w4.y, w[2] = w4.z, w[3] = w4.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) g[i] = G[e + i], w[i] = W[e + i];
      }
      {
#pragma clang fp contract(off)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = g[i] * w[i];
          acc = acc + p;
        }
      }
    } else {
      for (int64_t i = e; i < total; ++i) acc = fmaf(G[i], W[i], acc);
    }
  }
  acc = sn_block_sum(acc, red);
  if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * max_slices + blockIdx.x] = acc;
}

// grad_w = (G - c u v^T) / sigma with c = <G, W> / sigma: the partials of the matrix added in slice order
__global__ __launch_bounds__(kBlock) void sn_bwd_apply_kernel(const int64_t *__restrict__ table, int words,
                                                              const float *__restrict__ grad_sn, const float *__restrict__ saved,
                                                              const float *__restrict__ sigmas, const float *__restrict__ partial,
                                                              float *__restrict__ grad_w, int max_slices) {
  __shared__ float red[kBlock / 64];
  const SnRec rec = sn_rec(table, words, blockIdx.y);
  const uint32_t K = (uint32_t)rec.K;
  const int64_t total = rec.R * rec.K;
  const int64_t e0 = (int64_t)blockIdx.x * kSnElems;
  if (e0 >= total) return;
  const int slices = (int)((total + kSnElems - 1) / kSnElems);
  const float *mine = partial + (int64_t)blockIdx.y * max_slices;
  float acc = 0.f;
  for (int i = threadIdx.x; i < slices; i += kBlock) acc += mine[i];
  const float sigma = sigmas[blockIdx.y];
  const float c = sn_block_sum(acc, red) / sigma;
  const float *G = grad_sn + rec.elem_off;
  const float *u = saved + rec.r_off, *v = saved + rec.k_off;
  float *out = grad_w + rec.elem_off;
  const bool vec = ((reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
#pragma unroll
  for (int j = 0; j < kSnElems / (4 * kBlock); ++j) {
    const int64_t e = e0 + (int64_t)(j * kBlock + threadIdx.x) * 4;
    if (e >= total) break;
    const int n = (int)(total - e < 4 ? total - e : 4);
    float g[4], res[4];
    if (vec && n == 4) {
      const float4 g4 = *reinterpret_cast<const float4 *>(G + e);
      g[0] = g4.x, g[1] = g4.y, g[2] = g4.z, g[3] = g4.w;
    } else {
      for (int i = 0; i < n; ++i) g[i] = G[e + i];
    }
    if (rec.inner > 0) {                                           // storage (ci, r, tap): column ci inner + tap
      const uint32_t inner = (uint32_t)rec.inner, slab = (uint32_t)rec.R * inner;
      for (int i = 0; i < n; ++i) {
        const uint32_t o = (uint32_t)e + i, ci = o / slab, rem = o - ci * slab, r = rem / inner, j = rem - r * inner;
        res[i] = (g[i] - c * u[r] * v[ci * inner + j]) / sigma;
      }
    } else {
      uint32_t r = (uint32_t)e / K, col = (uint32_t)e - r * K;      // R K <= 2^31 - 1
      for (int i = 0; i < n; ++i) {
        res[i] = (g[i] - c * u[r] * v[col]) / sigma;
        if (++col == K) col = 0, ++r;
      }
    }
    if (vec && n == 4) {
      *reinterpret_cast<float4 *>(out + e) = make_float4(res[0], res[1], res[2], res[3]);
    } else {
      for (int i = 0; i < n; ++i) out[e + i] = res[i];
    }
  }
}

struct SnShape {
  int64_t col_slices = 0, row_slices = 0, max_elems = 0, max_inner = 0, vecs = 0;
};

// the argument checks every entry point shares; the shape summary the launch geometry needs.  words_per: 2 (R, K) for
// the dim-0 entry points, 3 (R, K, inner) for the mixed ones
static int sn_check(const int64_t *dims, int words_per, int64_t n, SnShape *shape) {
  if (dims == nullptr) return GFLA_ERR_NULL_POINTER;
  if (n <= 0) return GFLA_ERR_BAD_SHAPE;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t R = dims[words_per * i], K = dims[words_per * i + 1], inner = words_per > 2 ? dims[words_per * i + 2] : 0;
    if (R <= 0 || K <= 0 || inner < 0 || (inner > 0 && K % inner != 0)) return GFLA_ERR_BAD_SHAPE;
  }
  if (n > kSnMaxBatch) return GFLA_ERR_UNSUPPORTED;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t R = dims[words_per * i], K = dims[words_per * i + 1], inner = words_per > 2 ? dims[words_per * i + 2] : 0;
    if (R > kSnMaxDim || K > kSnMaxDim || R * K > kSnMaxElems || inner > kSnMaxInner) return GFLA_ERR_UNSUPPORTED;
    shape->col_slices = std::max(shape->col_slices, inner > 0 ? K / inner : ceil_div(K, (int64_t)kSnCols));
    shape->row_slices = std::max(shape->row_slices, ceil_div(R, (int64_t)(inner > 0 ? sn_rows1((int)inner) : kSnRows)));
    shape->max_elems = std::max(shape->max_elems, R * K);
    shape->max_inner = std::max(shape->max_inner, inner);
    shape->vecs += R + K;
  }
  return GFLA_OK;
}

static int sn_layout(const int64_t *dims, int words_per, int64_t n, int64_t *offsets, int64_t *totals) {
  if (offsets == nullptr || totals == nullptr) return GFLA_ERR_NULL_POINTER;
  SnShape shape;
  const int status = sn_check(dims, words_per, n, &shape);
  if (status != GFLA_OK) return status;
  int64_t elems = 0, vecs = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int64_t R = dims[words_per * i], K = dims[words_per * i + 1];
    offsets[3 * i] = elems;
    offsets[3 * i + 1] = vecs;
    offsets[3 * i + 2] = vecs + K;
    elems += R * K;
    vecs += R + K;
  }
  totals[0] = elems;
  totals[1] = vecs;
  return GFLA_OK;
}

static int64_t sn_bwd_scratch(const int64_t *dims, int words_per, int64_t n) {
  SnShape shape;
  const int status = sn_check(dims, words_per, n, &shape);
  if (status != GFLA_OK) return status;
  return n * ceil_div(shape.max_elems, (int64_t)kSnElems);
}

static int sn_forward(const void *table, int words, const int64_t *dims, int words_per, int64_t n, float *w_sn, float *sigma,
                      float *saved, float *scratch, int power_iterations, double eps, gfla_stream_t stream) {
  if (table == nullptr || dims == nullptr || w_sn == nullptr || sigma == nullptr || scratch == nullptr)
    return GFLA_ERR_NULL_POINTER;
  if (power_iterations < 0 || !(eps > 0)) return GFLA_ERR_BAD_SHAPE;
  SnShape shape;
  const int status = sn_check(dims, words_per, n, &shape);
  if (status != GFLA_OK) return status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t *recs = static_cast<const int64_t *>(table);
  const float feps = (float)eps;
  const dim3 cols((unsigned)shape.col_slices, (unsigned)n);
  const dim3 rows((unsigned)shape.row_slices, (unsigned)n);
  const dim3 elems((unsigned)ceil_div(shape.max_elems, (int64_t)kSnElems), (unsigned)n);
  const size_t bins = (size_t)shape.max_inner * kBlock * sizeof(double);     // 0 for a batch of dim-0 matrices
  // the float64 t and s of the dim-1 matrices: behind the float32 vector arrays, at the next multiple of 8 bytes; the
  // dim-0 entry points have neither (their scratch ends with the float32 arrays) and no kernel of theirs looks
  double *wide = words > kSnWords0
                     ? reinterpret_cast<double *>((reinterpret_cast<uintptr_t>(scratch + shape.vecs) + 7) & ~(uintptr_t)7)
                     : nullptr;
  for (int it = 0; it < power_iterations; ++it) {
    hipLaunchKernelGGL(sn_colsum_kernel, cols, dim3(kBlock), bins, st, recs, words, wide, scratch, it > 0 ? 1 : 0, feps);
    hipLaunchKernelGGL(sn_rowdot_kernel, rows, dim3(kBlock), 0, st, recs, words, wide, scratch, saved, 1, feps);
  }
  if (power_iterations == 0)
    hipLaunchKernelGGL(sn_rowdot_kernel, rows, dim3(kBlock), 0, st, recs, words, wide, scratch, saved, 0, feps);
  hipLaunchKernelGGL(sn_scale_kernel, elems, dim3(kBlock), 0, st, recs, words, wide, scratch, w_sn, sigma, saved,
                     power_iterations > 0 ? 1 : 0, feps);
  return launch_status();
}

static int sn_backward(const void *table, int words, const int64_t *dims, int words_per, int64_t n, const float *grad_sn,
                       const float *saved, const float *sigma, float *grad_w, float *scratch, gfla_stream_t stream) {
  if (table == nullptr || dims == nullptr || grad_sn == nullptr || saved == nullptr || sigma == nullptr ||
      grad_w == nullptr || scratch == nullptr)
    return GFLA_ERR_NULL_POINTER;
  SnShape shape;
  const int status = sn_check(dims, words_per, n, &shape);
  if (status != GFLA_OK) return status;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t *recs = static_cast<const int64_t *>(table);
  const int max_slices = (int)ceil_div(shape.max_elems, (int64_t)kSnElems);
  const dim3 elems((unsigned)max_slices, (unsigned)n);
  hipLaunchKernelGGL(sn_bwd_dot_kernel, elems, dim3(kBlock), 0, st, recs, words, grad_sn, scratch, max_slices);
  hipLaunchKernelGGL(sn_bwd_apply_kernel, elems, dim3(kBlock), 0, st, recs, words, grad_sn, saved, sigma, scratch, grad_w,
                     max_slices);
  return launch_status();
}

}  // namespace gfla

using namespace gfla;

extern "C" int gfla_spectral_norm_layout(const int64_t *dims, int64_t n, int64_t *offsets, int64_t *totals) {
  return sn_layout(dims, 2, n, offsets, totals);
}

extern "C" int64_t gfla_spectral_norm_bwd_scratch_floats(const int64_t *dims, int64_t n) { return sn_bwd_scratch(dims, 2, n); }

extern "C" int gfla_spectral_norm_fwd_f32(const void *table, const int64_t *dims, int64_t n, float *w_sn, float *sigma,
                                          float *saved, float *scratch, int power_iterations, double eps,
                                          gfla_stream_t stream) {
  return sn_forward(table, kSnWords0, dims, 2, n, w_sn, sigma, saved, scratch, power_iterations, eps, stream);
}

extern "C" int gfla_spectral_norm_bwd_f32(const void *table, const int64_t *dims, int64_t n, const float *grad_sn,
                                          const float *saved, const float *sigma, float *grad_w, float *scratch,
                                          gfla_stream_t stream) {
  return sn_backward(table, kSnWords0, dims, 2, n, grad_sn, saved, sigma, grad_w, scratch, stream);
}

extern "C" int gfla_spectral_norm_mixed_layout(const int64_t *dims, int64_t n, int64_t *offsets, int64_t *totals) {
  return sn_layout(dims, 3, n, offsets, totals);
}

extern "C" int64_t gfla_spectral_norm_mixed_bwd_scratch_floats(const int64_t *dims, int64_t n) {
  return sn_bwd_scratch(dims, 3, n);
}

extern "C" int gfla_spectral_norm_mixed_fwd_f32(const void *table, const int64_t *dims, int64_t n, float *w_sn, float *sigma,
                                                float *saved, float *scratch, int power_iterations, double eps,
                                                gfla_stream_t stream) {
  return sn_forward(table, kSnWords, dims, 3, n, w_sn, sigma, saved, scratch, power_iterations, eps, stream);
}

extern "C" int gfla_spectral_norm_mixed_bwd_f32(const void *table, const int64_t *dims, int64_t n, const float *grad_sn,
                                                const float *saved, const float *sigma, float *grad_w, float *scratch,
                                                gfla_stream_t stream) {
  return sn_backward(table, kSnWords, dims, 3, n, grad_sn, saved, sigma, grad_w, scratch, stream);
}
