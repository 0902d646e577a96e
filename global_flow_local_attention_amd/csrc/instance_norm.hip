// Fused InstanceNorm2d (+ affine) + LeakyReLU / ReLU, forward and backward, gfx950.
//
// Per plane (b, c) of N = H W values:
//   mean, rstd = 1 / sqrt(var_biased + eps),  z = (x - mean) rstd gamma[c] + beta[c],  y = z > 0 ? z : slope z
// and, with dz = dy (z > 0 ? 1 : slope), xhat = (x - mean) rstd, s1 = sum dz, s2 = sum dz xhat:
//   dx = rstd gamma (dz - s1 / N - xhat s2 / N),  dgamma[c] = sum_b s2[b,c],  dbeta[c] = sum_b s1[b,c].
// The op is pure memory traffic: the forward reads x once and writes y once, the backward reads x and dy once and writes
// dx once; z is recomputed from x, nothing but (mean, rstd) per plane is kept between the two.
//
// Registers.  A contiguous span of a plane is cut, by the ADDRESS of its first element, into a scalar head up to the next
// 16-byte boundary, 16-byte vectors (4 f32 / 8 f16, bf16 / 2 f64 values) and a scalar tail.  Thread t of the `nth` threads
// that share the span holds vectors t, t + nth, ... (NV of them at most, NV a template parameter) and at most one head or
// tail element, all as stored; they are widened where they are used.  Every load and store of the body is one
// global_load_dwordx4 / global_store_dwordx4 per lane, whole lines per wave.
//
// Three regimes, chosen on the host from (B C, N, element size) alone (in_plan):
//   0  wave per plane      N <= 1024.  Four planes per workgroup, one wave each, butterfly reduction, no LDS, no barrier.
//   1  workgroup per plane 64 .. 1024 threads (about four vectors each; at 1024 threads up to 11 for f32 = 45,056 values,
//                          6 for 16-bit = 49,152, 8 for f64 = 16,384: what 128 registers per thread hold twice over, for
//                          the backward's x and dy, without scratch).
//                          Wave butterfly, one LDS slot per wave, every thread adds the slots in wave order.
//   2  split plane         planes beyond that, and large planes (N >= 16384) when fewer than 256 of them
//                          exist: several workgroups per plane.  Kernel A leaves (count, mean, M2) -- or (sum dz,
//                          sum dz (x - mean), sum (x - mean)) -- per segment in the workspace as float64, kernel B combines them in segment
//                          order (Chan's update, in float64), and applies to its own segment, reading x (and dy) again.
//
// Variance.  Never E[x^2] - mean^2.  m = fl(sum / n); then ONE pass over the registers gives S1 = sum (x - m) and
// S2 = sum (x - m)^2; the mean is m + r with r = S1 / n (m alone is only as good as a float32 sum of n values around
// 1000 can be) and M2 = S2 - S1 r.  The forward normalises with ((x - m) - r): x - m is exact where it matters.
// The saved mean is fl(m + r); the backward finds its own r = sum (x - mean) / N in the same reduction round as s1 and
// s2 and folds it in: s2 = rstd (sum dz (x - mean) - r s1), xhat = ((x - mean) - r) rstd.  The slope side of dz is decided by
// z' = (x - mean) rstd gamma + beta, without r (r is below half a unit in the last place of the mean); z' == 0 takes the
// slope, as leaky_relu_backward does.
//
// No floating-point atomics: s1 and s2 of every plane go to a (B, C, 2) float64 workspace and one thread per channel
// adds them over b in ascending order.  Every sum has an order fixed by the shape and the alignment of the buffers, so
// results are bit-identical from call to call.
#include <algorithm>

#include "gfla_common.h"

namespace gfla {

constexpr int kInWavePlane = 1024;     // regime 0 up to this many values per plane
constexpr int kInWavesPerWg = 4;       // regime 0: planes per workgroup
constexpr int kInMaxThreads = 1024;
constexpr int kInVecPerThread = 4;     // below 1024 threads: grow the workgroup until a thread has about this many
constexpr int64_t kInSplitMinPlane = 16384;   // few planes: split planes of at least this many values ...
constexpr int64_t kInSplitMinSeg = 4096;      // ... into segments of at least this many
constexpr int64_t kInMaxSplit = 4096;         // workgroups per plane (kernel B walks the partials serially)
constexpr int kInMaxWaves = kInMaxThreads / 64;

// 16-byte vectors per thread at most, by element size
constexpr int in_max_nv(int esize) { return esize == 2 ? 6 : esize == 4 ? 11 : 8; }

template <typename T>
struct InV {
  static constexpr int V = 16 / (int)sizeof(T);
  static constexpr int kMaxNV = in_max_nv((int)sizeof(T));
};

// a thread's share of a span, as stored
template <typename T, int NV>
struct InRegs {
  Pack<T, InV<T>::V> v[NV];
  T e;
};

struct InSpan {
  int head, nvec, tail;
};

template <typename T>
__device__ __forceinline__ InSpan in_span(const T *p, int n) {
  InSpan s;
  const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 15);
  s.head = min(mis ? (16 - mis) / (int)sizeof(T) : 0, n);
  s.nvec = (n - s.head) / InV<T>::V;
  s.tail = n - s.head - s.nvec * InV<T>::V;
  return s;
}

// offset of edge element e (head first, then tail) from the span's first element
__device__ __forceinline__ int in_edge_offset(const InSpan &s, int e, int V) {
  return e < s.head ? e : s.head + s.nvec * V + (e - s.head);
}

template <typename T, int NV>
__device__ __forceinline__ void in_load(InRegs<T, NV> &r, const T *p, const InSpan &s, int tid, int nth) {
  constexpr int V = InV<T>::V;
  const Pack<T, V> *pv = reinterpret_cast<const Pack<T, V> *>(p + s.head);
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (tid + j * nth < s.nvec) r.v[j] = pv[tid + j * nth];
  if (tid < s.head + s.tail) r.e = p[in_edge_offset(s, tid, V)];
}

template <typename T, int NV>
__device__ __forceinline__ void in_store(const InRegs<T, NV> &r, T *p, const InSpan &s, int tid, int nth) {
  constexpr int V = InV<T>::V;
  Pack<T, V> *pv = reinterpret_cast<Pack<T, V> *>(p + s.head);
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (tid + j * nth < s.nvec) pv[tid + j * nth] = r.v[j];
  if (tid < s.head + s.tail) p[in_edge_offset(s, tid, V)] = r.e;
}

// f(value) for every value the thread holds
template <typename T, int NV, typename F>
__device__ __forceinline__ void in_each(const InRegs<T, NV> &r, const InSpan &s, int tid, int nth, F f) {
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (tid + j * nth < s.nvec) {
#pragma unroll
      for (int k = 0; k < InV<T>::V; ++k) f(Num<T>::ld(&r.v[j].v[k]));
    }
  if (tid < s.head + s.tail) f(Num<T>::ld(&r.e));
}

// f(a value, b value) over two spans of the same geometry
template <typename T, int NV, typename F>
__device__ __forceinline__ void in_each2(const InRegs<T, NV> &a, const InRegs<T, NV> &b, const InSpan &s, int tid, int nth,
                                         F f) {
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (tid + j * nth < s.nvec) {
#pragma unroll
      for (int k = 0; k < InV<T>::V; ++k) f(Num<T>::ld(&a.v[j].v[k]), Num<T>::ld(&b.v[j].v[k]));
    }
  if (tid < s.head + s.tail) f(Num<T>::ld(&a.e), Num<T>::ld(&b.e));
}

// b value = f(a value, b value), rounded once to the storage type
template <typename T, int NV, typename F>
__device__ __forceinline__ void in_map2(const InRegs<T, NV> &a, InRegs<T, NV> &b, const InSpan &s, int tid, int nth, F f) {
#pragma unroll
  for (int j = 0; j < NV; ++j)
    if (tid + j * nth < s.nvec) {
#pragma unroll
      for (int k = 0; k < InV<T>::V; ++k) b.v[j].v[k] = Num<T>::from(f(Num<T>::ld(&a.v[j].v[k]), Num<T>::ld(&b.v[j].v[k])));
    }
  if (tid < s.head + s.tail) b.e = Num<T>::from(f(Num<T>::ld(&a.e), Num<T>::ld(&b.e)));
}

// Sum of K values over the wave: xor butterfly, every lane ends with the same bits.  Threads add their own values in the
// arithmetic type; everything across threads, and the per-plane scalars derived from the sums, is float64 for every
// storage type (a few dozen operations per plane), so that mean, rstd, s1 and s2 are rounded once.
template <int K>
__device__ __forceinline__ void in_wave_sum(double (&v)[K]) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += __shfl_xor(v[k], o);
  }
}

// ... over the workgroup: one slot per wave in `slots` (kInMaxWaves x K, not reused by the caller), added in wave order
template <int K, bool WAVE>
__device__ __forceinline__ void in_sum(double (&v)[K], double *slots) {
  in_wave_sum(v);
  if (WAVE) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) slots[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = 0;
  for (int w = 0; w < nw; ++w) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] += slots[w * K + k];
  }
}

// which span a thread works on.  MODE 0: blockIdx.x = group of kInWavesPerWg planes, a wave each; 1: blockIdx.x = plane;
// 2: blockIdx.x = plane * wpp + segment.
struct InWhere {
  int64_t plane;
  int seg, off, n, tid, nth;
  bool active;
};
template <int MODE>
__device__ __forceinline__ InWhere in_where(int64_t BC, int N, int seg_len, int wpp) {
  InWhere w;
  w.seg = 0;
  w.off = 0;
  w.n = N;
  w.active = true;
  if (MODE == 0) {
    w.plane = (int64_t)blockIdx.x * kInWavesPerWg + (threadIdx.x >> 6);
    w.tid = threadIdx.x & 63;
    w.nth = 64;
    w.active = w.plane < BC;
  } else if (MODE == 1) {
    w.plane = blockIdx.x;
    w.tid = threadIdx.x;
    w.nth = blockDim.x;
  } else {
    w.plane = blockIdx.x / (unsigned)wpp;
    w.seg = (int)(blockIdx.x - (unsigned)w.plane * (unsigned)wpp);
    w.off = w.seg * seg_len;
    w.n = min(seg_len, N - w.off);
    w.tid = threadIdx.x;
    w.nth = blockDim.x;
  }
  return w;
}

template <typename A>
__device__ __forceinline__ A in_act(A z, A slope, int act) {
  return (act && !(z > (A)0)) ? z * slope : z;
}

// MODE 0 / 1: statistics and y.  MODE 2 (kernel A): the segment's (count, mean, M2) -> partial, float64.
template <typename T, int NV, int MODE>
__global__ __launch_bounds__(MODE == 0 ? 64 * kInWavesPerWg : kInMaxThreads) void in_fwd_kernel(
    const T *__restrict__ x, const typename Num<T>::acc *__restrict__ gamma, const typename Num<T>::acc *__restrict__ beta,
    T *__restrict__ y, typename Num<T>::acc *__restrict__ mean, typename Num<T>::acc *__restrict__ rstd,
    double *__restrict__ partial, int64_t BC, int C, int N, int seg_len, int wpp, double eps,
    typename Num<T>::acc slope, int act) {
  using A = typename Num<T>::acc;
  __shared__ double red0[kInMaxWaves], red1[kInMaxWaves * 2];
  const InWhere w = in_where<MODE>(BC, N, seg_len, wpp);
  if (!w.active) return;
  const T *px = x + w.plane * N + w.off;
  const InSpan sp = in_span(px, w.n);
  InRegs<T, NV> r;
  in_load(r, px, sp, w.tid, w.nth);
  A acc0 = 0;
  in_each(r, sp, w.tid, w.nth, [&](A v) { acc0 += v; });
  double s[1] = {(double)acc0};
  in_sum<1, MODE == 0>(s, red0);
  const A m = (A)(s[0] / (double)w.n);
  A acc1 = 0, acc2 = 0;
  in_each(r, sp, w.tid, w.nth, [&](A v) {
    const A d = v - m;
    acc1 += d;
    acc2 += d * d;
  });
  double q[2] = {(double)acc1, (double)acc2};
  in_sum<2, MODE == 0>(q, red1);
  const double rd = q[0] / (double)w.n, M2 = fmax(q[1] - q[0] * rd, 0.0);
  if (MODE == 2) {
    if (w.tid == 0) {
      double *pp = partial + ((int64_t)blockIdx.x) * 3;
      pp[0] = (double)w.n;
      pp[1] = (double)m + rd;
      pp[2] = M2;
    }
    return;
  }
  const double rsd = 1.0 / sqrt(M2 / (double)w.n + eps);
  if (w.tid == 0) {
    mean[w.plane] = (A)((double)m + rd);
    rstd[w.plane] = (A)rsd;
  }
  const int c = (int)(w.plane % C);
  const A b = beta ? beta[c] : (A)0, k = (A)(rsd * (gamma ? (double)gamma[c] : 1.0)), rr = (A)rd;
  in_map2(r, r, sp, w.tid, w.nth, [&](A v, A) { return in_act(((v - m) - rr) * k + b, slope, act); });
  in_store(r, y + w.plane * N + w.off, sp, w.tid, w.nth);
}

// regime 2, kernel B of the forward: combine the plane's partials in segment order, apply to this segment
template <typename T, int NV>
__global__ __launch_bounds__(kInMaxThreads) void in_fwd_apply_kernel(
    const T *__restrict__ x, const typename Num<T>::acc *__restrict__ gamma, const typename Num<T>::acc *__restrict__ beta,
    T *__restrict__ y, typename Num<T>::acc *__restrict__ mean, typename Num<T>::acc *__restrict__ rstd,
    const double *__restrict__ partial, int C, int N, int seg_len, int wpp, double eps, typename Num<T>::acc slope, int act) {
  using A = typename Num<T>::acc;
  const InWhere w = in_where<2>(0, N, seg_len, wpp);
  const double *pp = partial + w.plane * wpp * 3;
  double cnt = 0, mu = 0, M2 = 0;
  for (int s = 0; s < wpp; ++s) {
    const double nb = pp[3 * s], mb = pp[3 * s + 1], qb = pp[3 * s + 2];
    const double tot = cnt + nb, d = mb - mu;
    mu += d * (nb / tot);
    M2 += qb + d * d * (cnt * nb / tot);
    cnt = tot;
  }
  const double rsd = 1.0 / sqrt(M2 / (double)N + eps);
  const A m = (A)mu, rr = (A)(mu - (double)m);
  if (w.seg == 0 && w.tid == 0) {
    mean[w.plane] = m;
    rstd[w.plane] = (A)rsd;
  }
  const int c = (int)(w.plane % C);
  const A b = beta ? beta[c] : (A)0, k = (A)(rsd * (gamma ? (double)gamma[c] : 1.0));
  const T *px = x + w.plane * N + w.off;
  const InSpan sp = in_span(px, w.n);
  InRegs<T, NV> r;
  in_load(r, px, sp, w.tid, w.nth);
  in_map2(r, r, sp, w.tid, w.nth, [&](A v, A) { return in_act(((v - m) - rr) * k + b, slope, act); });
  in_store(r, y + w.plane * N + w.off, sp, w.tid, w.nth);
}

// dz of one element and its (x - mean): the slope side comes from z' = (x - mean) rstd gamma + beta
template <typename A>
__device__ __forceinline__ A in_dz(A d, A dy, A rs, A g, A b, A slope, int act) {
  const A z = d * rs * g + b;
  return (act && !(z > (A)0)) ? dy * slope : dy;
}

// MODE 0 / 1: (s1, s2) -> s12 (when given) and dx (when given).  MODE 2 (kernel A): the segment's (sum dz, sum dz (x - mean),
// sum (x - mean))
template <typename T, int NV, int MODE>
__global__ __launch_bounds__(MODE == 0 ? 64 * kInWavesPerWg : kInMaxThreads) void in_bwd_kernel(
    const T *__restrict__ x, const T *__restrict__ dy, const typename Num<T>::acc *__restrict__ gamma,
    const typename Num<T>::acc *__restrict__ beta, const typename Num<T>::acc *__restrict__ mean,
    const typename Num<T>::acc *__restrict__ rstd, T *__restrict__ dx, double *__restrict__ s12,
    double *__restrict__ partial, int64_t BC, int C, int N, int seg_len, int wpp, typename Num<T>::acc slope, int act) {
  using A = typename Num<T>::acc;
  __shared__ double red[kInMaxWaves * 3];
  const InWhere w = in_where<MODE>(BC, N, seg_len, wpp);
  if (!w.active) return;
  const T *px = x + w.plane * N + w.off;
  const InSpan sp = in_span(px, w.n);
  InRegs<T, NV> rx, rd;
  in_load(rx, px, sp, w.tid, w.nth);
  in_load(rd, dy + w.plane * N + w.off, sp, w.tid, w.nth);
  const int c = (int)(w.plane % C);
  const A g = gamma ? gamma[c] : (A)1, b = beta ? beta[c] : (A)0;
  const A m = mean[w.plane], rs = rstd[w.plane];
  A acc0 = 0, acc1 = 0, acc2 = 0;
  in_each2(rx, rd, sp, w.tid, w.nth, [&](A v, A gy) {
    const A d = v - m, dz = in_dz(d, gy, rs, g, b, slope, act);
    acc0 += dz;
    acc1 += dz * d;
    acc2 += d;
  });
  double t[3] = {(double)acc0, (double)acc1, (double)acc2};
  in_sum<3, MODE == 0>(t, red);
  if (MODE == 2) {
    if (w.tid == 0) {
      double *pp = partial + ((int64_t)blockIdx.x) * 3;
      pp[0] = t[0];
      pp[1] = t[1];
      pp[2] = t[2];
    }
    return;
  }
  const double r64 = t[2] / (double)N, s1 = t[0], s2 = (double)rs * (t[1] - r64 * s1);
  if (s12 && w.tid == 0) {
    s12[w.plane * 2] = s1;
    s12[w.plane * 2 + 1] = s2;
  }
  if (!dx) return;
  const A rr = (A)r64, a1 = (A)(s1 / (double)N), a2 = (A)(s2 / (double)N), k = rs * g;
  in_map2(rx, rd, sp, w.tid, w.nth, [&](A v, A gy) {
    const A d = v - m, dz = in_dz(d, gy, rs, g, b, slope, act);
    return k * (dz - a1 - ((d - rr) * rs) * a2);
  });
  in_store(rd, dx + w.plane * N + w.off, sp, w.tid, w.nth);
}

// regime 2, kernel B of the backward
template <typename T, int NV>
__global__ __launch_bounds__(kInMaxThreads) void in_bwd_apply_kernel(
    const T *__restrict__ x, const T *__restrict__ dy, const typename Num<T>::acc *__restrict__ gamma,
    const typename Num<T>::acc *__restrict__ beta, const typename Num<T>::acc *__restrict__ mean,
    const typename Num<T>::acc *__restrict__ rstd, T *__restrict__ dx, double *__restrict__ s12,
    const double *__restrict__ partial, int C, int N, int seg_len, int wpp, typename Num<T>::acc slope, int act) {
  using A = typename Num<T>::acc;
  const InWhere w = in_where<2>(0, N, seg_len, wpp);
  if (!dx && w.seg != 0) return;
  const double *pp = partial + w.plane * wpp * 3;
  double t0 = 0, t1 = 0, t2 = 0;
  for (int s = 0; s < wpp; ++s) {
    t0 += pp[3 * s];
    t1 += pp[3 * s + 1];
    t2 += pp[3 * s + 2];
  }
  const A m = mean[w.plane], rs = rstd[w.plane];
  const double rd64 = t2 / (double)N, s2d = (double)rs * (t1 - rd64 * t0);
  if (s12 && w.seg == 0 && w.tid == 0) {
    s12[w.plane * 2] = t0;
    s12[w.plane * 2 + 1] = s2d;
  }
  if (!dx) return;
  const int c = (int)(w.plane % C);
  const A g = gamma ? gamma[c] : (A)1, b = beta ? beta[c] : (A)0;
  const A rr = (A)rd64, a1 = (A)(t0 / (double)N), a2 = (A)(s2d / (double)N), k = rs * g;
  const T *px = x + w.plane * N + w.off;
  const InSpan sp = in_span(px, w.n);
  InRegs<T, NV> rx, rd;
  in_load(rx, px, sp, w.tid, w.nth);
  in_load(rd, dy + w.plane * N + w.off, sp, w.tid, w.nth);
  in_map2(rx, rd, sp, w.tid, w.nth, [&](A v, A gy) {
    const A d = v - m, dz = in_dz(d, gy, rs, g, b, slope, act);
    return k * (dz - a1 - ((d - rr) * rs) * a2);
  });
  in_store(rd, dx + w.plane * N + w.off, sp, w.tid, w.nth);
}

// dgamma[c] = sum_b s2[b,c], dbeta[c] = sum_b s1[b,c]: one thread per channel, b ascending
template <typename A>
__global__ __launch_bounds__(kBlock) void in_dparam_kernel(const double *__restrict__ s12, A *__restrict__ dgamma,
                                                           A *__restrict__ dbeta, int B, int C) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= C) return;
  double s1 = 0, s2 = 0;
  for (int b = 0; b < B; ++b) {
    s1 += s12[((int64_t)b * C + c) * 2];
    s2 += s12[((int64_t)b * C + c) * 2 + 1];
  }
  if (dgamma) dgamma[c] = (A)s2;
  if (dbeta) dbeta[c] = (A)s1;
}

// ---- host: the launch plan, a function of (B C, N, element size) only -------------------------------------------------
struct InPlan {
  int regime, threads, ppw, nv, vpt, lds;
  int64_t wpp, seg_len, nwg;
};

// the instantiated vector counts: 1, 2, 4, then 6 (16-bit) or 8 and 11 (f32) or 8 (f64)
static int in_round_nv(int64_t nv, int esize) {
  return nv <= 1 ? 1 : nv <= 2 ? 2 : nv <= 4 ? 4 : (nv <= 8 && esize != 2) ? 8 : in_max_nv(esize);
}

static int in_plan(int64_t B, int64_t C, int64_t H, int64_t W, int esize, InPlan *p) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (esize != 2 && esize != 4 && esize != 8)) return GFLA_ERR_BAD_SHAPE;
  if (H > 0x7fffffffLL / W || C > 0x7fffffffLL || B > 0x7fffffffLL / C) return GFLA_ERR_UNSUPPORTED;
  const int64_t N = H * W, BC = B * C;
  if (N == 1) return GFLA_ERR_BAD_SHAPE;     // one value per plane has no variance (torch refuses it as well)
  const int V = 16 / esize;
  p->wpp = 1;
  p->seg_len = N;
  if (N <= kInWavePlane) {
    p->regime = 0;
    p->threads = 64 * kInWavesPerWg;
    p->ppw = kInWavesPerWg;
    p->nv = in_round_nv(ceil_div(ceil_div(N, V), 64), esize);
    p->lds = 0;
    p->nwg = ceil_div(BC, kInWavesPerWg);
  } else {
    const int64_t cap = (int64_t)kInMaxThreads * in_max_nv(esize) * V;
    int64_t wpp = ceil_div(N, cap);
    if (BC < kNumCU && N >= kInSplitMinPlane) wpp = std::max(wpp, std::min(ceil_div(2 * kNumCU, BC), N / kInSplitMinSeg));
    if (wpp > 1) {
      p->seg_len = ceil_div(ceil_div(N, wpp), 16) * 16;
      p->wpp = ceil_div(N, p->seg_len);      // (no empty segment)
    }
    if (p->wpp > kInMaxSplit || BC > 0x7fffffffLL / p->wpp) return GFLA_ERR_UNSUPPORTED;
    p->regime = p->wpp > 1 ? 2 : 1;
    const int64_t nvec = ceil_div(p->seg_len, V);
    p->threads = 64;
    while (p->threads < kInMaxThreads && (int64_t)p->threads * kInVecPerThread < nvec) p->threads *= 2;
    p->nv = in_round_nv(ceil_div(nvec, p->threads), esize);
    p->ppw = 1;
    p->lds = kInMaxWaves * 3 * 8;     // one float64 slot per wave and sum
    p->nwg = BC * p->wpp;
  }
  p->vpt = p->nv * V + 1;
  return GFLA_OK;
}

static int64_t in_workspace_bytes(int64_t BC, const InPlan &p) {
  return 8 * (2 * BC + (p.regime == 2 ? 3 * BC * p.wpp : 0));
}

// The kernels take a span's head / vectors / tail from x's address (in_span) and use the same element offsets for y, dy and
// dx: every access stays inside the span whatever the other pointers' phase is, it only is no longer 16-byte aligned there.
// So any pointer aligned to its element is taken (include/gfla_hip.h, "Pointer placement").
template <typename T>
static bool in_element_aligned(const T *p) {
  return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0;
}

// run the statement with NV = the plan's vector count (only the counts in_round_nv gives for T are instantiated)
#define GFLA_IN_CASE(N_, ...)                                    \
  case N_: {                                                     \
    constexpr int NV = N_ <= InV<T>::kMaxNV ? N_ : 1;            \
    __VA_ARGS__;                                                 \
  } break;
#define GFLA_IN_NV(NVAL, ...)                                    \
  switch (NVAL) {                                                \
    GFLA_IN_CASE(1, __VA_ARGS__)                                 \
    GFLA_IN_CASE(2, __VA_ARGS__)                                 \
    GFLA_IN_CASE(4, __VA_ARGS__)                                 \
    GFLA_IN_CASE(6, __VA_ARGS__)                                 \
    GFLA_IN_CASE(8, __VA_ARGS__)                                 \
    GFLA_IN_CASE(11, __VA_ARGS__)                                \
  }

template <typename T>
static int in_fwd(const T *x, const typename Num<T>::acc *gamma, const typename Num<T>::acc *beta, T *y,
                  typename Num<T>::acc *mean, typename Num<T>::acc *rstd, void *workspace, int64_t B, int64_t C, int64_t H,
                  int64_t W, double eps, double slope, int act, gfla_stream_t stream) {
  using A = typename Num<T>::acc;
  if (!x || !y || !mean || !rstd || !workspace) return GFLA_ERR_NULL_POINTER;
  InPlan p;
  if (int rc = in_plan(B, C, H, W, (int)sizeof(T), &p)) return rc;
  if (!(eps >= 0) || !in_element_aligned(x) || !in_element_aligned(y)) return GFLA_ERR_UNSUPPORTED;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t BC = B * C;
  const int N = (int)(H * W), seg = (int)p.seg_len, wpp = (int)p.wpp;
  double *partial = static_cast<double *>(workspace) + 2 * BC;
  const dim3 grid((unsigned)p.nwg);
  if (p.regime == 0) {
    GFLA_IN_NV(p.nv, in_fwd_kernel<T, NV, 0><<<grid, p.threads, 0, st>>>(x, gamma, beta, y, mean, rstd, partial, BC, (int)C, N,
                                                                        seg, wpp, eps, (A)slope, act))
  } else if (p.regime == 1) {
    GFLA_IN_NV(p.nv, in_fwd_kernel<T, NV, 1><<<grid, p.threads, 0, st>>>(x, gamma, beta, y, mean, rstd, partial, BC, (int)C, N,
                                                                        seg, wpp, eps, (A)slope, act))
  } else {
    GFLA_IN_NV(p.nv, in_fwd_kernel<T, NV, 2><<<grid, p.threads, 0, st>>>(x, gamma, beta, y, mean, rstd, partial, BC, (int)C, N,
                                                                        seg, wpp, eps, (A)slope, act);
               in_fwd_apply_kernel<T, NV><<<grid, p.threads, 0, st>>>(x, gamma, beta, y, mean, rstd, partial, (int)C, N, seg,
                                                                     wpp, eps, (A)slope, act))
  }
  return launch_status();
}

template <typename T>
static int in_bwd(const T *x, const T *dy, const typename Num<T>::acc *gamma, const typename Num<T>::acc *beta,
                  const typename Num<T>::acc *mean, const typename Num<T>::acc *rstd, T *dx, typename Num<T>::acc *dgamma,
                  typename Num<T>::acc *dbeta, void *workspace, int64_t B, int64_t C, int64_t H, int64_t W, double slope,
                  int act, gfla_stream_t stream) {
  using A = typename Num<T>::acc;
  if (!x || !dy || !mean || !rstd || !workspace) return GFLA_ERR_NULL_POINTER;
  InPlan p;
  if (int rc = in_plan(B, C, H, W, (int)sizeof(T), &p)) return rc;
  if (!in_element_aligned(x) || !in_element_aligned(dy) || !in_element_aligned(dx)) return GFLA_ERR_UNSUPPORTED;
  if (!dx && !dgamma && !dbeta) return GFLA_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t BC = B * C;
  const int N = (int)(H * W), seg = (int)p.seg_len, wpp = (int)p.wpp;
  double *s12 = (dgamma || dbeta) ? static_cast<double *>(workspace) : nullptr;
  double *partial = static_cast<double *>(workspace) + 2 * BC;
  const dim3 grid((unsigned)p.nwg);
  if (p.regime == 0) {
    GFLA_IN_NV(p.nv, in_bwd_kernel<T, NV, 0><<<grid, p.threads, 0, st>>>(x, dy, gamma, beta, mean, rstd, dx, s12, partial, BC,
                                                                        (int)C, N, seg, wpp, (A)slope, act))
  } else if (p.regime == 1) {
    GFLA_IN_NV(p.nv, in_bwd_kernel<T, NV, 1><<<grid, p.threads, 0, st>>>(x, dy, gamma, beta, mean, rstd, dx, s12, partial, BC,
                                                                        (int)C, N, seg, wpp, (A)slope, act))
  } else {
    GFLA_IN_NV(p.nv, in_bwd_kernel<T, NV, 2><<<grid, p.threads, 0, st>>>(x, dy, gamma, beta, mean, rstd, dx, s12, partial, BC,
                                                                        (int)C, N, seg, wpp, (A)slope, act);
               in_bwd_apply_kernel<T, NV><<<grid, p.threads, 0, st>>>(x, dy, gamma, beta, mean, rstd, dx, s12, partial, (int)C,
                                                                     N, seg, wpp, (A)slope, act))
  }
  if (s12)
    in_dparam_kernel<A><<<dim3((unsigned)ceil_div(C, kBlock)), kBlock, 0, st>>>(s12, dgamma, dbeta, (int)B, (int)C);
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int gfla_instance_norm_geometry(int64_t B, int64_t C, int64_t H, int64_t W, int elem_size, int is_backward, int64_t *out) {
  if (!out) return GFLA_ERR_NULL_POINTER;
  (void)is_backward;     // both directions hold the same number of 16-byte vectors per thread: one plan
  gfla::InPlan p;
  if (int rc = gfla::in_plan(B, C, H, W, elem_size, &p)) return rc;
  out[0] = p.regime;
  out[1] = p.threads;
  out[2] = p.ppw;
  out[3] = p.wpp;
  out[4] = p.vpt;
  out[5] = p.lds;
  out[6] = p.nwg;
  return GFLA_OK;
}

int64_t gfla_instance_norm_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int elem_size) {
  gfla::InPlan p;
  if (int rc = gfla::in_plan(B, C, H, W, elem_size, &p)) return rc;
  return gfla::in_workspace_bytes(B * C, p);
}

#define GFLA_DEF_INSTANCE_NORM(SFX, ABI_T, T, ACC)                                                                            \
  int gfla_instance_norm_fwd_##SFX(const ABI_T *x, const ACC *gamma, const ACC *beta, ABI_T *y, ACC *mean, ACC *rstd,         \
                                   void *workspace, int64_t B, int64_t C, int64_t H, int64_t W, double eps, double slope,     \
                                   int act, gfla_stream_t stream) {                                                           \
    return gfla::in_fwd<T>(reinterpret_cast<const T *>(x), gamma, beta, reinterpret_cast<T *>(y), mean, rstd, workspace, B,  \
                           C, H, W, eps, slope, act, stream);                                                                 \
  }                                                                                                                           \
  int gfla_instance_norm_bwd_##SFX(const ABI_T *x, const ABI_T *dy, const ACC *gamma, const ACC *beta, const ACC *mean,       \
                                   const ACC *rstd, ABI_T *dx, ACC *dgamma, ACC *dbeta, void *workspace, int64_t B,           \
                                   int64_t C, int64_t H, int64_t W, double slope, int act, gfla_stream_t stream) {            \
    return gfla::in_bwd<T>(reinterpret_cast<const T *>(x), reinterpret_cast<const T *>(dy), gamma, beta, mean, rstd,         \
                           reinterpret_cast<T *>(dx), dgamma, dbeta, workspace, B, C, H, W, slope, act, stream);              \
  }
GFLA_DEF_INSTANCE_NORM(f32, float, float, float)
GFLA_DEF_INSTANCE_NORM(f64, double, double, double)
GFLA_DEF_INSTANCE_NORM(f16, uint16_t, f16_t, float)
GFLA_DEF_INSTANCE_NORM(bf16, uint16_t, bf16_t, float)
#undef GFLA_DEF_INSTANCE_NORM
}
