// One Adam / AdamW step over all parameters of a group, gfx950 (include/gfla_adam.h).
//
// torch's multi-tensor Adam is a dozen launches per tensor group, and under a GradScaler an unscale pass over every
// gradient plus a host-side decision.  Here a group is one launch over (tensor, chunk of kAdamChunk elements): a
// workgroup finds its record by a uniform binary search over the table's first-chunk column, so small tensors cost one
// mostly idle workgroup each and nothing else.  The unscale and the skip happen in the kernel: every workgroup reads
// found_inf and leaves when it is set.  The step counter is read by every workgroup and written by none: a one-wave
// launch after the main one advances it.
//
// Pure streaming: per element 4 (p) + 4 (g) + 8 (m, unless beta1 == 0: 4) + 8 (v) bytes for float32 storage.  A tensor
// whose addresses are all multiples of 16 moves as float4 (16-bit storage: 8-byte p and g beside 16-byte moments and
// master), two per thread in flight at a time; any other phase of p or g goes by elements.  The arithmetic is one inline function
// for both paths, float32 without contraction, so a tensor's bits do not depend on the path or on its neighbours.
#include "gfla_common.h"

namespace gfla {

constexpr int kAdamQuads = 4;                            // float4 per thread and chunk
constexpr int kAdamFlight = 2;                           // of which in flight at a time: 64 VGPRs, eight waves per SIMD
constexpr int kAdamChunk = kBlock * 4 * kAdamQuads;      // elements per workgroup
constexpr int64_t kAdamMaxTensors = 65535;
constexpr int64_t kAdamMaxElems = 2147483647;
constexpr int64_t kAdamMaxChunks = ((int64_t)1 << 24) - 1;   // grid.x * kBlock stays below 2^32

struct AdamRec {
  int64_t p, g, m, v, master, numel, first_chunk, zero;
};
static_assert(sizeof(AdamRec) == 64, "the table is 8 int64 per tensor");

struct AdamHyper {
  double lr, beta1, beta2;
  float wd, decay, w1, beta2f, w2, eps;
  int decoupled;
};

// what an element needs, the same in every thread of a launch
struct AdamCoef {
  float inv_scale, wd, decay, w1, beta2, w2, neg_step, bc2_sqrt, eps;
  int unscale, decoupled, use_m;
};

// the 16-byte path: every address of the tensor a multiple of 16 (no master: 0)
__host__ __device__ __forceinline__ int adam_vector_path(int64_t p, int64_t g, int64_t m, int64_t v, int64_t master) {
  return ((p | g | m | v | master) & 15) == 0;
}

// b^t for an integer-valued t >= 1, by squaring, in double
__device__ __forceinline__ double adam_pow(double b, float t) {
  double r = 1.0;
  for (uint32_t e = (uint32_t)t; e != 0; e >>= 1) {
    if (e & 1u) r *= b;
    b *= b;
  }
  return r;
}

// torch's _single_tensor_adam on one element, operation by operation
__device__ __forceinline__ void adam_elem(float &p, float g, float &m, float &v, const AdamCoef &c) {
#pragma clang fp contract(off)
  if (c.unscale) g = g * c.inv_scale;
  if (c.decoupled)
    p = p * c.decay;
  else if (c.wd != 0.f)
    g = g + c.wd * p;
  m = c.use_m ? m + (g - m) * c.w1 : g;
  v = c.beta2 * v + (c.w2 * g) * g;
  const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
  p = p + (c.neg_step * m) / denom;
}

__device__ __forceinline__ void adam_quad(float4 &p, const float4 &g, float4 &m, float4 &v, const AdamCoef &c) {
  adam_elem(p.x, g.x, m.x, v.x, c);
  adam_elem(p.y, g.y, m.y, v.y, c);
  adam_elem(p.z, g.z, m.z, v.z, c);
  adam_elem(p.w, g.w, m.w, v.w, c);
}

// four storage elements at a 16-byte (float) / 8-byte (16-bit) boundary, as floats
__device__ __forceinline__ float4 adam_ld4(const float *a) { return *reinterpret_cast<const float4 *>(a); }
template <typename T>
__device__ __forceinline__ float4 adam_ld4(const T *a) {
  const Pack<T, 4> q = *reinterpret_cast<const Pack<T, 4> *>(a);
  return make_float4(Num<T>::ld(&q.v[0]), Num<T>::ld(&q.v[1]), Num<T>::ld(&q.v[2]), Num<T>::ld(&q.v[3]));
}
__device__ __forceinline__ void adam_st4(float *a, const float4 &x) { *reinterpret_cast<float4 *>(a) = x; }
template <typename T>
__device__ __forceinline__ void adam_st4(T *a, const float4 &x) {
  Pack<T, 4> q;
  q.v[0] = Num<T>::from(x.x);
  q.v[1] = Num<T>::from(x.y);
  q.v[2] = Num<T>::from(x.z);
  q.v[3] = Num<T>::from(x.w);
  *reinterpret_cast<Pack<T, 4> *>(a) = q;
}

// the pointers of a record; the float32 value of the parameter lives in the master when there is one, else in p itself
template <typename T>
struct AdamPtrs {
  T *p;
  const T *g;
  float *m, *v, *master;
};

template <typename T>
__device__ __forceinline__ void adam_one(const AdamPtrs<T> &a, int64_t i, const AdamCoef &c) {
  float p = a.master != nullptr ? a.master[i] : Num<T>::ld(a.p + i);
  float m = c.use_m ? a.m[i] : 0.f, v = a.v[i];
  adam_elem(p, Num<T>::ld(a.g + i), m, v, c);
  a.m[i] = m;
  a.v[i] = v;
  if (a.master != nullptr) a.master[i] = p;
  a.p[i] = Num<T>::from(p);
}

template <typename T>
__device__ __forceinline__ void adam_four(const AdamPtrs<T> &a, int64_t i, const AdamCoef &c) {
  float4 p = a.master != nullptr ? adam_ld4(a.master + i) : adam_ld4(a.p + i);
  const float4 g = adam_ld4(a.g + i);
  float4 m = c.use_m ? adam_ld4(a.m + i) : make_float4(0.f, 0.f, 0.f, 0.f), v = adam_ld4(a.v + i);
  adam_quad(p, g, m, v, c);
  adam_st4(a.m + i, m);
  adam_st4(a.v + i, v);
  if (a.master != nullptr) adam_st4(a.master + i, p);
  adam_st4(a.p + i, p);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void adam_step_kernel(const AdamRec *__restrict__ table, int n,
                                                           const float *__restrict__ step,
                                                           const float *__restrict__ grad_scale,
                                                           const float *__restrict__ found_inf, AdamHyper h) {
  if (found_inf != nullptr && *found_inf != 0.f) return;        // the scaler's skip: nothing is stored
  // the last record whose first chunk is not behind this workgroup's: uniform, scalar loads
  const int64_t chunk = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].first_chunk <= chunk)
      lo = mid;
    else
      hi = mid - 1;
  }
  const AdamRec rec = table[lo];
  if (rec.g == 0) return;                                       // no gradient this step
  const int64_t numel = rec.numel;
  const int64_t base = (chunk - rec.first_chunk) * kAdamChunk;
  if (base >= numel) return;

  const float t = *step + 1.f;
  const double bc1 = 1.0 - adam_pow(h.beta1, t), bc2 = 1.0 - adam_pow(h.beta2, t);
  AdamCoef c;
  c.unscale = grad_scale != nullptr;
  c.inv_scale = c.unscale ? 1.f / *grad_scale : 1.f;
  c.wd = h.wd;
  c.decay = h.decay;
  c.decoupled = h.decoupled;
  c.use_m = h.beta1 != 0.0;
  c.w1 = h.w1;
  c.beta2 = h.beta2f;
  c.w2 = h.w2;
  c.eps = h.eps;
  c.neg_step = (float)(-(h.lr / bc1));
  c.bc2_sqrt = (float)sqrt(bc2);

  AdamPtrs<T> a;
  a.p = reinterpret_cast<T *>(rec.p);
  a.g = reinterpret_cast<const T *>(rec.g);
  a.m = reinterpret_cast<float *>(rec.m);
  a.v = reinterpret_cast<float *>(rec.v);
  a.master = reinterpret_cast<float *>(rec.master);
  const int tid = threadIdx.x;

  if (!adam_vector_path(rec.p, rec.g, rec.m, rec.v, rec.master)) {   // the element path: any phase of p and g
    for (int it = 0; it < 4 * kAdamQuads; ++it) {
      const int64_t i = base + it * kBlock + tid;
      if (i < numel) adam_one(a, i, c);
    }
    return;
  }
  if (base + kAdamChunk <= numel) {                             // a whole chunk: 4 kAdamFlight loads in flight, then arithmetic
#pragma unroll 1
    for (int round = 0; round < kAdamQuads; round += kAdamFlight) {
      float4 p[kAdamFlight], g[kAdamFlight], m[kAdamFlight], v[kAdamFlight];
#pragma unroll
      for (int it = 0; it < kAdamFlight; ++it) {
        const int64_t i = base + (int64_t)((round + it) * kBlock + tid) * 4;
        p[it] = a.master != nullptr ? adam_ld4(a.master + i) : adam_ld4(a.p + i);
        g[it] = adam_ld4(a.g + i);
        m[it] = c.use_m ? adam_ld4(a.m + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[it] = adam_ld4(a.v + i);
      }
#pragma unroll
      for (int it = 0; it < kAdamFlight; ++it) {
        const int64_t i = base + (int64_t)((round + it) * kBlock + tid) * 4;
        adam_quad(p[it], g[it], m[it], v[it], c);
        adam_st4(a.m + i, m[it]);
        adam_st4(a.v + i, v[it]);
        if (a.master != nullptr) adam_st4(a.master + i, p[it]);
        adam_st4(a.p + i, p[it]);
      }
    }
    return;
  }
  for (int it = 0; it < kAdamQuads; ++it) {                     // the tensor's last chunk: its tail goes by elements
    const int64_t i = base + (int64_t)(it * kBlock + tid) * 4;
    if (i + 4 <= numel) {
      adam_four(a, i, c);
    } else {
      for (int64_t e = i; e < numel; ++e) adam_one(a, e, c);
    }
  }
}

// after the main launch: the count of steps taken, unless the step was skipped
__global__ void adam_advance_kernel(float *__restrict__ step, const float *__restrict__ found_inf) {
  if (threadIdx.x != 0) return;
  if (found_inf != nullptr && *found_inf != 0.f) return;
  *step = *step + 1.f;
}

// the argument checks of the layout and of the step, in the header's order; total: the chunk count
static int adam_check(const int64_t *numels, int64_t n, int64_t *total) {
  if (numels == nullptr) return GFLA_ERR_NULL_POINTER;
  if (n <= 0) return GFLA_ERR_BAD_SHAPE;
  for (int64_t i = 0; i < n; ++i)
    if (numels[i] <= 0) return GFLA_ERR_BAD_SHAPE;
  if (n > kAdamMaxTensors) return GFLA_ERR_UNSUPPORTED;
  int64_t chunks = 0;
  for (int64_t i = 0; i < n; ++i) {
    if (numels[i] > kAdamMaxElems) return GFLA_ERR_UNSUPPORTED;
    chunks += ceil_div(numels[i], kAdamChunk);
  }
  if (chunks > kAdamMaxChunks) return GFLA_ERR_UNSUPPORTED;
  *total = chunks;
  return GFLA_OK;
}

template <typename T>
static int adam_step(const void *table, const int64_t *numels, int64_t n, float *step, const float *grad_scale,
                     const float *found_inf, double lr, double beta1, double beta2, double eps, double weight_decay,
                     int flags, gfla_stream_t stream) {
  if (table == nullptr || numels == nullptr || step == nullptr) return GFLA_ERR_NULL_POINTER;
  if (n <= 0) return GFLA_ERR_BAD_SHAPE;
  if (!(lr >= 0) || !(eps > 0) || !(beta1 >= 0 && beta1 < 1) || !(beta2 >= 0 && beta2 < 1) || !(weight_decay >= 0) ||
      (flags & ~1) != 0)
    return GFLA_ERR_BAD_SHAPE;
  int64_t chunks = 0;
  const int status = adam_check(numels, n, &chunks);
  if (status != GFLA_OK) return status;
  AdamHyper h;
  h.lr = lr;
  h.beta1 = beta1;
  h.beta2 = beta2;
  h.decoupled = flags & 1;
  h.wd = (float)weight_decay;
  h.decay = (float)(1.0 - lr * weight_decay);
  h.w1 = (float)(1.0 - beta1);
  h.beta2f = (float)beta2;
  h.w2 = (float)(1.0 - beta2);
  h.eps = (float)eps;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adam_step_kernel<T>, dim3((unsigned)chunks), dim3(kBlock), 0, st,
                     static_cast<const AdamRec *>(table), (int)n, step, grad_scale, found_inf, h);
  hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, st, step, found_inf);
  return launch_status();
}

}  // namespace gfla

using namespace gfla;

extern "C" int64_t gfla_adam_chunk_elems(void) { return kAdamChunk; }

extern "C" int gfla_adam_layout(const int64_t *numels, int64_t n, int64_t *first_chunk, int64_t *totals) {
  if (numels == nullptr || first_chunk == nullptr || totals == nullptr) return GFLA_ERR_NULL_POINTER;
  int64_t chunks = 0;
  const int status = adam_check(numels, n, &chunks);
  if (status != GFLA_OK) return status;
  int64_t at = 0;
  for (int64_t i = 0; i < n; ++i) {
    first_chunk[i] = at;
    at += ceil_div(numels[i], kAdamChunk);
  }
  totals[0] = at;
  return GFLA_OK;
}

extern "C" int gfla_adam_vector_path(int64_t p, int64_t g, int64_t m, int64_t v, int64_t master, int elem_size) {
  return (elem_size == 2 || elem_size == 4) && adam_vector_path(p, g, m, v, master) ? 1 : 0;
}

#define GFLA_DEF_ADAM(SFX)                                                                                            \
  extern "C" int gfla_adam_step_##SFX(const void *table, const int64_t *numels, int64_t n, float *step,               \
                                      const float *grad_scale, const float *found_inf, double lr, double beta1,      \
                                      double beta2, double eps, double weight_decay, int flags, gfla_stream_t stream) { \
    return adam_step<elem_##SFX>(table, numels, n, step, grad_scale, found_inf, lr, beta1, beta2, eps, weight_decay,  \
                                 flags, stream);                                                                      \
  }
GFLA_DEF_ADAM(f32)
GFLA_DEF_ADAM(f16)
GFLA_DEF_ADAM(bf16)
#undef GFLA_DEF_ADAM
