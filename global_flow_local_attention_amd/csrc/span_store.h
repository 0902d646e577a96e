// A span of a plane stored 16 bytes at a time, and the generator that turns staged interleaved bytes into normalised
// values: shared by csrc/pose_inputs.hip and csrc/image_inputs.hip.
#pragma once

#include "gfla_common.h"

namespace gfla {

// n elements at dst, any multiple of sizeof(T).  A generator yields the elements in the arithmetic type: seek(k) positions
// it at element k, next() yields that element and moves on by one, pack(q) fills a pack with the V elements at its position
// without moving, jump(m) moves it on by m elements (always kBlock * V here).  A thread divides once, in its first seek.
template <typename T, typename Gen>
__device__ __forceinline__ void store_span(T *dst, int n, Gen &gen) {
  constexpr int V = 16 / (int)sizeof(T);
  const int tid = threadIdx.x;
  int head = (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / sizeof(T));
  if (head > n) head = n;
  if (tid < head) {
    gen.seek(tid);
    dst[tid] = Num<T>::from(gen.next());
  }
  const int nv = (n - head) / V;
  if (tid < nv) gen.seek(head + tid * V);
  for (int v = tid; v < nv; v += kBlock) {
    Pack<T, V> q;
    gen.pack(q);
    *reinterpret_cast<Pack<T, V> *>(dst + head + v * V) = q;
    gen.jump(kBlock * V);
  }
  const int done = head + nv * V;
  if (tid < n - done) {
    gen.seek(done + tid);
    dst[done + tid] = Num<T>::from(gen.next());
  }
}

// ((v / 255) - mean) / std per channel, as float32
struct NormCoef {
  float mean[4], std[4];
};

// lut[c * 256 + v] for thread v of a 256-thread workgroup (the caller synchronises)
__device__ __forceinline__ void norm_lut_fill(float *lut, int C, const NormCoef &coef) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  const float q = (float)tid / 255.f;
  for (int c = 0; c < C; ++c) lut[c * 256 + tid] = (q - coef.mean[c]) / coef.std[c];
}

struct NormGen {
  const uint8_t *px;                                 // this channel's first byte of the staged pixels
  const float *lut;
  int C, at;
  __device__ __forceinline__ void seek(int k) { at = k * C; }
  __device__ __forceinline__ void jump(int m) { at += m * C; }
  __device__ __forceinline__ float next() {
    const float v = lut[px[at]];
    at += C;
    return v;
  }
  template <typename T, int V>
  __device__ __forceinline__ void pack(Pack<T, V> &q) const {
#pragma unroll
    for (int i = 0; i < V; ++i) q.v[i] = Num<T>::from(lut[px[at + i * C]]);
  }
};

}  // namespace gfla
