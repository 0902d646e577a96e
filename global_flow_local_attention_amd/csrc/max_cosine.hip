// Best-match cosine similarity for the sampling-correctness loss, gfx950.
//
// Reference: PerceptualCorrectness.calculate_loss, external_function.py:255-268 --
//   source_norm = source / (|source|_c + eps)        [b, Ns, C]
//   target_norm = target / (|target|_c + eps)        [b, C, Nt]
//   correction  = bmm(source_norm, target_norm)      [b, Ns, Nt]   (4096^2 floats per sample at 64x64)
//   correction_max, max_indices = max(correction, dim=1)
// The reference materialises `correction` (2.1 GB at B=32, 64x64) only to reduce it.  Here it never
// leaves the accumulator registers: one workgroup owns 128 target positions of one sample, streams
// all source positions past them in 128-row tiles (f32 MFMA, v_mfma_f32_32x32x2_f32: exact f32,
// 157 TF/s peak) and keeps a running (max, argmax) per lane.  In the MFMA C/D layout a lane holds
// 16 rows of ONE column, so the max over source rows is a register reduction; lanes l / l^32 and the
// two waves stacked along the rows are merged once at the very end.  The norms are applied to the
// accumulators (dot * 1/(|s|+eps), then * 1/(|t|+eps) on the maxima; both factors are positive so
// the max commutes with them), which saves normalised copies of both feature maps.
//
// Work decomposition: a unit = (sample, 128 target columns, a RANGE of source tiles).  The source range is
// split until there are several units per workgroup slot (2 per CU), otherwise B x ceil(Nt/128) units
// quantise badly onto 512 slots (704 units = two rounds, the second 37 % full).  Units merge through one
// 64-bit atomic max per column on (ordered float bits << 32 | ~index), decoded by a small final kernel.
//
// This is the one GEMM-shaped op on the path, hence the one place MFMA is used in this library.
#include "gfla_common.h"

namespace gfla {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTM = 128;  // source positions per tile (rows)
constexpr int kTN = 128;  // target positions per unit (columns)

// (value, index) -> one orderable 64-bit key; ties prefer the lower index.  Any real key is > 0.
__device__ __forceinline__ unsigned long long pack_best(float v, int idx) {
  uint32_t u = __float_as_uint(v);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (uint32_t)(0x7fffffff - idx);
}
__device__ __forceinline__ float unpack_best(unsigned long long key, int *idx) {
  uint32_t u = (uint32_t)(key >> 32);
  u = (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u;
  *idx = 0x7fffffff - (int)(uint32_t)key;
  return __uint_as_float(u);
}

// out[b, n] = 1 / (sqrt(sum_c x[b, c, n]^2) + eps): lanes along n (coalesced), 4 channel slices; float32 sums whatever
// the storage type T (float, f16_t, bf16_t).
// keys != NULL (the target map): also reset the packed maxima of these positions and the sample's first_bad slot.
//
// Non-finite features.  In the reference a position with a NaN or an inf among its channels normalises to a vector with
// a NaN in it (x / (|x| + eps): NaN / NaN, inf / inf), so every similarity it takes part in is NaN, and torch.max
// returns NaN at the FIRST NaN of a column.  The similarity of two finite positions is finite, hence: a column is NaN
// iff its target position is bad (first NaN: row 0) or the sample has a bad source position (first NaN: the first such
// row).  Both are known here, and nothing in the MFMA kernels' loops has to look for a NaN: a bad position gets the
// scale NaN -- its similarities are NaN and are never merged (val > best is false) --, the first bad source position
// of a sample goes to first_bad[b] (keys == NULL: the source map), and max_cosine_finish_kernel puts the NaN and its
// index in place.  Only a sum that is not finite is looked at again, channel by channel: a sum that merely overflowed
// (all features finite) keeps the scale 0 it always had.
template <typename T>
__global__ __launch_bounds__(256) void inv_norm_kernel(const T *__restrict__ x, float *__restrict__ out,
                                                      unsigned long long *__restrict__ keys,
                                                      int *__restrict__ first_bad, int C, int N, float eps) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + lane;
  const int64_t b = blockIdx.y;
  const T *p = x + b * C * (int64_t)N + min(n, N - 1);
  float s = 0.f;
  if (n < N) {
    for (int c = slice; c < C; c += 4) {
      const float v = Num<T>::ld(p + (int64_t)c * N);
      s = fmaf(v, v, s);
    }
  }
  part[slice][lane] = s;
  if (keys && blockIdx.x == 0 && threadIdx.x == 0) first_bad[b] = 0x7fffffff;
  __syncthreads();
  if (slice == 0 && n < N) {
    s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
    float r = 1.f / (sqrtf(s) + eps);
    if (!(s < INFINITY)) {
      bool bad = false;
      for (int c = 0; c < C; ++c) bad |= !(fabsf(Num<T>::ld(p + (int64_t)c * N)) < INFINITY);
      if (bad) {
        r = __uint_as_float(0x7fc00000u);
        if (!keys) atomicMin(&first_bad[b], n);
      }
    }
    out[b * N + n] = r;
    if (keys) keys[b * N + n] = 0ull;
  }
}

// keys -> (best, index).  A column that merged no key (every similarity NaN), a bad target position and a sample with
// a bad source position come out NaN at the index torch.max gives (see inv_norm_kernel); the index is in [0, Ns) always.
__global__ __launch_bounds__(256) void max_cosine_finish_kernel(const unsigned long long *__restrict__ keys,
                                                               const float *__restrict__ rt,
                                                               const int *__restrict__ first_bad,
                                                               float *__restrict__ out_max, int *__restrict__ out_idx,
                                                               int64_t n, int Ns, int Nt) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int idx;
  const unsigned long long key = keys[i];
  const float scale = rt[i];
  float v = unpack_best(key, &idx) * scale;
  const int fb = first_bad[i / Nt];
  if (scale != scale || key == 0ull) {
    v = __uint_as_float(0x7fc00000u);
    idx = 0;
  } else if (fb < Ns) {
    v = __uint_as_float(0x7fc00000u);
    idx = fb;
  }
  out_max[i] = v;
  if (out_idx) out_idx[i] = min(max(idx, 0), Ns - 1);
}

// Four consecutive floats of one channel row.  FAST (rows 16-byte aligned, N % 4 == 0, C % KC == 0): one
// unconditional 16-byte load; a quad past the row end is redirected to the last quad of the row -- those
// rows/columns are masked after the MFMAs (rows -> -inf, columns never merged), so their content is free.
// Otherwise: element-wise, zero beyond the row end / channel count.
template <bool FAST>
__device__ __forceinline__ float4 load_quad(const float *__restrict__ plane, int c, int C, int N, int col) {
  if constexpr (FAST) {
    return *reinterpret_cast<const float4 *>(plane + (int64_t)c * N + min(col, N - 4));
  }
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c >= C) return r;
  const float *row = plane + (int64_t)c * N;
  if (col < N) r.x = row[col];
  if (col + 1 < N) r.y = row[col + 1];
  if (col + 2 < N) r.z = row[col + 2];
  if (col + 3 < N) r.w = row[col + 3];
  return r;
}

// KC: channels per staged chunk.  NW waves = 2 (rows) x NW/2 (columns); a wave owns 64 x (256/NW) outputs.
template <bool FAST, int KC, int NW>
__global__ __launch_bounds__(NW * 64) void max_cosine_kernel(const float *__restrict__ S, const float *__restrict__ T,
                                                        const float *__restrict__ rs,
                                                        unsigned long long *__restrict__ keys, int C, int Ns,
                                                        int Nt, int tilesN, int splitM, int total, int per_xcd) {
  constexpr int kThreads = NW * 64;
  constexpr int kQuads = KC * kTM / 4 / kThreads;  // float4 per thread, operand and chunk
  constexpr int kRowStep = kThreads / 32;          // staging rows covered by one pass of the workgroup
  constexpr int WN = 256 / NW;                     // columns per wave
  constexpr int NJ = WN / 32;                      // 32-column MFMA blocks per wave
  __shared__ float As[2][KC][kTM];
  __shared__ float Bs[2][KC][kTN];
  __shared__ float rsl[2][kTM];
  __shared__ float red_v[kTN];
  __shared__ int red_i[kTN];

  // Workgroups are dealt round-robin to the 8 XCDs: give every XCD a contiguous run of units so the
  // planes of a sample are streamed through ONE L2.  unit -> (sample, column tile, source range).
  const int v = (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD;
  if (v >= total) return;
  const int per_sample = tilesN * splitM;
  const int64_t b = v / per_sample;
  const int rem = v - (int)b * per_sample;
  const int n0 = (rem / splitM) * kTN;
  const int part = rem % splitM;
  const int nM_all = (Ns + kTM - 1) / kTM;
  const int mt0 = (int)((int64_t)nM_all * part / splitM);
  const int mt1 = (int)((int64_t)nM_all * (part + 1) / splitM);

  const float *Sb = S + b * C * (int64_t)Ns;
  const float *Tb = T + b * C * (int64_t)Nt;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave / (NW / 2), wn = wave % (NW / 2);
  const int l31 = lane & 31, kh = lane >> 5;
  const int ld_row = t >> 5, ld_col = (t & 31) * 4;  // staging: rows ld_row + kRowStep * h; 4 floats at ld_col

  const int nK = (C + KC - 1) / KC;
  const int iters = (mt1 - mt0) * nK;

  float4 ra[kQuads], rb[kQuads];
  float rscale = 0.f;
  auto fetch = [&](int it) {
    const int mt = mt0 + it / nK, c0 = (it % nK) * KC;
#pragma unroll
    for (int h = 0; h < kQuads; ++h) {
      ra[h] = load_quad<FAST>(Sb, c0 + ld_row + kRowStep * h, C, Ns, mt * kTM + ld_col);
      rb[h] = load_quad<FAST>(Tb, c0 + ld_row + kRowStep * h, C, Nt, n0 + ld_col);
    }
    if (c0 == 0 && t < kTM) {
      const int m = mt * kTM + t;
      rscale = m < Ns ? rs[b * Ns + m] : 0.f;
    }
  };
  auto stage = [&](int it) {
    const int buf = it & 1;
#pragma unroll
    for (int h = 0; h < kQuads; ++h) {
      *reinterpret_cast<float4 *>(&As[buf][ld_row + kRowStep * h][ld_col]) = ra[h];
      *reinterpret_cast<float4 *>(&Bs[buf][ld_row + kRowStep * h][ld_col]) = rb[h];
    }
    if (it % nK == 0 && t < kTM) rsl[(it / nK) & 1][t] = rscale;
  };

  f32x16 acc[2][NJ];
  float best[NJ];
  int bidx[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    best[j] = -INFINITY;
    bidx[j] = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }

  if (iters > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();

  for (int it = 0; it < iters; ++it) {
    if (it + 1 < iters) fetch(it + 1);

    const int buf = it & 1;
    const float *Ab = &As[buf][kh][wm * 64 + l31];
    const float *Bb = &Bs[buf][kh][wn * WN + l31];
#pragma unroll
    for (int kk = 0; kk < KC; kk += 2) {
      const float a0 = Ab[kk * kTM], a1 = Ab[kk * kTM + 32];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float bj = Bb[kk * kTN + 32 * j];
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bj, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bj, acc[1][j], 0, 0, 0);
      }
    }

    if (it % nK == nK - 1) {
      // rows of this tile are complete: scale by 1/(|s|+eps), fold into the running column maxima.
      // C/D layout: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
      const int lt = it / nK, mt = mt0 + lt;
      const float *sc = rsl[lt & 1];
      const bool ragged = (mt + 1) * kTM > Ns;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
          const int m = mt * kTM + ml;
          const float s = sc[ml];
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            float val = acc[i][j][r] * s;
            if (ragged && m >= Ns) val = -INFINITY;
            if (val > best[j]) {
              best[j] = val;
              bidx[j] = m;
            }
            acc[i][j][r] = 0.f;
          }
        }
    }

    if (it + 1 < iters) stage(it + 1);
    __syncthreads();
  }

  // merge the two row groups of a wave (lanes l, l ^ 32), then the two waves stacked along the rows,
  // then this unit into the global keys
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float ov = __shfl_xor(best[j], 32);
    const int oi = __shfl_xor(bidx[j], 32);
    if (ov > best[j] || (ov == best[j] && oi < bidx[j])) {
      best[j] = ov;
      bidx[j] = oi;
    }
  }
  if (wm == 1 && kh == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      red_v[wn * WN + j * 32 + l31] = best[j];
      red_i[wn * WN + j * 32 + l31] = bidx[j];
    }
  }
  __syncthreads();
  if (wm == 0 && kh == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int nl = wn * WN + j * 32 + l31;
      const float ov = red_v[nl];
      const int oi = red_i[nl];
      if (ov > best[j] || (ov == best[j] && oi < bidx[j])) {
        best[j] = ov;
        bidx[j] = oi;
      }
      const int n = n0 + nl;
      if (n < Nt && best[j] > -INFINITY) atomicMax(&keys[b * Nt + n], pack_best(best[j], bidx[j]));
    }
  }
}

static int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

static int max_cosine(const float *source, const float *target, void *workspace, float *out_max, int32_t *out_idx,
                      int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps, gfla_stream_t stream_) {
  if (!source || !target || !workspace || !out_max) return GFLA_ERR_NULL_POINTER;
  if (B < 0 || C <= 0 || Ns <= 0 || Nt < 0) return GFLA_ERR_BAD_SHAPE;
  if (B == 0 || Nt == 0) return GFLA_OK;
  if (Ns > 0x7fffff00LL || Nt > 0x7fffff00LL || C > 0x7fffff00LL || B > 65535) return GFLA_ERR_UNSUPPORTED;
  const int64_t tilesN = ceil_div(Nt, kTN), nM = ceil_div(Ns, kTM);
  // several units per workgroup slot (2 per CU) so that the tail of the launch is short
  int64_t splitM = 1;
  const int64_t slots = 2 * kNumCU;
  if (tuning(GFLA_TUNE_SPLIT) > 0)
    splitM = tuning(GFLA_TUNE_SPLIT);
  else
    splitM = ceil_div(8 * slots, B * tilesN);  // workgroups start as slots free up: many short units pack best
  if (splitM > nM) splitM = nM;
  if (splitM < 1) splitM = 1;
  const int64_t total = B * tilesN * splitM;
  if (total > 0x7ffffff0LL) return GFLA_ERR_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);

  char *ws = static_cast<char *>(workspace);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
  float *inv_t = reinterpret_cast<float *>(ws + align16(8 * B * Nt));
  float *inv_s = reinterpret_cast<float *>(ws + align16(8 * B * Nt) + align16(4 * B * Nt));
  int *first_bad = reinterpret_cast<int *>(ws + align16(8 * B * Nt) + align16(4 * B * Nt) + align16(4 * B * Ns));

  // the target map first: it resets first_bad, which the source map's pass then lowers
  inv_norm_kernel<float><<<dim3((unsigned)ceil_div(Nt, 64), (unsigned)B), 256, 0, stream>>>(target, inv_t, keys, first_bad,
                                                                                    (int)C, (int)Nt, (float)eps);
  inv_norm_kernel<float><<<dim3((unsigned)ceil_div(Ns, 64), (unsigned)B), 256, 0, stream>>>(source, inv_s, nullptr, first_bad,
                                                                                    (int)C, (int)Ns, (float)eps);
  const int64_t per_xcd = ceil_div(total, kNumXCD);
  const dim3 grid((unsigned)(per_xcd * kNumXCD));
  const bool fast = C % 32 == 0 && Ns % 4 == 0 && Nt % 4 == 0 && Ns >= 4 && Nt >= 4 &&
                    ((reinterpret_cast<uintptr_t>(source) | reinterpret_cast<uintptr_t>(target)) & 15) == 0;
#define GFLA_MC_LAUNCH(FAST_, KC_, NW_)                                                                       \
  max_cosine_kernel<FAST_, KC_, NW_><<<grid, NW_ * 64, 0, stream>>>(source, target, inv_s, keys, (int)C, (int)Ns, \
                                                                    (int)Nt, (int)tilesN, (int)splitM, (int)total, \
                                                                    (int)per_xcd)
  // Measured on MI355X (profiles/r1_max_cosine_variants.txt), B=32 C=256 N=64x64: 4 waves x KC 16: 99 TF/s,
  // 4 x 32: 110, 8 x 16: 115, 8 x 32: 121 (8 waves = 64x32 outputs per wave, 4 waves per SIMD resident).
  if (fast)
    GFLA_MC_LAUNCH(true, 32, 8);
  else
    GFLA_MC_LAUNCH(false, 32, 8);
#undef GFLA_MC_LAUNCH
  max_cosine_finish_kernel<<<dim3((unsigned)ceil_div(B * Nt, 256)), 256, 0, stream>>>(keys, inv_t, first_bad, out_max,
                                                                                     out_idx, B * Nt, (int)Ns, (int)Nt);
  return launch_status();
}


// ------------------------------------------------------------------------------------------------------------------
// 16-bit storage (float16 / bfloat16) on v_mfma_f32_32x32x16_{f16,bf16}.  A product of two f16 or two bf16 values is
// exact in the float32 accumulator, so this evaluates the same rounded features as the float32 kernel would after an
// up-cast, at 16 x the matrix rate and without the float32 copies.
//
// A unit = (sample, TN target columns, a range of source tiles), as above, but the target tile stays RESIDENT in the LDS
// for the unit's lifetime ([c][n] rows exactly as they lie in memory, 16-byte loads along n) and only 128-row source
// tiles stream past it, double-buffered in chunks of 32 channels: at the 16-bit rate a unit that re-read both operands
// per source tile would be bound by the L2.  TN = 256 while C <= 256 (128 KB), 128 while C <= 512; beyond that the
// target is re-staged in passes of 512 channels per source tile (correct for any C, no longer resident).
//
// K = C is the strided axis of both maps, while a lane's MFMA fragment is 8 consecutive k of ONE position: the
// fragments are read with ds_read_b64_tr_b16, which hands lane i of a 16-lane group column i of a 4-row x 16-column
// block.  Within a 32-lane half the two groups read 4 rows x 64 contiguous bytes; the 64-byte segments of a row are
// XOR-ed with (row & 3) so that the four rows fall into the four quarters of the 256-byte bank row (conflict-free; the
// row pitches are multiples of 256 bytes).  The read needs EXEC all ones: nothing in the loop below is lane-dependent.
constexpr int kTM16 = 128;     // source positions per streamed tile
constexpr int kKC16 = 32;      // channels per streamed chunk (two k = 16 steps)
constexpr int kCR16 = 512;     // most channels of a 128-column target tile kept in the LDS
constexpr int kThreads16 = 512;

typedef _Float16 mc_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 mc_bf16x8 __attribute__((ext_vector_type(8)));
typedef short mc_s16x4 __attribute__((ext_vector_type(4)));
typedef short mc_s16x8 __attribute__((ext_vector_type(8)));

// byte offset of 16-bit element (row, col) in an image with `pitch` bytes per row (pitch % 256 == 0)
__device__ __forceinline__ int img_off(int row, int col, int pitch) { return row * pitch + ((col * 2) ^ ((row & 3) << 6)); }

__device__ __forceinline__ mc_s16x8 tr_frag(const unsigned char *p, int pitch) {
  typedef __attribute__((address_space(3))) mc_s16x4 lds_s16x4;
  const mc_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p));
  const mc_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p + 4 * pitch));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

template <typename T>
__device__ __forceinline__ f32x16 mma16(mc_s16x8 a, mc_s16x8 b, f32x16 acc) {
  if constexpr (sizeof(T) == 2 && __is_same(T, f16_t))
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(mc_f16x8, a), __builtin_bit_cast(mc_f16x8, b), acc, 0,
                                                  0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(mc_bf16x8, a), __builtin_bit_cast(mc_bf16x8, b), acc,
                                                   0, 0, 0);
}

// Eight consecutive 16-bit elements of channel row c, columns col .. col + 7 (col % 8 == 0).  FAST (rows 16-byte
// aligned, N % 8 == 0): one 16-byte load; an octet past the row end is redirected to the last octet of the row (those
// source rows are masked to -inf after the MFMAs and those target columns are never merged).  Otherwise element-wise,
// zero beyond the row end.  Channels >= C are zero either way.
template <bool FAST>
__device__ __forceinline__ uint4 load_octet(const uint16_t *__restrict__ plane, int c, int C, int N, int col) {
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (c >= C) return r;
  const uint16_t *row = plane + (int64_t)c * N;
  if constexpr (FAST) {
    return *reinterpret_cast<const uint4 *>(row + min(col, N - 8));
  }
  uint32_t w[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t lo = col + 2 * e < N ? row[col + 2 * e] : 0u;
    const uint32_t hi = col + 2 * e + 1 < N ? row[col + 2 * e + 1] : 0u;
    w[e] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// 8 waves = 2 (rows) x 4 (columns); a wave owns 64 x (TN / 4) outputs.
template <typename T, bool FAST, int TN>
__global__ __launch_bounds__(kThreads16) void max_cosine16_kernel(const uint16_t *__restrict__ S,
                                                                  const uint16_t *__restrict__ Tg,
                                                                  const float *__restrict__ rs,
                                                                  unsigned long long *__restrict__ keys, int C, int Ns,
                                                                  int Nt, int CR, int tilesN, int splitM, int total,
                                                                  int per_xcd) {
  constexpr int WN = TN / 4;       // columns per wave
  constexpr int NJ = WN / 32;      // 32-column MFMA blocks per wave
  constexpr int PA = kTM16 * 2;    // byte pitch of a source chunk row
  constexpr int PB = TN * 2;       // byte pitch of a target row
  constexpr int kOctB = TN / 8;    // 16-byte loads per target row
  extern __shared__ __attribute__((aligned(16))) unsigned char mc_smem[];
  unsigned char *Bs = mc_smem;                               // [CR][TN] 16-bit, swizzled
  unsigned char *As = Bs + CR * PB;                          // [2][kKC16][kTM16] 16-bit, swizzled
  float *rsl = reinterpret_cast<float *>(As + 2 * kKC16 * PA);   // [2][kTM16]
  float *red_v = rsl + 2 * kTM16;                            // [TN]
  int *red_i = reinterpret_cast<int *>(red_v + TN);          // [TN]

  const int v = (blockIdx.x % kNumXCD) * per_xcd + blockIdx.x / kNumXCD;
  if (v >= total) return;
  const int per_sample = tilesN * splitM;
  const int64_t b = v / per_sample;
  const int rem = v - (int)b * per_sample;
  const int n0 = (rem / splitM) * TN;
  const int part = rem % splitM;
  const int nM_all = (Ns + kTM16 - 1) / kTM16;
  const int mt0 = (int)((int64_t)nM_all * part / splitM);
  const int mt1 = (int)((int64_t)nM_all * (part + 1) / splitM);

  const uint16_t *Sb = S + b * C * (int64_t)Ns;
  const uint16_t *Tb = Tg + b * C * (int64_t)Nt;

  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int wm = wave >> 2, wn = wave & 3;
  const int l31 = lane & 31, kh = lane >> 5;
  // transposed read: lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3 of the group's block
  const int tq = (lane & 15) >> 2, tcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  // (one offset per 32-position block: the XOR does not commute with adding a block's 64 bytes)
  int a_off[2], b_off[NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i) a_off[i] = img_off(8 * kh + tq, wm * 64 + i * 32 + tcol, PA);
#pragma unroll
  for (int j = 0; j < NJ; ++j) b_off[j] = img_off(8 * kh + tq, wn * WN + j * 32 + tcol, PB);
  const int ld_row = t >> 4, ld_col = (t & 15) * 8;  // source staging: one octet per thread and chunk

  const int nK = (C + kKC16 - 1) / kKC16;   // chunks per source tile
  const int nKR = CR / kKC16;               // chunks per resident target pass
  const bool resident = nK <= nKR;
  const int iters = (mt1 - mt0) * nK;

  auto stage_target = [&](int cb) {   // channels cb .. cb + CR - 1 of the unit's TN columns
    for (int i = t; i < CR * kOctB; i += kThreads16) {
      const int r = i / kOctB, col = (i % kOctB) * 8;
      *reinterpret_cast<uint4 *>(Bs + img_off(r, col, PB)) = load_octet<FAST>(Tb, cb + r, C, Nt, n0 + col);
    }
  };

  uint4 ra;
  float rscale = 0.f;
  auto fetch = [&](int it) {
    const int mt = mt0 + it / nK, c0 = (it % nK) * kKC16;
    ra = load_octet<FAST>(Sb, c0 + ld_row, C, Ns, mt * kTM16 + ld_col);
    if (c0 == 0 && t < kTM16) {
      const int m = mt * kTM16 + t;
      rscale = m < Ns ? rs[b * Ns + m] : 0.f;
    }
  };
  auto stage = [&](int it) {
    *reinterpret_cast<uint4 *>(As + (it & 1) * kKC16 * PA + img_off(ld_row, ld_col, PA)) = ra;
    if (it % nK == 0 && t < kTM16) rsl[((it / nK) & 1) * kTM16 + t] = rscale;
  };

  f32x16 acc[2][NJ];
  float best[NJ];
  int bidx[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    best[j] = -INFINITY;
    bidx[j] = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }

  if (iters > 0) {
    fetch(0);
    if (resident) stage_target(0);
    stage(0);
  }
  __syncthreads();

  for (int it = 0; it < iters; ++it) {
    const int kc = it % nK;
    if (!resident && kc % nKR == 0) {   // uniform: the next pass of target channels replaces the last one
      __syncthreads();
      stage_target(kc * kKC16);
      __syncthreads();
    }
    if (it + 1 < iters) fetch(it + 1);

    const unsigned char *Ab = As + (it & 1) * kKC16 * PA;
    const unsigned char *Bb = Bs + (kc % nKR) * kKC16 * PB;
#pragma unroll
    for (int kk = 0; kk < kKC16; kk += 16) {   // rows kk + 16 n and + 4 keep (row & 3): the offsets carry over
      const mc_s16x8 a0 = tr_frag(Ab + kk * PA + a_off[0], PA), a1 = tr_frag(Ab + kk * PA + a_off[1], PA);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const mc_s16x8 bj = tr_frag(Bb + kk * PB + b_off[j], PB);
        acc[0][j] = mma16<T>(a0, bj, acc[0][j]);
        acc[1][j] = mma16<T>(a1, bj, acc[1][j]);
      }
    }

    if (kc == nK - 1) {
      // rows of this tile are complete: scale by 1/(|s|+eps), fold into the running column maxima.
      // C/D layout: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
      const int lt = it / nK, mt = mt0 + lt;
      const float *sc = rsl + (lt & 1) * kTM16;
      const bool ragged = (mt + 1) * kTM16 > Ns;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
          const int m = mt * kTM16 + ml;
          const float s = sc[ml];
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            float val = acc[i][j][r] * s;
            if (ragged && m >= Ns) val = -INFINITY;
            if (val > best[j]) {
              best[j] = val;
              bidx[j] = m;
            }
            acc[i][j][r] = 0.f;
          }
        }
    }

    if (it + 1 < iters) stage(it + 1);
    __syncthreads();
  }

  // merge the two row groups of a wave (lanes l, l ^ 32), then the two waves stacked along the rows,
  // then this unit into the global keys
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float ov = __shfl_xor(best[j], 32);
    const int oi = __shfl_xor(bidx[j], 32);
    if (ov > best[j] || (ov == best[j] && oi < bidx[j])) {
      best[j] = ov;
      bidx[j] = oi;
    }
  }
  if (wm == 1 && kh == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      red_v[wn * WN + j * 32 + l31] = best[j];
      red_i[wn * WN + j * 32 + l31] = bidx[j];
    }
  }
  __syncthreads();
  if (wm == 0 && kh == 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int nl = wn * WN + j * 32 + l31;
      const float ov = red_v[nl];
      const int oi = red_i[nl];
      if (ov > best[j] || (ov == best[j] && oi < bidx[j])) {
        best[j] = ov;
        bidx[j] = oi;
      }
      const int n = n0 + nl;
      if (n < Nt && best[j] > -INFINITY) atomicMax(&keys[b * Nt + n], pack_best(best[j], bidx[j]));
    }
  }
}

template <typename T>
static int max_cosine16(const uint16_t *source, const uint16_t *target, void *workspace, float *out_max, int32_t *out_idx,
                        int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps, gfla_stream_t stream_) {
  if (!source || !target || !workspace || !out_max) return GFLA_ERR_NULL_POINTER;
  if (B < 0 || C <= 0 || Ns <= 0 || Nt < 0) return GFLA_ERR_BAD_SHAPE;
  if (B == 0 || Nt == 0) return GFLA_OK;
  if (Ns > 0x7fffff00LL || Nt > 0x7fffff00LL || C > 0x7fffff00LL || B > 65535) return GFLA_ERR_UNSUPPORTED;
  const int64_t Cpad = ceil_div(C, kKC16) * kKC16;
  const int TN = Cpad <= 256 ? 256 : 128;
  const int64_t CR = Cpad < kCR16 ? Cpad : kCR16;
  const int64_t tilesN = ceil_div(Nt, TN), nM = ceil_div(Ns, kTM16);
  // one workgroup per CU while the target tile fills the LDS: several units per slot keep the tail of the launch short,
  // few enough that the one-off load of the resident tile stays small beside the source tiles streamed past it
  int64_t splitM = tuning(GFLA_TUNE_SPLIT) > 0 ? tuning(GFLA_TUNE_SPLIT) : ceil_div(4 * (int64_t)kNumCU, B * tilesN);
  if (splitM > nM) splitM = nM;
  if (splitM < 1) splitM = 1;
  const int64_t total = B * tilesN * splitM;
  if (total > 0x7ffffff0LL) return GFLA_ERR_UNSUPPORTED;
  hipStream_t stream = static_cast<hipStream_t>(stream_);

  char *ws = static_cast<char *>(workspace);
  unsigned long long *keys = reinterpret_cast<unsigned long long *>(ws);
  float *inv_t = reinterpret_cast<float *>(ws + align16(8 * B * Nt));
  float *inv_s = reinterpret_cast<float *>(ws + align16(8 * B * Nt) + align16(4 * B * Nt));
  int *first_bad = reinterpret_cast<int *>(ws + align16(8 * B * Nt) + align16(4 * B * Nt) + align16(4 * B * Ns));
  const T *src_t = reinterpret_cast<const T *>(source), *tgt_t = reinterpret_cast<const T *>(target);
  inv_norm_kernel<T><<<dim3((unsigned)ceil_div(Nt, 64), (unsigned)B), 256, 0, stream>>>(tgt_t, inv_t, keys, first_bad,
                                                                                       (int)C, (int)Nt, (float)eps);
  inv_norm_kernel<T><<<dim3((unsigned)ceil_div(Ns, 64), (unsigned)B), 256, 0, stream>>>(src_t, inv_s, nullptr, first_bad,
                                                                                       (int)C, (int)Ns, (float)eps);
  const int64_t per_xcd = ceil_div(total, kNumXCD);
  const dim3 grid((unsigned)(per_xcd * kNumXCD));
  const bool fast = Ns % 8 == 0 && Nt % 8 == 0 && Ns >= 8 && Nt >= 8 &&
                    ((reinterpret_cast<uintptr_t>(source) | reinterpret_cast<uintptr_t>(target)) & 15) == 0;
  // resident target + two source chunks + the source scales of two tiles + the cross-wave merge
  const size_t lds = (size_t)CR * TN * 2 + 2 * kKC16 * kTM16 * 2 + 2 * kTM16 * 4 + (size_t)TN * 8;
#define GFLA_MC16_LAUNCH(FAST_, TN_)                                                                                  \
  do {                                                                                                                \
    auto kern = max_cosine16_kernel<T, FAST_, TN_>;                                                                   \
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,       \
                              (int)lds);                                                                              \
    kern<<<grid, kThreads16, lds, stream>>>(source, target, inv_s, keys, (int)C, (int)Ns, (int)Nt, (int)CR,           \
                                            (int)tilesN, (int)splitM, (int)total, (int)per_xcd);                      \
  } while (0)
  if (TN == 256) {
    if (fast) GFLA_MC16_LAUNCH(true, 256);
    else GFLA_MC16_LAUNCH(false, 256);
  } else {
    if (fast) GFLA_MC16_LAUNCH(true, 128);
    else GFLA_MC16_LAUNCH(false, 128);
  }
#undef GFLA_MC16_LAUNCH
  max_cosine_finish_kernel<<<dim3((unsigned)ceil_div(B * Nt, 256)), 256, 0, stream>>>(keys, inv_t, first_bad, out_max,
                                                                                     out_idx, B * Nt, (int)Ns, (int)Nt);
  return launch_status();
}

}  // namespace gfla

extern "C" {
int64_t gfla_max_cosine_workspace_bytes(int64_t B, int64_t Ns, int64_t Nt) {
  if (B < 0 || Ns < 0 || Nt < 0) return 0;
  return gfla::align16(8 * B * Nt) + gfla::align16(4 * B * Nt) + gfla::align16(4 * B * Ns) + gfla::align16(4 * B);
}

int gfla_max_cosine_fwd_f32(const float *source, const float *target, void *workspace, float *out_max,
                            int32_t *out_idx, int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps,
                            gfla_stream_t stream) {
  return gfla::max_cosine(source, target, workspace, out_max, out_idx, B, C, Ns, Nt, eps, stream);
}

int gfla_max_cosine_fwd_f16(const uint16_t *source, const uint16_t *target, void *workspace, float *out_max,
                            int32_t *out_idx, int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps,
                            gfla_stream_t stream) {
  return gfla::max_cosine16<gfla::f16_t>(source, target, workspace, out_max, out_idx, B, C, Ns, Nt, eps, stream);
}

int gfla_max_cosine_fwd_bf16(const uint16_t *source, const uint16_t *target, void *workspace, float *out_max,
                             int32_t *out_idx, int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps,
                             gfla_stream_t stream) {
  return gfla::max_cosine16<gfla::bf16_t>(source, target, workspace, out_max, out_idx, B, C, Ns, Nt, eps, stream);
}
}
