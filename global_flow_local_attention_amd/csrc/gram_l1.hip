// Style term of VGGLoss (external_function.py:121-160): L1 distance of two Gram matrices, gfx950.
//
//   F = x.view(B, C, N)      G(x) = F F^T / (N C)      D = G(x) - G(y)      loss = mean |D|  over B C^2 entries
//   d loss / d F_x = +g 2 / (B C^3 N) S F_x ,   d loss / d F_y = -g 2 / (B C^3 N) S F_y ,   S = sign(D)  (symmetric)
//
// The reference forms both Grams with bmm (16-bit under torch.autocast: an entry overflows float16 beyond 65504 and is
// rounded at 2^-11 / 2^-8 BEFORE the two nearly equal matrices are subtracted).  Here the features are read as stored
// and every sum is float32: a product of two f16 / bf16 values is exact in the accumulator of
// v_mfma_f32_32x32x16_{f16,bf16}; float32 features use v_mfma_f32_32x32x2_f32.
//
// Forward.  K = N is the contiguous axis of both operands, so a lane's fragment (8 consecutive k of one channel, or 4 for
// float32) is 16 consecutive bytes of a staged row: no transposition.  The output is only C x C per sample against K up
// to 16384, so N is cut into chunks; a workgroup owns (side x|y, sample, 128 x 128 tile on or above the diagonal, chunk)
// and writes its partial tile to the workspace.  Inside a chunk the accumulators are folded into a second set every 256
// k, which keeps the float32 rounding of a long sum of non-negative products at the level of a short one.  The finishing
// kernel adds the chunks of G(x) and of G(y) separately and in the same order (x == y gives D = 0 exactly), scales by
// 1/(N C), writes D and its mirror image (D is symmetric bit for bit) and reduces |D| into one float64 slot per
// workgroup; a one-workgroup kernel adds the slots in a fixed order.  No atomics: bit-identical from call to call.
//
// Backward.  grad = +-coef S F: M = C, K = C, N = HW.  S is rebuilt from the saved D while it is staged; its entries
// -1, 0, +1 are exact in every storage type, so the product loses nothing to operand rounding.  K is the strided axis
// of F: 16-bit fragments are read with ds_read_b64_tr_b16 from rows laid out as in memory (the layout of the 16-bit
// best-match kernel, csrc/max_cosine.hip); float32 fragments are four scalar reads.  grad_loss is a device scalar.
#include "gfla_common.h"

namespace gfla {

typedef float gl_f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 gl_f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 gl_bf16x8 __attribute__((ext_vector_type(8)));
typedef short gl_s16x4 __attribute__((ext_vector_type(4)));
typedef short gl_s16x8 __attribute__((ext_vector_type(8)));

constexpr int kGT = 128;                  // output tile: kGT x kGT, 4 waves = 2 x 2, a wave owns 64 x 64
constexpr int kGRowB = 128;               // bytes of one staged row of a K-contiguous operand: 64 16-bit k, 32 float k
constexpr int kGPitch = kGRowB + 16;      // 36 banks per row: the 16 rows of a ds_read_b128 pass cover the 64 banks once
constexpr int kGFold = 256;               // k between two folds of the accumulators
constexpr int kGChunkUnit = 64;           // chunks are whole multiples of 64 k in every storage type
constexpr int kGMinChunk = 4;             // shortest chunk, in units
constexpr int kGOpBytes = kGT * kGPitch;  // one staged K-contiguous operand
constexpr int64_t kGMaxC = 4096, kGMaxN = 1 << 24, kGMaxB = 16384;

template <typename T>
constexpr int seg_elems() { return 16 / (int)sizeof(T); }

// 16 bytes of `row` (of `rows`, `ld` elements apart) from element k on; zero past kend and for rows >= rows.
// vec: every row starts 16-byte aligned and k is a multiple of the segment.
template <typename T>
__device__ __forceinline__ uint4 load_seg(const T *__restrict__ base, int row, int rows, int64_t ld, int k, int kend,
                                          bool vec) {
  constexpr int E = seg_elems<T>();
  uint4 r = make_uint4(0u, 0u, 0u, 0u);
  if (row >= rows || k >= kend) return r;
  const T *p = base + (int64_t)row * ld + k;
  if (vec && k + E <= kend) return *reinterpret_cast<const uint4 *>(p);
  T e[E];
  __builtin_memset(e, 0, sizeof(e));
#pragma unroll
  for (int i = 0; i < E; ++i)
    if (k + i < kend) e[i] = p[i];
  __builtin_memcpy(&r, e, 16);
  return r;
}

// acc += a b over the 16 bytes of k both lanes hold (the same k in both)
template <typename T>
__device__ __forceinline__ gl_f32x16 gram_mma(uint4 a, uint4 b, gl_f32x16 acc) {
  if constexpr (__is_same(T, float)) {
    const float4 fa = __builtin_bit_cast(float4, a), fb = __builtin_bit_cast(float4, b);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.x, fb.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.y, fb.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa.z, fb.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(fa.w, fb.w, acc, 0, 0, 0);
  } else if constexpr (__is_same(T, f16_t)) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(gl_f16x8, a), __builtin_bit_cast(gl_f16x8, b), acc, 0,
                                                  0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gl_bf16x8, a), __builtin_bit_cast(gl_bf16x8, b), acc,
                                                   0, 0, 0);
  }
}

// (ti, tj), ti <= tj, of the t-th tile on or above the diagonal of a T x T grid, rows first
__device__ __forceinline__ void tri_tile(int t, int T, int &ti, int &tj) {
  ti = 0;
  while (t >= T - ti) {
    t -= T - ti;
    ++ti;
  }
  tj = ti + t;
}
static int64_t tri_count(int64_t T) { return T * (T + 1) / 2; }

// N in units of 64 k -> units per chunk and number of chunks: enough workgroups for two per CU, no chunk under 256 k
static void gram_chunks(int64_t B, int64_t C, int64_t N, int64_t &per, int64_t &chunks) {
  const int64_t units = ceil_div(N, kGChunkUnit), tiles = tri_count(ceil_div(C, kGT));
  int64_t want = ceil_div(2 * (int64_t)kNumCU, 2 * B * tiles);
  const int64_t most = units / kGMinChunk > 0 ? units / kGMinChunk : 1;
  if (want > most) want = most;
  if (want < 1) want = 1;
  per = ceil_div(units, want);
  chunks = ceil_div(units, per);
}

// partial[(side B + b), chunk, tile][128][128] = F[ti rows, chunk] F[tj rows, chunk]^T
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void gram_partial_kernel(const T *__restrict__ x, const T *__restrict__ y,
                                                              float *__restrict__ partial, int B, int C, int N,
                                                              int tilesC, int per, bool vec) {
  constexpr int E = seg_elems<T>();
  constexpr int KE = kGRowB / (int)sizeof(T);         // k per staged chunk
  constexpr int kFoldIt = kGFold / KE;
  constexpr int kSegs = kGT * (kGRowB / 16) / kBlock;   // 16-byte segments per thread and operand
  extern __shared__ __attribute__((aligned(16))) unsigned char gl_smem[];
  unsigned char *As = gl_smem;                 // [2][kGT] rows of kGPitch bytes
  unsigned char *Bs = gl_smem + 2 * kGOpBytes;

  const int chunk = blockIdx.x, tile = blockIdx.y, sb = blockIdx.z;
  int ti, tj;
  tri_tile(tile, tilesC, ti, tj);
  const T *F = (sb >= B ? y : x) + (int64_t)(sb >= B ? sb - B : sb) * C * (int64_t)N;
  const int rowsA = C - ti * kGT, rowsB = C - tj * kGT;     // > 0; rows beyond them are zero
  const T *FA = F + (int64_t)ti * kGT * N, *FB = F + (int64_t)tj * kGT * N;
  const int k_lo = chunk * per * kGChunkUnit;
  const int k_hi = min(k_lo + per * kGChunkUnit, N);
  const int iters = (k_hi - k_lo + KE - 1) / KE;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, kh = lane >> 5;

  uint4 ra[kSegs], rb[kSegs];
  auto fetch = [&](int it) {
    const int k0 = k_lo + it * KE;
#pragma unroll
    for (int h = 0; h < kSegs; ++h) {
      const int seg = t + kBlock * h, row = seg >> 3, k = k0 + (seg & 7) * E;
      ra[h] = load_seg<T>(FA, row, rowsA, N, k, k_hi, vec);
      rb[h] = load_seg<T>(FB, row, rowsB, N, k, k_hi, vec);
    }
  };
  auto stage = [&](int it) {
    const int buf = (it & 1) * kGOpBytes;
#pragma unroll
    for (int h = 0; h < kSegs; ++h) {
      const int seg = t + kBlock * h, off = buf + (seg >> 3) * kGPitch + (seg & 7) * 16;
      *reinterpret_cast<uint4 *>(As + off) = ra[h];
      *reinterpret_cast<uint4 *>(Bs + off) = rb[h];
    }
  };

  gl_f32x16 acc[2][2], sum[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = sum[i][j][r] = 0.f;

  if (iters > 0) {
    fetch(0);
    stage(0);
  }
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    if (it + 1 < iters) fetch(it + 1);
    const int buf = (it & 1) * kGOpBytes;
    const unsigned char *Ab = As + buf + (wm * 64 + l31) * kGPitch + kh * 16;
    const unsigned char *Bb = Bs + buf + (wn * 64 + l31) * kGPitch + kh * 16;
#pragma unroll
    for (int s = 0; s < kGRowB; s += 32) {
      const uint4 a0 = *reinterpret_cast<const uint4 *>(Ab + s), a1 = *reinterpret_cast<const uint4 *>(Ab + 32 * kGPitch + s);
      const uint4 b0 = *reinterpret_cast<const uint4 *>(Bb + s), b1 = *reinterpret_cast<const uint4 *>(Bb + 32 * kGPitch + s);
      acc[0][0] = gram_mma<T>(a0, b0, acc[0][0]);
      acc[0][1] = gram_mma<T>(a0, b1, acc[0][1]);
      acc[1][0] = gram_mma<T>(a1, b0, acc[1][0]);
      acc[1][1] = gram_mma<T>(a1, b1, acc[1][1]);
    }
    if (it % kFoldIt == kFoldIt - 1 || it == iters - 1) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            sum[i][j][r] += acc[i][j][r];
            acc[i][j][r] = 0.f;
          }
    }
    if (it + 1 < iters) stage(it + 1);
    __syncthreads();
  }

  // C/D layout: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).  The whole tile is written (rows and
  // columns >= C are zero), so the finishing kernel never meets an unwritten float.
  float *P = partial + (((int64_t)sb * gridDim.x + chunk) * gridDim.y + tile) * (kGT * kGT);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh, col = wn * 64 + j * 32 + l31;
        P[row * kGT + col] = sum[i][j][r];
      }
}

// One thread per (b, i, j): i <= j adds the chunks of G(x) and of G(y), writes D[i][j] and D[j][i] and counts |D| once
// on the diagonal, twice off it.  slots[workgroup] = the workgroup's sum.
__global__ __launch_bounds__(kBlock) void gram_finish_kernel(const float *__restrict__ partial, float *__restrict__ diff,
                                                             double *__restrict__ slots, int B, int C, int tilesC,
                                                             int chunks, int ntri, float inv_nc) {
  __shared__ double red[kBlock];
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  double mine = 0;
  if (e < (int64_t)B * C * C) {
    const int b = (int)(e / ((int64_t)C * C));
    const int ij = (int)(e - (int64_t)b * C * C), i = ij / C, j = ij - i * C;
    if (i <= j) {
      const int ti = i / kGT, tj = j / kGT;
      const int tile = ti * tilesC - ti * (ti - 1) / 2 + (tj - ti);
      const int64_t at = (int64_t)tile * (kGT * kGT) + (i - ti * kGT) * kGT + (j - tj * kGT);
      const int64_t step = (int64_t)ntri * (kGT * kGT);
      const float *px = partial + (int64_t)b * chunks * step + at;
      const float *py = partial + (int64_t)(B + b) * chunks * step + at;
      float gx = 0.f, gy = 0.f;
      for (int c = 0; c < chunks; ++c) {
        gx += px[c * step];
        gy += py[c * step];
      }
      float d;
      {
        // two rounded products, then the difference: contracted into an fma (one product exact, the other rounded),
        // x == y would leave the rounding of G(y) in D instead of exactly 0
#pragma clang fp contract(off)
        const float sx = gx * inv_nc, sy = gy * inv_nc;
        d = sx - sy;
      }
      float *Db = diff + (int64_t)b * C * C;
      Db[i * C + j] = d;
      if (i != j) Db[j * C + i] = d;
      mine = (i != j ? 2.0 : 1.0) * (double)fabsf(d);
    }
  }
  red[threadIdx.x] = mine;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) slots[blockIdx.x] = red[0];
}

// loss = scale * sum(slots[0..n)), one workgroup, fixed order
__global__ __launch_bounds__(kBlock) void gram_sum_kernel(const double *__restrict__ slots, int64_t n, double scale,
                                                          float *__restrict__ loss) {
  __shared__ double red[kBlock];
  double s = 0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) s += slots[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(red[0] * scale);
}

// ---- backward -----------------------------------------------------------------------------------------------------
// sign(d) in T's bits; NaN -> 0
template <typename T>
__device__ __forceinline__ T sign_of(float d) {
  const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if constexpr (__is_same(T, float)) return s;
  else return T(s);
}

// byte offset of 16-bit element (row, col) of the [k][n] image, 256 bytes per row: the 64-byte segments of a row are
// XOR-ed with (row & 3) so that the four rows of a transposed read fall into the four quarters of the bank row
__device__ __forceinline__ int gl_img_off(int row, int col) { return row * 256 + ((col * 2) ^ ((row & 3) << 6)); }

__device__ __forceinline__ uint4 gl_tr_frag(const unsigned char *p) {
  typedef __attribute__((address_space(3))) gl_s16x4 lds_s16x4;
  const gl_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p));
  const gl_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4 *)(p + 4 * 256));
  return __builtin_bit_cast(uint4, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

constexpr int kGPitchF = kGT + 8;   // floats per row of the float32 [k][n] image: rows k and k + 4 are 32 banks apart

// grad[b, c, n] = (negate ? -1 : 1) grad_loss coef sum_k sign(D[b, c, k]) F[b, k, n]; a workgroup owns 128 c x 128 n
template <typename T>
__global__ __launch_bounds__(kBlock) void gram_bwd_kernel(const T *__restrict__ feat, const float *__restrict__ diff,
                                                          const float *__restrict__ grad_loss, T *__restrict__ grad,
                                                          int C, int N, float coef, bool vec) {
  constexpr bool kF32 = __is_same(T, float);
  constexpr int E = seg_elems<T>();
  constexpr int KE = kGRowB / (int)sizeof(T);              // k per staged chunk: 64 (16-bit) or 32
  constexpr int kSegs = kGT * (kGRowB / 16) / kBlock;      // 4 per thread for S, and 4 for F
  constexpr int kRowSegs = kGT / E;                        // 16-byte segments along n in a row of F
  constexpr int kImgB = kF32 ? KE * kGPitchF * 4 : KE * 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char gl_smem[];
  unsigned char *As = gl_smem;                  // S: [2][kGT] rows of kGPitch bytes, k contiguous
  unsigned char *Bs = gl_smem + 2 * kGOpBytes;  // F: [2][KE] rows along n

  const int n0 = blockIdx.x * kGT, c0 = blockIdx.y * kGT;
  const int64_t b = blockIdx.z;
  const float *Db = diff + b * C * (int64_t)C + (int64_t)c0 * C;
  const T *Fb = feat + b * C * (int64_t)N;
  const int rowsA = C - c0;
  const bool vecD = C % 4 == 0;   // rows of D are whole float4s: 16-byte aligned where `diff` is, the same loads unaligned elsewhere

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, kh = lane >> 5;
  const int iters = (C + KE - 1) / KE;

  uint4 ra[kSegs], rb[kSegs];
  auto fetch = [&](int it) {
    const int k0 = it * KE;
#pragma unroll
    for (int h = 0; h < kSegs; ++h) {
      const int seg = t + kBlock * h;
      {   // E signs of row (seg >> 3) of this c tile
        const int row = seg >> 3, k = k0 + (seg & 7) * E;
        T s[E];
#pragma unroll
        for (int q = 0; q < E; q += 4) {
          const uint4 d = load_seg<float>(Db, row, rowsA, C, k + q, C, vecD);
          const float4 f = __builtin_bit_cast(float4, d);
          s[q] = sign_of<T>(f.x);
          s[q + 1] = sign_of<T>(f.y);
          s[q + 2] = sign_of<T>(f.z);
          s[q + 3] = sign_of<T>(f.w);
        }
        __builtin_memcpy(&ra[h], s, 16);
      }
      const int row = seg / kRowSegs, col = (seg % kRowSegs) * E;
      rb[h] = load_seg<T>(Fb, k0 + row, C, N, n0 + col, N, vec);
    }
  };
  auto stage = [&](int it) {
    const int buf = it & 1;
#pragma unroll
    for (int h = 0; h < kSegs; ++h) {
      const int seg = t + kBlock * h;
      *reinterpret_cast<uint4 *>(As + buf * kGOpBytes + (seg >> 3) * kGPitch + (seg & 7) * 16) = ra[h];
      const int row = seg / kRowSegs, col = (seg % kRowSegs) * E;
      if constexpr (kF32)
        *reinterpret_cast<uint4 *>(Bs + buf * kImgB + (row * kGPitchF + col) * 4) = rb[h];
      else
        *reinterpret_cast<uint4 *>(Bs + buf * kImgB + gl_img_off(row, col)) = rb[h];
    }
  };

  gl_f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // transposed read: lane 4q + p of a 16-lane group supplies row q, columns 4p .. 4p + 3 of the group's block
  const int tq = (lane & 15) >> 2, tcol = ((lane >> 4) & 1) * 16 + (lane & 3) * 4;
  int b_off[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
    b_off[j] = kF32 ? ((4 * kh) * kGPitchF + wn * 64 + j * 32 + l31) * 4 : gl_img_off(8 * kh + tq, wn * 64 + j * 32 + tcol);

  fetch(0);
  stage(0);
  __syncthreads();
  for (int it = 0; it < iters; ++it) {
    if (it + 1 < iters) fetch(it + 1);
    const int buf = it & 1;
    const unsigned char *Ab = As + buf * kGOpBytes + (wm * 64 + l31) * kGPitch + kh * 16;
    const unsigned char *Bb = Bs + buf * kImgB;
#pragma unroll
    for (int s = 0; s < kGRowB / 32; ++s) {   // 16 k (16-bit) or 8 k (float32) per step
      const uint4 a0 = *reinterpret_cast<const uint4 *>(Ab + 32 * s), a1 = *reinterpret_cast<const uint4 *>(Ab + 32 * kGPitch + 32 * s);
      uint4 bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if constexpr (kF32) {
          // k = 8 s + 4 kh + {0..3}: the four floats S holds for this lane
          const float *p = reinterpret_cast<const float *>(Bb + b_off[j]) + 8 * s * kGPitchF;
          bf[j] = __builtin_bit_cast(uint4, make_float4(p[0], p[kGPitchF], p[2 * kGPitchF], p[3 * kGPitchF]));
        } else {
          bf[j] = gl_tr_frag(Bb + 16 * s * 256 + b_off[j]);   // rows + 16 s keep (row & 3): the offset carries over
        }
      }
      acc[0][0] = gram_mma<T>(a0, bf[0], acc[0][0]);
      acc[0][1] = gram_mma<T>(a0, bf[1], acc[0][1]);
      acc[1][0] = gram_mma<T>(a1, bf[0], acc[1][0]);
      acc[1][1] = gram_mma<T>(a1, bf[1], acc[1][1]);
    }
    if (it + 1 < iters) stage(it + 1);
    __syncthreads();
  }

  const float scale = *grad_loss * coef;
  T *Gb = grad + b * C * (int64_t)N;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = c0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh, n = n0 + wn * 64 + j * 32 + l31;
        if (c < C && n < N) Gb[(int64_t)c * N + n] = (T)(acc[i][j][r] * scale);
      }
}

static int gram_check(int64_t B, int64_t C, int64_t N) {
  if (B <= 0 || C <= 0 || N <= 0) return GFLA_ERR_BAD_SHAPE;
  if (B > kGMaxB || C > kGMaxC || N > kGMaxN) return GFLA_ERR_UNSUPPORTED;
  return GFLA_OK;
}

static int64_t gram_finish_blocks(int64_t B, int64_t C) { return ceil_div(B * C * C, kBlock); }

static int64_t gram_partial_bytes(int64_t B, int64_t C, int64_t N) {
  int64_t per, chunks;
  gram_chunks(B, C, N, per, chunks);
  return 2 * B * chunks * tri_count(ceil_div(C, kGT)) * kGT * kGT * (int64_t)sizeof(float);
}

template <typename T>
static bool rows_aligned(const void *p, const void *q, int64_t N) {
  return N % seg_elems<T>() == 0 && ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) == 0;
}

template <typename T>
static int gram_fwd(const T *x, const T *y, void *workspace, float *diff, float *loss, int64_t B, int64_t C, int64_t N,
                    gfla_stream_t stream) {
  if (!x || !y || !workspace || !diff || !loss) return GFLA_ERR_NULL_POINTER;
  if (int rc = gram_check(B, C, N)) return rc;
  int64_t per, chunks;
  gram_chunks(B, C, N, per, chunks);
  const int64_t tilesC = ceil_div(C, kGT), ntri = tri_count(tilesC);
  if (chunks > 0x7fffffffLL || ntri > 65535 || 2 * B > 65535) return GFLA_ERR_UNSUPPORTED;
  float *partial = static_cast<float *>(workspace);
  double *slots = reinterpret_cast<double *>(static_cast<char *>(workspace) + gram_partial_bytes(B, C, N));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t lds = 4 * kGOpBytes;
  auto kern = gram_partial_kernel<T>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<dim3((unsigned)chunks, (unsigned)ntri, (unsigned)(2 * B)), kBlock, lds, st>>>(
      x, y, partial, (int)B, (int)C, (int)N, (int)tilesC, (int)per, rows_aligned<T>(x, y, N));
  const int64_t blocks = gram_finish_blocks(B, C);
  gram_finish_kernel<<<dim3((unsigned)blocks), kBlock, 0, st>>>(partial, diff, slots, (int)B, (int)C, (int)tilesC,
                                                                (int)chunks, (int)ntri,
                                                                (float)(1.0 / ((double)N * (double)C)));
  gram_sum_kernel<<<1, kBlock, 0, st>>>(slots, blocks, 1.0 / ((double)B * (double)C * (double)C), loss);
  return launch_status();
}

template <typename T>
static int gram_bwd(const T *feat, const float *diff, const float *grad_loss, T *grad_feat, int64_t B, int64_t C, int64_t N,
                    int negate, gfla_stream_t stream) {
  if (!feat || !diff || !grad_loss || !grad_feat) return GFLA_ERR_NULL_POINTER;
  if (int rc = gram_check(B, C, N)) return rc;
  const int64_t tilesN = ceil_div(N, kGT), tilesC = ceil_div(C, kGT);
  if (B > 65535 || tilesC > 65535) return GFLA_ERR_UNSUPPORTED;
  constexpr bool kF32 = __is_same(T, float);
  constexpr int KE = kGRowB / (int)sizeof(T);
  const size_t lds = 2 * kGOpBytes + 2 * (kF32 ? KE * kGPitchF * 4 : KE * 256);
  const double coef = (negate ? -2.0 : 2.0) / ((double)B * (double)C * (double)C * (double)C * (double)N);
  auto kern = gram_bwd_kernel<T>;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<dim3((unsigned)tilesN, (unsigned)tilesC, (unsigned)B), kBlock, lds, static_cast<hipStream_t>(stream)>>>(
      feat, diff, grad_loss, grad_feat, (int)C, (int)N, (float)coef, rows_aligned<T>(feat, grad_feat, N));
  return launch_status();
}

}  // namespace gfla

using gfla::bf16_t;
using gfla::f16_t;

extern "C" {
int64_t gfla_gram_l1_workspace_bytes(int64_t B, int64_t C, int64_t N) {
  if (int rc = gfla::gram_check(B, C, N)) return rc;
  return gfla::gram_partial_bytes(B, C, N) + gfla::gram_finish_blocks(B, C) * (int64_t)sizeof(double);
}

int gfla_gram_l1_fwd_f32(const float *x, const float *y, void *workspace, float *diff, float *loss, int64_t B, int64_t C,
                         int64_t N, gfla_stream_t stream) {
  return gfla::gram_fwd<float>(x, y, workspace, diff, loss, B, C, N, stream);
}
int gfla_gram_l1_fwd_f16(const uint16_t *x, const uint16_t *y, void *workspace, float *diff, float *loss, int64_t B,
                         int64_t C, int64_t N, gfla_stream_t stream) {
  return gfla::gram_fwd<f16_t>(reinterpret_cast<const f16_t *>(x), reinterpret_cast<const f16_t *>(y), workspace, diff,
                               loss, B, C, N, stream);
}
int gfla_gram_l1_fwd_bf16(const uint16_t *x, const uint16_t *y, void *workspace, float *diff, float *loss, int64_t B,
                          int64_t C, int64_t N, gfla_stream_t stream) {
  return gfla::gram_fwd<bf16_t>(reinterpret_cast<const bf16_t *>(x), reinterpret_cast<const bf16_t *>(y), workspace, diff,
                                loss, B, C, N, stream);
}

int gfla_gram_l1_bwd_f32(const float *feat, const float *diff, const float *grad_loss, float *grad_feat, int64_t B,
                         int64_t C, int64_t N, int negate, gfla_stream_t stream) {
  return gfla::gram_bwd<float>(feat, diff, grad_loss, grad_feat, B, C, N, negate, stream);
}
int gfla_gram_l1_bwd_f16(const uint16_t *feat, const float *diff, const float *grad_loss, uint16_t *grad_feat, int64_t B,
                         int64_t C, int64_t N, int negate, gfla_stream_t stream) {
  return gfla::gram_bwd<f16_t>(reinterpret_cast<const f16_t *>(feat), diff, grad_loss,
                               reinterpret_cast<f16_t *>(grad_feat), B, C, N, negate, stream);
}
int gfla_gram_l1_bwd_bf16(const uint16_t *feat, const float *diff, const float *grad_loss, uint16_t *grad_feat, int64_t B,
                          int64_t C, int64_t N, int negate, gfla_stream_t stream) {
  return gfla::gram_bwd<bf16_t>(reinterpret_cast<const bf16_t *>(feat), diff, grad_loss,
                                reinterpret_cast<bf16_t *>(grad_feat), B, C, N, negate, stream);
}
}
