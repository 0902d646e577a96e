// Winograd-domain convolutions of ExtractorAttn's first FC layer with TWO-TERM f16 OPERANDS on the f16 matrix cores
// (arithmetic mode 5), gfx950, and the k = 5 weight gradient on the same operands (second half of the file).  Mode 5 runs
// only the k = 3 forward on the convolution kernel (csrc/fc_block.hip: fc_plan); the formulation below covers both kernel
// sizes.  The skeletons the kernels share with their float32 twins of fc_wino.hip are fc_wino_shared.h and fc_wino_wgrad.h.
//
// Same formulation, tiling and staging as fc_wino.hip (F(2x2,5x5) / F(4x4,3x3) on the points {0, 1, -1, 2, -1/2, inf}; reference
// base_function.py:799-807): the transforms B^T d B and A^T M A stay float32 on the vector ALUs.  What changes is the 36
// point-wise GEMMs over the channels.  fc_wino.hip runs them on v_mfma_f32_16x16x4_f32, which executes at the f32 VECTOR rate
// (157 TFLOP/s) and was 300 of that kernel's 432 us.  Here every transformed input value v and every transformed weight u is
// split into two f16 terms, v * s = hi + lo with hi = RN16(v s), lo = RN16(v s - hi) (s a power of two from the tensor's
// max |x|, so nothing over- or underflows: |v s - hi - lo| <= 2^-24 |v s|, the rounding of a float32 itself), and the product
// is formed EXACTLY from all four cross terms with f32 accumulation inside the MFMA:
//     sum_c v_c u_c = sum_c (vhi_c uhi_c + vlo_c ulo_c)  +  sum_c (vhi_c ulo_c + vlo_c uhi_c)
// With the K slots of v_mfma_f32_32x32x16_f16 filled as (hi_c, lo_c) pairs on the A side, the first sum is the MFMA against
// the weights' own (hi, lo) words and the second the MFMA against the same words with their halves swapped (one v_alignbit
// per dword): two MFMAs of 32 cycles per (32 tiles x 32 channels x 8 input channels x point) instead of eight of 32 cycles --
// the matrix-core time drops 4x and the kernel becomes bound by its LDS / vector work.  Measured error against float64 at the
// bench shapes: the same as the float32 Winograd kernels' (tools/experiments/winograd_numerics.py f16: 3.0e-6 vs 2.7e-6 of
// the largest output at k = 5, 4.7e-6 vs 4.8e-6 at k = 3 -- the f32 accumulation dominates both).
//
//   workgroup = 32 tiles x 64 output channels x 36 points, 8 waves; wave w: channel block w & 1 (32 channels), points
//   9 (w >> 1) .. +8 -> 9 accumulators of 32x32 (144 registers, two waves per SIMD);
//   per 8-channel step: A = V[point][channel quad g][tile][4 x (hi, lo)] from LDS, ONE ds_read_b128 per point (lanes 0-31 /
//   32-63 = quads 0 / 1 = the two K halves of the MFMA); B = the same layout of U from global memory, one 16-byte load per
//   point, a step ahead; the transform of the NEXT step (fc_wino.hip's, plus the split) runs in the other wave of the SIMD;
//   epilogue: every wave reduces its nine points to an m x m partial per (tile, channel); the four waves of a channel block
//   exchange partials through LDS, a quarter of the tiles each, and store 128-byte rows of the (pixel, channel) map.
#include "fc_wino_wgrad.h"

namespace gfla {

// ---- weights: conv0.weight (128, 2C, 3, 3) -> U = G w G^T * scale as (hi, lo) words in B-fragment order --------------
// U16[ntile][step = ci >> 3][point][g = (ci >> 2) & 1][n = co & 63][ci & 3]: a lane of channel block nb (n = 32 nb + lane & 31,
// g = lane >> 5) loads its 16 bytes of a (step, point) with one request; a wave's request is two runs of 512 bytes.
__global__ __launch_bounds__(256) void fc_wino16_pack_w_kernel(const float *__restrict__ w0, WnPackJobs jobs, int C,
                                                               const uint32_t *__restrict__ amax_w) {
  constexpr int KS = 3;
  const WnPackJob jb = jobs.j[blockIdx.y];
  const int nch = (jb.n_in + kFcChunk - 1) / kFcChunk, ntn = (jb.n_out + kWnN - 1) / kWnN;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (in channel, out channel), out fastest
  if (!jb.U || idx >= (int64_t)ntn * kWnN * nch * kFcChunk) return;
  const float su = wn16_pow2(wn16_scale_exp(*amax_w, kWn16HeadW));
  const int co = (int)(idx % (ntn * kWnN)), ci = (int)(idx / (ntn * kWnN));
  float w[KS][KS];
#pragma unroll
  for (int i = 0; i < KS; ++i)
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      float v = 0.f;
      if (ci < jb.n_in && co < jb.n_out) v = w0[(((int64_t)co * 2 * C + jb.c_off + ci) * KS + i) * KS + j];
      w[i][j] = v * su;
    }
  float t[6][KS];  // G w: columns first
#pragma unroll
  for (int j = 0; j < KS; ++j) {
    float col[KS], o[6];
#pragma unroll
    for (int i = 0; i < KS; ++i) col[i] = w[i][j];
    wn_g<KS>(col, o);
#pragma unroll
    for (int a = 0; a < 6; ++a) t[a][j] = o[a];
  }
  const int ntile = co / kWnN, n = co % kWnN;
  const int step = ci >> 3, g = (ci >> 2) & 1, c4 = ci & 3;
  uint32_t *dst = reinterpret_cast<uint32_t *>(jb.U) + ((((int64_t)ntile * 2 * nch + step) * kWnXi * 2 + g) * kWnN + n) * 4 + c4;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float o[6];
    wn_g<KS>(t[a], o);
#pragma unroll
    for (int e = 0; e < 6; ++e) dst[(int64_t)(a * 6 + e) * 2 * kWnN * 4] = wn16_split(o[e]);
  }
}

// the two forward weight sets of one layer (k = 3; same slots and sizes as fc_wino_pack_weights: fc_wino_wpack_bytes)
int fc_wino16_pack_weights(const float *w0, const uint32_t *amax_w, float *u_ft, float *u_fs, int C, int k, hipStream_t stream) {
  if (k != 3) return GFLA_ERR_UNSUPPORTED;
  WnPackJobs jobs;
  jobs.j[0] = WnPackJob{u_ft, 0, 0, C, kFcHidden};
  jobs.j[1] = WnPackJob{u_fs, C, 0, C, kFcHidden};
  const dim3 grid((unsigned)ceil_div(ceil_div(kFcHidden, kWnN) * kWnN * ceil_div(C, kFcChunk) * kFcChunk, 256), 2);
  fc_wino16_pack_w_kernel<<<grid, 256, 0, stream>>>(w0, jobs, C, amax_w);
  return launch_status();
}

// ---- the convolution ---------------------------------------------------------------------------------------------
// A^T (m x 6) as a table (the epilogue folds it at compile time)
template <int M>
struct WnAT;
template <>
struct WnAT<2> {
  static constexpr float v[2][6] = {{1.f, 1.f, 1.f, 1.f, 1.f, 0.f}, {0.f, 1.f, -1.f, 2.f, -0.5f, 1.f}};
};
template <>
struct WnAT<4> {
  static constexpr float v[4][6] = {{1.f, 1.f, 1.f, 1.f, 1.f, 0.f},
                                    {0.f, 1.f, -1.f, 2.f, -0.5f, 0.f},
                                    {0.f, 1.f, 1.f, 4.f, 0.25f, 0.f},
                                    {0.f, 1.f, -1.f, 8.f, -0.125f, 1.f}};
};

template <int PG_>
struct PgTag { static constexpr int value = PG_; };

// DBG: no timing ablation of this kernel is left (k = 5 went to the direct kernels); the parameter keeps the kernel's symbol
template <int KS, bool DB = true, int DBG = 0>
__global__ __launch_bounds__(kWnThreads, 2) void fc_wino16_conv_kernel(WnKArgs a0, WnKArgs a1, unsigned n0, int nch,
                                                                      const uint32_t *__restrict__ amax_w) {
  constexpr int M = Wn<KS>::M, PITCH = Wn<KS>::PITCH, NP = 9;   // points per wave
  const bool second = blockIdx.x >= n0;
  const WnKArgs a = wn_pick(second, a0, a1);
  const uint32_t *__restrict__ U = reinterpret_cast<const uint32_t *>(a.U);
  const uint32_t *__restrict__ amax_x = a.amax_x;
  float *__restrict__ out = a.out;
  extern __shared__ __attribute__((aligned(16))) unsigned char gfla_smem[];
  uint32_t *vbuf = reinterpret_cast<uint32_t *>(gfla_smem);   // [2][36 points][2 quads][32 tiles][4 channels] (hi, lo) words
  unsigned char *raw = gfla_smem + 2 * kWnVFloats * 4;        // [1 or 2][span][PITCH] float32, scaled
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nblk = wave & 1, pg = (wave >> 1) & 3, xh = wave >> 2;
  const int g = lane >> 5, l31 = lane & 31;
  // scales: input (this job's tensor), weights; the epilogue multiplies by their inverses (two exact power-of-two factors)
  const int ex = wn16_scale_exp(*amax_x, kWn16HeadX), ew = wn16_scale_exp(*amax_w, kWn16HeadW);
  const float sx = wn16_pow2(ex), inv_x = wn16_pow2(254 - ex), inv_w = wn16_pow2(254 - ew);
  WnGroup<KS> grp;
  if (!grp.claim(a, blockIdx.x - (second ? n0 : 0u))) return;
  grp.decode(a);

  // transform item of this thread: (tile, channel of the 8-channel step), rows 3*xh .. 3*xh + 2 of the point grid
  const int tl = (t & 255) >> 3, c8 = t & 7;
  const int toff = grp.toff(a, tl, c8);
  // word offset of V[first point of this half][quad c8 >> 2][tile][c8 & 3]
  const int vpos = xh * 18 * 256 + (c8 >> 2) * 128 + tl * 4 + (c8 & 3);

  f32x16 acc[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[p][i] = 0.f;

  WnStage<KS, DB, true> st;   // raw span of a chunk, scaled
  st.init(a, grp, raw, sx);

  // this lane's B words: U16[grp.ntile][step][point][g][n][4]
  const int nsteps = 2 * nch;
  const unsigned ub_wave = __builtin_amdgcn_readfirstlane((unsigned)((((unsigned)grp.ntile * nsteps) * kWnXi + NP * pg) * 2 * kWnN + nblk * 32));
  const u32x4w *ub = reinterpret_cast<const u32x4w *>(U) + ub_wave + g * kWnN + l31;
  u32x4w bf[NP];
  auto load_b = [&](int step, int p) { return ub[((unsigned)step * kWnXi + p) * 2 * kWnN]; };

  // transform of step `step` (the shared passes, then the split): raw -> V[step & 1][point rows 3*HALF..][quad][tile][channel]
  auto transform = [&](auto half_tag, int step) {
    constexpr int HALF = decltype(half_tag)::value;
    const unsigned char *src = raw + (DB ? ((step >> 1) & 1) * st.raw_bytes : 0) + toff + (step & 1) * 32;
    uint32_t *dst = vbuf + (step & 1) * kWnVFloats + vpos;
    const int row_pitch = a.Wp;
    auto store_row = [&](int r, const float (&o)[6]) {
#pragma unroll
      for (int e = 0; e < 6; ++e) dst[(r * 6 + e) * 256] = wn16_split(o[e]);
    };
#include "fc_wino_btdb3.inc"
  };

  // the wave's 18 MFMAs of step s: 9 points x (words, swapped words), taken in pairs of points so that the two MFMAs of an
  // accumulator are an issue slot apart; A words run one pair ahead of their MFMAs
  auto multiply = [&](int s, int sn) {
    const u32x4w *va = reinterpret_cast<const u32x4w *>(vbuf + (s & 1) * kWnVFloats + (NP * pg) * 256 + g * 128 + l31 * 4);
    u32x4w ra[2][2];
    auto read_pair = [&](int p, int sl) {
      ra[sl][0] = va[p * 64];
      if (p + 1 < NP) ra[sl][1] = va[(p + 1) * 64];
    };
    auto swapped = [](u32x4w w) {
      u32x4w r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = __builtin_amdgcn_alignbit(w[e], w[e], 16);
      return r;
    };
    read_pair(0, 0);
#pragma unroll
    for (int p = 0; p < NP; p += 2) {
      const int sl = (p >> 1) & 1;
      if (p + 2 < NP) read_pair(p + 2, sl ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      const f16x8 a0v = __builtin_bit_cast(f16x8, ra[sl][0]);
      const f16x8 b0v = __builtin_bit_cast(f16x8, bf[p]), b0s = __builtin_bit_cast(f16x8, swapped(bf[p]));
      if (p + 1 < NP) {
        const f16x8 a1v = __builtin_bit_cast(f16x8, ra[sl][1]);
        const f16x8 b1v = __builtin_bit_cast(f16x8, bf[p + 1]), b1s = __builtin_bit_cast(f16x8, swapped(bf[p + 1]));
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0v, b0v, acc[p], 0, 0, 0);
        acc[p + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1v, b1v, acc[p + 1], 0, 0, 0);
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0v, b0s, acc[p], 0, 0, 0);
        acc[p + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1v, b1s, acc[p + 1], 0, 0, 0);
        bf[p] = load_b(sn, p);
        bf[p + 1] = load_b(sn, p + 1);
      } else {
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0v, b0v, acc[p], 0, 0, 0);
        acc[p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0v, b0s, acc[p], 0, 0, 0);
        bf[p] = load_b(sn, p);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  st.prefetch(0);
  st.commit(0);
#pragma unroll
  for (int p = 0; p < NP; ++p) bf[p] = load_b(0, p);
  auto stamp = [](int) {};
#include "fc_wino_step_loop.inc"

  // epilogue: Y = A^T M A = sum over the points (a, e) of A^T[i][a] A^T[j][e] M[a][e].  A wave holds nine points -- row
  // a = (9 pg) / 6 from column (9 pg) % 6 on and what follows -- of 32 tiles x 32 channels: C/D layout of the 32x32 MFMA,
  // acc[p][i] = (tile 8 (i >> 2) + 4 g + (i & 3), channel lane & 31).  The tiles are finished a quarter at a time: every wave
  // reduces its points to the m x m partial of the quarter's four accumulator rows, three waves of a channel block park
  // theirs in LDS, the fourth (pg == quarter) adds them to its own and stores.
  float4 *xch = reinterpret_cast<float4 *>(gfla_smem);   // [3 writers][2 channel blocks][4 rows][m*m / 4][64 lanes]
  constexpr int MM4 = M * M / 4;
  const int col = grp.ntile * kWnN + nblk * 32 + l31;
  float *ob = out + grp.b * a.out_bs + col;
  auto partial = [&](auto pg_tag, int i, float (&part)[M * M]) {
    constexpr int PG = decltype(pg_tag)::value;
#pragma unroll
    for (int e = 0; e < M * M; ++e) part[e] = 0.f;
    // the wave's points, row by row of the point grid
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      constexpr int first = NP * PG, last = NP * PG + NP - 1;
      const int e0 = a * 6 > first ? 0 : first - a * 6, e1 = a * 6 + 5 < last ? 5 : last - a * 6;   // columns of row a in the set
      if (a * 6 + 5 < first || a * 6 > last) continue;
      float tj[M];
#pragma unroll
      for (int j = 0; j < M; ++j) {
        float sacc = 0.f;
#pragma unroll
        for (int e = 0; e < 6; ++e)
          if (e >= e0 && e <= e1 && WnAT<M>::v[j][e] != 0.f) sacc = fmaf(WnAT<M>::v[j][e], acc[a * 6 + e - first][i], sacc);
        tj[j] = sacc;
      }
#pragma unroll
      for (int ii = 0; ii < M; ++ii)
        if (WnAT<M>::v[ii][a] != 0.f) {
#pragma unroll
          for (int j = 0; j < M; ++j) part[ii * M + j] = fmaf(WnAT<M>::v[ii][a], tj[j], part[ii * M + j]);
        }
    }
  };
  // quarters per exchange round: all four at m = 2 (one round: two barriers per workgroup -- four rounds of two measured
  // 70 us of the k = 5 forward's 490), one at m = 4 (16 values per tile and channel: a round of one quarter fills 96 KB)
  constexpr int QPR = M == 2 ? 4 : 1;
  auto finish = [&](auto pg_tag) {
    constexpr int PG = decltype(pg_tag)::value;
#pragma unroll
    for (int q0 = 0; q0 < 4; q0 += QPR) {
      float part[QPR][4][M * M];
#pragma unroll
      for (int qq = 0; qq < QPR; ++qq)
#pragma unroll
        for (int r = 0; r < 4; ++r) partial(pg_tag, 4 * (q0 + qq) + r, part[qq][r]);
      __syncthreads();   // the main loop's LDS (or the previous round's partials) is dead
#pragma unroll
      for (int qq = 0; qq < QPR; ++qq) {
        const int qd = q0 + qq;
        if (PG != qd) {
          const int w3 = (PG - qd - 1) & 3;   // 0..2
          float4 *dst = xch + (((qq * 3 + w3) * 2 + nblk) * 4 * MM4) * 64 + lane;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c4 = 0; c4 < MM4; ++c4)
              dst[(r * MM4 + c4) * 64] = make_float4(part[qq][r][4 * c4], part[qq][r][4 * c4 + 1], part[qq][r][4 * c4 + 2],
                                                     part[qq][r][4 * c4 + 3]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int qq = 0; qq < QPR; ++qq) {
        const int qd = q0 + qq;
        if (PG != qd) continue;
#pragma unroll
        for (int w3 = 0; w3 < 3; ++w3) {
          const float4 *srcp = xch + (((qq * 3 + w3) * 2 + nblk) * 4 * MM4) * 64 + lane;
#pragma unroll
          for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c4 = 0; c4 < MM4; ++c4) {
              const float4 v = srcp[(r * MM4 + c4) * 64];
              part[qq][r][4 * c4] += v.x, part[qq][r][4 * c4 + 1] += v.y, part[qq][r][4 * c4 + 2] += v.z, part[qq][r][4 * c4 + 3] += v.w;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int slot_ = 8 * qd + 4 * g + r, tau = grp.tile0 + slot_;
          if (slot_ >= a.geo.tpg || tau >= grp.ntiles || col >= a.n_valid) continue;
          const int ty = tau / a.geo.TW, tx = tau - ty * a.geo.TW;
#pragma unroll
          for (int i = 0; i < M; ++i) {
            const int yo = M * ty + i;
            if (yo >= a.Ho) continue;
#pragma unroll
            for (int j = 0; j < M; ++j) {
              const int xo = M * tx + j;
              if (xo < a.Wv) ob[(int64_t)(yo * a.Wv + xo) * a.ldo] = (part[qq][r][i * M + j] * inv_x) * inv_w;
            }
          }
        }
      }
    }
  };
  if (pg == 0) finish(PgTag<0>{});
  else if (pg == 1) finish(PgTag<1>{});
  else if (pg == 2) finish(PgTag<2>{});
  else finish(PgTag<3>{});
}

// epilogue: three writers per channel block, a round of QPR quarters
constexpr unsigned wn16_exchange(int k) { return (unsigned)(3 * 2 * 4 * (k == 5 ? 2 * 2 : 4 * 4) * 64 * 4) * (k == 5 ? 4u : 1u); }

bool fc_wino16_fits(int M, int Wv, int Wp, int k) {
  if (!fc_wino_fits(M, Wv, Wp, k)) return false;
  const unsigned lds = k == 5 ? wn_lds_bytes<5>(wn_geometry<5>(M, Wv, Wp), false, wn16_exchange(5))
                              : wn_lds_bytes<3>(wn_geometry<3>(M, Wv, Wp), false, wn16_exchange(3));
  return lds <= kWnLdsLimit;
}

// one or two convolutions (same B, input chunks nch, k) in one launch; the contract of fc_wino_conv_jobs with the weights of
// fc_wino16_pack_weights and the max |x| slot of every job's input (amax_x[j])
int fc_wino16_conv_jobs(const WnConvJob *jobs, int njobs, const uint32_t *const *amax_x, int64_t B, int nch, int k,
                        const uint32_t *amax_w, hipStream_t stream) {
  if (B <= 0 || njobs <= 0) return GFLA_OK;
  if (njobs > 2 || !amax_w || k != 3) return GFLA_ERR_UNSUPPORTED;   // (k = 5 runs on the direct kernels: fc_block.hip)
  for (int j = 0; j < njobs; ++j)
    if (!amax_x[j] || !fc_wino16_fits(jobs[j].M, jobs[j].Wv, jobs[j].Wp, k)) return GFLA_ERR_UNSUPPORTED;
  if (njobs == 2 && tuning(GFLA_TUNE_WINO_LAUNCH) == 2) {
    const int st = fc_wino16_conv_jobs(jobs, 1, amax_x, B, nch, k, amax_w, stream);
    return st != GFLA_OK ? st : fc_wino16_conv_jobs(jobs + 1, 1, amax_x + 1, B, nch, k, amax_w, stream);
  }
  WnLaunch L;
  const int st = wn_plan<3>(jobs, njobs, amax_x, B, wn16_exchange(3), L);
  if (st != GFLA_OK) return st;
  return L.db ? wn_start(fc_wino16_conv_kernel<3, true>, L, nch, stream, amax_w)
              : wn_start(fc_wino16_conv_kernel<3, false>, L, nch, stream, amax_w);
}

// =====================================================================================================================
// The k = 5 weight gradient with TWO-TERM f16 OPERANDS (arithmetic mode 5, round 6).
//
// fc_wino_wgrad_kernel spends 4 608 of a step's cycles per wave in v_mfma_f32_16x16x4_f32 (36 points x 4 k steps x 32 cycles),
// and the float32 matrix instructions run at the f32 VECTOR rate: 0.54-0.56 of that pipe is all the kernel ever reached.  Same
// formulation and skeleton (fc_wino_wgrad.h: units, staging, pipeline and epilogue) here, but both operands of the 36 point-wise products are split into two f16 terms
// (as above: hi = RN16(v s), lo = RN16(v s - hi), s a power of two from the tensor's max |x|) and a step's 16 tiles are ONE
// K = 32 reduction of v_mfma_f32_16x16x32_f16 -- K slots of a lane = its four tiles as (hi, hi, lo, lo | hi, hi, lo, lo) --
// issued twice per point: against the lifted gradient's words as they are (hi hi + lo lo) and with the words of each pair
// exchanged, which is a RENAMING of registers (hi lo + lo hi): 72 MFMAs of 16 cycles per step instead of 144 of 32.
//   A = V[point][tile quad][c][(hi, hi, lo, lo) x 2] from LDS: the transform threads store their two halves of a value as two
//       16-bit words (a lane = one (tile, channel, half of the points) item as before, but lanes now run over the four tiles of a
//       quad first: 16-byte records fill up from four lanes);
//   B = Zh: a lane lifts the dY values of ITS FOUR tiles (tile quad = lane >> 4) of a step, one point row at a time, and splits
//       PAIRS of tiles: v_cvt_pk_f16_f32 (both hi), two v_fma_mix_f32 (the exact remainders, hi read as f16 from either half),
//       v_cvt_pk_f16_f32 (both lo) -- two instructions per value, no half swaps;
//   dY of the NEXT step (16 floats per lane) is requested while this step multiplies.
// Error: the same as the convolutions' (every product is formed from all four cross terms with f32 accumulation inside the
// MFMA); the accumulation over the tiles is f32 in both kernels.
constexpr int kWw16Pitch = 80;      // LDS bytes per raw pixel: the four tiles of a quad are 2 pixels = 40 words = 8 banks apart
constexpr int kWn16HeadZ = 4;       // A dY A^T grows a gradient by at most 9
constexpr int kWw16VBytes = kWnXi * 4 * 16 * 16;   // one V buffer: [point][tile quad][channel][16 bytes]

__device__ __forceinline__ void wn16_split_halves(float v, _Float16 &h, _Float16 &l) {
  asm("" : "+v"(v));   // (opaque: see wn16_split)
  h = (_Float16)v;
  float rem;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(rem) : "v"(v), "v"(h));
  l = (_Float16)rem;
}
// (hi0, hi1) and (lo0, lo1) words of two values (fc_gemm.h)
__device__ __forceinline__ void wn16_split_pair(float v0, float v1, uint32_t &hi, uint32_t &lo) { fc_split_pair(v0, v1, hi, lo); }

template <int A6>
__device__ __forceinline__ f32x2v ww_lift2v(f32x2v a, f32x2v b) {
  if constexpr (A6 == 0) return a;
  else if constexpr (A6 == 1) return a + b;
  else if constexpr (A6 == 2) return a - b;
  else if constexpr (A6 == 3) return __builtin_elementwise_fma(f32x2v{2.f, 2.f}, b, a);
  else if constexpr (A6 == 4) return __builtin_elementwise_fma(f32x2v{-0.5f, -0.5f}, b, a);
  else return b;
}

// DBG (timing ablations, `make PROBES=1` builds only, tuning key 20 = 64 + bits; results are garbage): 1 no input transform,
// 2 no MFMAs / A reads, 4 no lift / split of dY (constant B words), 8 no dY loads
template <bool MR, int DBG = 0>
__global__ __launch_bounds__(kWnThreads, 2) void fc_wino16_wgrad_kernel(WwKArgs a0, WwKArgs a1, int nsplit0, int cpad,
                                                                       int raw_stride, const uint32_t *__restrict__ amax_x0,
                                                                       const uint32_t *__restrict__ amax_x1,
                                                                       const uint32_t *__restrict__ amax_z0,
                                                                       const uint32_t *__restrict__ amax_z1) {
  constexpr int KS = 5;
  const bool second = (int)blockIdx.y >= nsplit0;
  const WwKArgs a = ww_pick(second, a0, a1);
  const float *__restrict__ Z = a.Z;
  float *__restrict__ part = a.part;
  const int ex = wn16_scale_exp(second ? *amax_x1 : *amax_x0, kWn16HeadX), ez = wn16_scale_exp(second ? *amax_z1 : *amax_z0, kWn16HeadZ);
  const float sx = wn16_pow2(ex), sz = wn16_pow2(ez), inv_x = wn16_pow2(254 - ex), inv_z = wn16_pow2(254 - ez);
  constexpr int M = 2, PITCH = kWw16Pitch;
  extern __shared__ __attribute__((aligned(16))) unsigned char gfla_smem[];
  unsigned char *vbuf = gfla_smem;                                  // [2][kWw16VBytes]
  unsigned char *raw = gfla_smem + 2 * kWw16VBytes;                 // [2][rows][L][PITCH] float32, scaled
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, xh = wave >> 2;
  const int cc = blockIdx.x, sp = (int)blockIdx.y - (second ? nsplit0 : 0);
  const int64_t u0 = a.total_units * sp / a.nsplit, u1 = a.total_units * (sp + 1) / a.nsplit;
  WwWalk<KS, MR, PITCH> walk;
  walk.init(a.geo, raw_stride);
  WwStage<KS, MR, PITCH, true> st;   // raw rows of a unit, scaled
  st.init(a, walk, cc, raw, sx);

  f32x4v acc[kWnXi];
#pragma unroll
  for (int q = 0; q < kWnXi; ++q) acc[q] = f32x4v{0.f, 0.f, 0.f, 0.f};

  // transform item: tile 4 * (wave & 3) + (lane & 3) of the step's 16, channel lane >> 2, point rows 3*xh..
  const int tj = lane & 3, tc = lane >> 2, tkg = wave & 3;
  const int tl = 4 * tkg + tj;
  // byte offset of this item's hi half inside a (point, quad, channel) record: (hi0, hi1, lo0, lo1, hi2, hi3, lo2, lo3)
  const int vpos = (tkg * 16 + tc) * 16 + (tj >> 1) * 8 + (tj & 1) * 2;
  auto transform = [&](auto half_tag, const WwUnit &un, int h, int rbuf, int vb) {
    constexpr int HALF = decltype(half_tag)::value;
    const unsigned char *src = walk.window(raw, un, h, tl, tc, rbuf);
    unsigned char *dst = vbuf + vb * kWw16VBytes + vpos;
    const int row_pitch = walk.Lr;
    auto store_row = [&](int r, const float (&o)[6]) {
#pragma unroll
      for (int e = 0; e < 6; ++e) {
        _Float16 hh, ll;
        wn16_split_halves(o[e], hh, ll);
        unsigned char *rec = dst + ((HALF * 3 + r) * 6 + e) * (4 * 16 * 16);
        *reinterpret_cast<_Float16 *>(rec) = hh;
        *reinterpret_cast<_Float16 *>(rec + 4) = ll;
      }
    };
#include "fc_wino_btdb3.inc"
  };

  // multiply: this lane's B operand = Zh of the step's tiles 4 kq .. 4 kq + 3, hidden channel 16 wave + (lane & 15)
  const int kq = lane >> 4, n = wave * 16 + (lane & 15);
  float dy[4][M][M];   // raw dY values of the step about to be multiplied (masked and scaled at the top of multiply)
  auto load_dy = [&](const WwUnit &un, int h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int tile = h * 16 + 4 * kq + j;
      int tr, tcol;
      walk.tile_rc(tile < un.nt ? tile : 0, tr, tcol);
      const float *zp = Z + un.b * a.z_bs + (a.z_lead + (int64_t)(M * (un.ty + tr)) * a.Wp + M * (un.tx0 + tcol)) * kFcHidden + n;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int jj = 0; jj < M; ++jj) dy[j][i][jj] = (DBG & 8) ? 1.f : zp[(int64_t)(i * a.Wp + jj) * kFcHidden];
    }
  };
  typedef unsigned int u32x2w __attribute__((ext_vector_type(2)));
  auto multiply = [&](const WwUnit &un, int h, int vb, const WwUnit &un_next, int h_next, bool any_next) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool live = h * 16 + 4 * kq + j < un.nt;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int jj = 0; jj < M; ++jj) dy[j][i][jj] = live ? dy[j][i][jj] * sz : 0.f;
    }
    const u32x4w *va = reinterpret_cast<const u32x4w *>(vbuf + vb * kWw16VBytes) + kq * 16 + (lane & 15);
    // A words run two points ahead of their MFMAs (an LDS round trip is longer than a point's eight split instructions)
    u32x4w a_q[4];
    a_q[0] = va[0];
    a_q[1] = va[64];
    auto row = [&](auto a6_tag) {
      constexpr int A6 = decltype(a6_tag)::value;
      // the row's lift of the four tiles, as PAIRS of tiles (packed f32 adds; a pair is what one split consumes)
      f32x2v ta01, ta23, tb01, tb23;
      ta01 = ww_lift2v<A6>(f32x2v{dy[0][0][0], dy[1][0][0]}, f32x2v{dy[0][1][0], dy[1][1][0]});
      ta23 = ww_lift2v<A6>(f32x2v{dy[2][0][0], dy[3][0][0]}, f32x2v{dy[2][1][0], dy[3][1][0]});
      tb01 = ww_lift2v<A6>(f32x2v{dy[0][0][1], dy[1][0][1]}, f32x2v{dy[0][1][1], dy[1][1][1]});
      tb23 = ww_lift2v<A6>(f32x2v{dy[2][0][1], dy[3][0][1]}, f32x2v{dy[2][1][1], dy[3][1][1]});
      // two points at a time: the second product of a point depends on its first -- the other point's MFMA sits between them
      auto points = [&](auto e_tag) {
        constexpr int E = decltype(e_tag)::value;
        constexpr int q = A6 * 6 + E;
        u32x4w bw[2], bx[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (q + u + 2 < kWnXi && !(DBG & 2)) a_q[(q + u + 2) % 4] = va[(q + u + 2) * 64];
          f32x2v z01, z23;
          if (u == 0) z01 = ww_lift2v<E>(ta01, tb01), z23 = ww_lift2v<E>(ta23, tb23);
          else z01 = ww_lift2v<E + 1>(ta01, tb01), z23 = ww_lift2v<E + 1>(ta23, tb23);
          uint32_t h01, l01, h23, l23;
          if constexpr (DBG & 4) {
            h01 = __float_as_uint(dy[0][0][0]), l01 = __float_as_uint(dy[1][0][0]), h23 = __float_as_uint(dy[2][0][0]), l23 = __float_as_uint(dy[3][0][0]);
          } else {
            wn16_split_pair(z01[0], z01[1], h01, l01);
            wn16_split_pair(z23[0], z23[1], h23, l23);
          }
          const u32x2w p01 = u32x2w{h01, l01}, p23 = u32x2w{h23, l23};
          // (lo, hi) of each pair for the cross terms: one v_pk_mov_b32 per pair (the MFMA wants four consecutive registers).
          // EARLY-CLOBBER outputs + s_nop: hipcc's hazard recognizer does not look inside inline asm.  Allocated in place the
          // move landed right behind the first MFMA, which was still reading those registers (wrong sums, measured); a vector
          // write also needs wait states before an MFMA reads the register (NaNs without the s_nop, measured).
          u32x2w x01, x23;
          asm("v_pk_mov_b32 %0, %2, %2 op_sel:[1,0]\n\tv_pk_mov_b32 %1, %3, %3 op_sel:[1,0]\n\ts_nop 3"
              : "=&v"(x01), "=&v"(x23)
              : "v"(p01), "v"(p23));
          bw[u] = u32x4w{p01[0], p01[1], p23[0], p23[1]}, bx[u] = u32x4w{x01[0], x01[1], x23[0], x23[1]};
        }
        const f16x8 av0 = __builtin_bit_cast(f16x8, a_q[q % 4]), av1 = __builtin_bit_cast(f16x8, a_q[(q + 1) % 4]);
        if constexpr (DBG & 2) {
          acc[q][0] += __uint_as_float(bw[0][0] ^ bx[0][1]), acc[q + 1][0] += __uint_as_float(bw[1][2] ^ bx[1][3]);
        } else {
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av0, __builtin_bit_cast(f16x8, bw[0]), acc[q], 0, 0, 0);
          acc[q + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av1, __builtin_bit_cast(f16x8, bw[1]), acc[q + 1], 0, 0, 0);
          acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av0, __builtin_bit_cast(f16x8, bx[0]), acc[q], 0, 0, 0);
          acc[q + 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av1, __builtin_bit_cast(f16x8, bx[1]), acc[q + 1], 0, 0, 0);
        }
      };
      points(PgTag<0>{}), points(PgTag<2>{}), points(PgTag<4>{});
    };
    row(PgTag<0>{}), row(PgTag<1>{}), row(PgTag<2>{}), row(PgTag<3>{}), row(PgTag<4>{}), row(PgTag<5>{});
    // the NEXT step's dY values: requested now, into the registers this step is done with; they fly through the barrier and
    // the other half of the next step
    if (any_next) load_dy(un_next, h_next);
  };

  constexpr bool T = !(DBG & 1), S = true;
  auto first = [&](const WwUnit &un) { load_dy(un, 0); };
#include "fc_wino_wgrad_pipeline.inc"

  // times the two inverse scales
  float *o = part + (((int64_t)sp * KS * KS) * cpad + cc * kFcChunk) * kFcHidden + wave * 16 + (lane & 15);
  auto unscaled = [&](float v) { return (v * inv_x) * inv_z; };
#include "fc_wino_wgrad_epilogue.inc"
}

// the k = 5 weight gradients of both halves with two-term f16 operands: fc_wino_wgrad_jobs' contract plus the max |x| slots of
// every job's activations (amax_x) and gradient map (amax_z)
int fc_wino16_wgrad_jobs(const WwJob *jobs, int njobs, int cpad, int64_t B, int k, const uint32_t *const *amax_x,
                         const uint32_t *const *amax_z, hipStream_t stream) {
  if (k != 5 || njobs > 2) return GFLA_ERR_UNSUPPORTED;
  if (B <= 0 || njobs <= 0) return GFLA_OK;
  for (int j = 0; j < njobs; ++j)
    if (!amax_x[j] || !amax_z[j]) return GFLA_ERR_UNSUPPORTED;
  auto single = fc_wino16_wgrad_kernel<false>, multi = fc_wino16_wgrad_kernel<true>;
#ifdef GFLA_PROBES
  switch (tuning(GFLA_TUNE_WINO_PROBE) >= 64 ? tuning(GFLA_TUNE_WINO_PROBE) - 64 : 0) {
    case 1: single = multi = fc_wino16_wgrad_kernel<true, 1>; break;
    case 2: single = multi = fc_wino16_wgrad_kernel<true, 2>; break;
    case 3: single = multi = fc_wino16_wgrad_kernel<true, 3>; break;
    case 4: single = multi = fc_wino16_wgrad_kernel<true, 4>; break;
    case 6: single = multi = fc_wino16_wgrad_kernel<true, 6>; break;
    case 7: single = multi = fc_wino16_wgrad_kernel<true, 7>; break;
    case 8: single = multi = fc_wino16_wgrad_kernel<true, 8>; break;
    case 15: single = multi = fc_wino16_wgrad_kernel<true, 15>; break;
    default: break;
  }
#endif
  return ww_launch(jobs, njobs, cpad, B, k, kWw16Pitch, kWw16VBytes, single, multi, stream, amax_x[0], amax_x[njobs > 1 ? 1 : 0],
                   amax_z[0], amax_z[njobs > 1 ? 1 : 0]);
}

}  // namespace gfla
