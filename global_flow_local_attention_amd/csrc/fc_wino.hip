// Winograd-domain f32 MFMA convolutions for ExtractorAttn's first FC layer, gfx950 (arithmetic mode 4).
//
// The stride-1 k x k convolutions of the "sample the convolved map" formulation (fc_gemm.hip; reference
// base_function.py:799-807) are evaluated as F(2x2, 5x5) (k = 5) / F(4x4, 3x3) (k = 3) with the SAME 6 interpolation
// points {0, 1, -1, 2, -1/2, inf}:   Y = A^T [ (G w G^T) .* (B^T d B) ] A   per 6 x 6 input tile d and channel pair,
// so a tile's m x m outputs cost 36 multiplies per (input channel, output channel) instead of 100 (k = 5, m = 2) or
// 144 (k = 3, m = 4): 2.78x / 4x fewer MFMA flops, all arithmetic float32 (transforms on the vector ALUs, the 36
// point-wise products as 36 small GEMMs over the channels on v_mfma_f32_16x16x4_f32).  Measured error of the
// formulation in float32 against float64 (tests/test_fc_wino_*.py): forward 2.4e-6 / 5.6e-6 of the largest output,
// weight gradient 5e-6 -- the direct f32 form gives 4e-7 / 2.6e-6; the reference's own cuDNN / MIOpen convolutions
// are Winograd kernels of the same family.
//
// One fused kernel per convolution (forward of either half, and the data gradient = the same kernel on the Z-layout
// gradient map with flipped / transposed weights): no transformed tensor ever exists in HBM.
//   workgroup = 32 tiles (two 16-row MFMA blocks) x 64 output channels x ALL 36 points; 8 waves, wave w = output
//   channels 16(w&3)..+15 and 18 of the 36 points (three rows of the point grid): 18 x 2 accumulators of 16x16 (144
//   registers, two waves per SIMD);
//   per 8-channel step:  A = transformed input V[point][tile][8 ch] from LDS (double buffered: the NEXT step's
//   transform -- a thread takes one (tile, channel) item, B^T d in registers, then its wave's three rows of
//   (B^T d) B -- runs on the vector ALUs while the other wave of the SIMD runs this step's MFMAs: the two waves of a
//   SIMD take the two halves of a step in opposite order), B = the wave's slice of U = G w G^T, global -> registers
//   directly in fragment layout, each register reloaded for the next step right after its last use;
//   raw input pixels of a 16-channel chunk: one contiguous span of the linearised map (tap (i,j) = pixel offset
//   i*Wp + j, as in fc_conv_impl.h), prefetched into registers one step ahead, LDS pitch 80 / 72 bytes so that the
//   transform's reads (8 tiles x 8 channels per wave) are spread over all banks;
//   epilogue: A^T M A: each wave reduces its three point rows to an m x m partial per (tile, channel) in registers, the
//   wave pairs swap partials through LDS, stores go to the same (pixel, channel) f32 map fc_conv writes.
// What these kernels have in common with their two-term f16 twins (fc_wino16.hip) is written once: fc_wino_shared.h (the
// transforms, the convolution kernels' skeleton), fc_wino_wgrad.h (the weight-gradient kernels' skeleton).  This file holds
// the float32 arithmetic: the weight pack, fc_wino_conv_kernel, fc_wino_wgrad_kernel, and ww_geometry / fc_wino_wgrad_splits
// for both weight-gradient kernels.
#include "fc_wino_wgrad.h"

namespace gfla {


// ---- weights: conv0.weight (128, 2C, k, k) -> U = G w G^T in MFMA B-fragment order -------------------------------
// U[ntile][chunk][half][point pair][nblock][lane][point & 1][2]: lane (kq = lane >> 4, n = lane & 15) holds input channels
// 16*chunk + 8*half + {kq, 4 + kq} of output channel 64*ntile + 16*nblock + n, for two neighbouring points: ONE 16-byte
// load per point pair and step.
// forward:        in = conv0 input channel c_off + ci, out = hidden n, taps as stored;
// data gradient:  in = hidden n, out = conv0 input channel c_off + co, taps flipped (the transposed convolution).

// grid (blocks, 4 jobs): forward / data-gradient sets of the target / source half in ONE launch.  Threads run along the
// OUTPUT channel: the 36 stores of 16 neighbouring threads fill consecutive fragment slots.
template <int KS>
__global__ __launch_bounds__(256) void fc_wino_pack_w_kernel(const float *__restrict__ w0, WnPackJobs jobs, int C) {
  const WnPackJob jb = jobs.j[blockIdx.y];
  const int nch = (jb.n_in + kFcChunk - 1) / kFcChunk, ntn = (jb.n_out + kWnN - 1) / kWnN;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (in channel, out channel), out fastest
  if (!jb.U || idx >= (int64_t)ntn * kWnN * nch * kFcChunk) return;
  const int co = (int)(idx % (ntn * kWnN)), ci = (int)(idx / (ntn * kWnN));
  float w[KS][KS];
#pragma unroll
  for (int i = 0; i < KS; ++i)
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      float v = 0.f;
      if (ci < jb.n_in && co < jb.n_out) {
        v = jb.dgrad ? w0[(((int64_t)ci * 2 * C + jb.c_off + co) * KS + (KS - 1 - i)) * KS + (KS - 1 - j)]
                     : w0[(((int64_t)co * 2 * C + jb.c_off + ci) * KS + i) * KS + j];
      }
      w[i][j] = v;
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
  const int ntile = co / kWnN, nb = (co % kWnN) >> 4, n = co & 15;
  const int cc = ci >> 4, half = (ci >> 3) & 1, ks = (ci >> 2) & 1, kq = ci & 3;
  float *dst = jb.U + ((((((int64_t)ntile * nch + cc) * 2 + half) * (kWnXi / 2)) * 4 + nb) * 64 + kq * 16 + n) * 4 + ks;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    float o[6];
    wn_g<KS>(t[a], o);
#pragma unroll
    for (int e = 0; e < 6; ++e) {
      const int q = a * 6 + e;
      dst[(int64_t)(q >> 1) * 4 * 64 * 4 + (q & 1) * 2] = o[e];
    }
  }
}

int64_t fc_wino_wpack_bytes(int n_in, int n_out) {
  return (int64_t)ceil_div(n_out, kWnN) * ceil_div(n_in, kFcChunk) * 2 * kWnXi * 4 * 64 * 2 * 4;
}

// the four weight sets of one layer: forward (C -> 128) and data gradient (128 -> C) of the target / source half
int fc_wino_pack_weights(const float *w0, float *u_ft, float *u_fs, float *u_dt, float *u_ds, int C, int k,
                         hipStream_t stream) {
  WnPackJobs jobs;
  jobs.j[0] = WnPackJob{u_ft, 0, 0, C, kFcHidden};
  jobs.j[1] = WnPackJob{u_fs, C, 0, C, kFcHidden};
  jobs.j[2] = WnPackJob{u_dt, 0, 1, kFcHidden, C};
  jobs.j[3] = WnPackJob{u_ds, C, 1, kFcHidden, C};
  int64_t most = 0;
  for (int q = 0; q < 4; ++q) {
    const int64_t n = ceil_div(jobs.j[q].n_out, kWnN) * kWnN * ceil_div(jobs.j[q].n_in, kFcChunk) * kFcChunk;
    if (jobs.j[q].U && n > most) most = n;
  }
  if (most == 0) return GFLA_OK;
  const dim3 grid((unsigned)ceil_div(most, 256), 4);
  if (k == 5)
    fc_wino_pack_w_kernel<5><<<grid, 256, 0, stream>>>(w0, jobs, C);
  else if (k == 3)
    fc_wino_pack_w_kernel<3><<<grid, 256, 0, stream>>>(w0, jobs, C);
  else
    return GFLA_ERR_UNSUPPORTED;
  return launch_status();
}

// ---- the convolution ---------------------------------------------------------------------------------------------

// 8 waves.  Wave w: output channels 16*(w & 3) .. +15 of the workgroup's 64, points 18*(w >> 2) .. +17 (three rows of the
// 6 x 6 point grid), both 16-tile blocks: 18 x 2 accumulators of 16x16 = 144 registers, two waves per SIMD.  Waves w and
// w + 4 sit on the same SIMD and run the two halves of a step in OPPOSITE order -- one multiplies (matrix cores) while the
// other transforms the next step's input (vector ALUs, LDS).
// The skeleton -- two jobs per launch, the workgroup decode, the raw-span stager, the step loop, the launcher -- is
// fc_wino_shared.h's; this kernel supplies the fragment layouts, the V store, `multiply` and the epilogue.
// DBG (timing ablations of the k = 5 kernel, `make PROBES=1` builds only, tuning key 20; results are garbage): 1 no transform,
// 2 no MFMAs / A reads, 4 no B reloads, 8 no raw staging, 16 per-wave phase times (s_memtime) summed over the steps ->
// stamps[workgroup][wave][6]
template <int KS, int DBG = 0, bool DB = true>
__global__ __launch_bounds__(kWnThreads, 2) void fc_wino_conv_kernel(WnKArgs a0, WnKArgs a1, unsigned n0, int nch,
                                                                    unsigned long long *stamps) {
  constexpr int M = Wn<KS>::M, PITCH = Wn<KS>::PITCH, NX = kWnXi / 2;
  const bool second = blockIdx.x >= n0;
  const WnKArgs a = wn_pick(second, a0, a1);
  const float *__restrict__ U = a.U;
  float *__restrict__ out = a.out;
  unsigned long long tk0 = 0, tsum[5] = {0, 0, 0, 0, 0};   // prologue, first half, second half, barrier, epilogue
  if constexpr (DBG & 16) tk0 = __builtin_amdgcn_s_memtime();
  auto stamp = [&](int slot) {
    if constexpr (DBG & 16) {
      if (slot >= 1 && slot <= 3) __builtin_amdgcn_s_waitcnt(0);   // the halves and the barrier: everything they asked for is back
      const unsigned long long n = __builtin_amdgcn_s_memtime();
      tsum[slot] += n - tk0;
      tk0 = n;
    }
  };
  extern __shared__ __attribute__((aligned(16))) unsigned char gfla_smem[];
  float *vbuf = reinterpret_cast<float *>(gfla_smem);      // [2][36][32][8]
  unsigned char *raw = gfla_smem + 2 * kWnVFloats * 4;     // [1 or 2][span][PITCH]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nb = wave & 3, xh = wave >> 2;
  WnGroup<KS> g;
  if (!g.claim(a, blockIdx.x - (second ? n0 : 0u))) return;
  g.decode(a);

  // transform item of this thread: (tile, channel of the 8-channel step), rows 3*xh .. 3*xh + 2 of the point grid
  const int tl = (t & 255) >> 3, c8 = t & 7;
  const int toff = g.toff(a, tl, c8);
  // float offset of V[first point][16-tile block][channel pair kq >> 1][tile][kq & 1][k step]: the A fragments of a
  // half-wave (kq = 0, 1 x 16 tiles, 8 bytes each) are then 256 contiguous bytes -- no bank conflicts on the b64 reads
  const int vpos = xh * NX * kWnTiles * 8 + (tl >> 4) * 128 + (((c8 & 3) >> 1) * 16 + (tl & 15)) * 4 + (c8 & 1) * 2 + (c8 >> 2);

  f32x4v acc[NX][2];
#pragma unroll
  for (int q = 0; q < NX; ++q)
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) acc[q][mb] = f32x4v{0.f, 0.f, 0.f, 0.f};

  WnStage<KS, DB, false> st;
  st.init(a, g, raw);

  // this lane's B fragments of the current step: U[g.ntile][cc][half][point][nb][lane][2]
  // (the wave's base offset goes through readfirstlane: a scalar base + one per-lane offset register, no per-load
  // vector address arithmetic in the MFMA stream)
  const unsigned ub_wave = __builtin_amdgcn_readfirstlane((unsigned)((((unsigned)g.ntile * nch * 2 * (kWnXi / 2) + xh * (NX / 2)) * 4 + nb) * 64));
  const f32x4v *ub = reinterpret_cast<const f32x4v *>(U) + ub_wave;
  f32x4v bf[NX / 2];   // [point pair]: (point 0: k step 0, 1; point 1: k step 0, 1)
  auto load_b = [&](int step, int qp) { return (ub + ((unsigned)step * (kWnXi / 2) + qp) * 4 * 64)[lane]; };

  const int arow = ((lane >> 5) * 16 + (lane & 15)) * 4 + ((lane >> 4) & 1) * 2;  // this lane's A fragment inside V[point][block]

  // ---- the two halves of a step ---------------------------------------------------------------------------------------
  // f32-input MFMAs execute on the SIMD's f32 ALUs (157 TFLOP/s = the vector rate): vector instructions are NOT hidden
  // behind them, they add (measured: every ablation of this kernel is additive).  So the instruction streams are kept
  // lean, and the two waves of a SIMD run the two halves in opposite order so that the LDS / global latencies of one sit
  // under the arithmetic of the other.
  // transform of step `step`: raw[(tile pixel + i*Wp + j)][channel] -> V[step & 1][point rows 3*HALF..][tile][channel]
  auto transform = [&](auto half_tag, int step) {
    constexpr int HALF = decltype(half_tag)::value;
    const unsigned char *src = raw + (DB ? ((step >> 1) & 1) * st.raw_bytes : 0) + toff + (step & 1) * 32;
    float *dst = vbuf + (step & 1) * kWnVFloats + vpos;
    const int row_pitch = a.Wp;
    auto store_row = [&](int r, const float (&o)[6]) {
#pragma unroll
      for (int e = 0; e < 6; ++e) dst[(r * 6 + e) * kWnTiles * 8] = o[e];
    };
#include "fc_wino_btdb3.inc"
  };

  // the wave's 72 MFMAs of step s: 18 points x 2 tile blocks x 2 k steps, taken in 9 pairs of points -- eight MFMAs on
  // four accumulators, the two MFMAs of an accumulator four issue slots apart (a 16x16x4 f32 MFMA has a 40-cycle
  // dependent latency against a 32-cycle issue).  A fragments run one pair ahead of their MFMAs; the sched_barriers keep
  // hipcc from sinking the reads next to their use, where every point would expose a full LDS round trip.
  auto multiply = [&](int s, int sn) {
    const float *va = vbuf + (s & 1) * kWnVFloats + xh * NX * kWnTiles * 8 + arow;
    float2 ra[2][2][2];  // [pair parity][point of the pair][tile block]
    auto read_pair = [&](int q, int slot) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        ra[slot][u][0] = *reinterpret_cast<const float2 *>(va + (q + u) * kWnTiles * 8);
        ra[slot][u][1] = *reinterpret_cast<const float2 *>(va + (q + u) * kWnTiles * 8 + 16 * 8);
      }
    };
    read_pair(0, 0);
#pragma unroll
    for (int q = 0; q < NX; q += 2) {
      const int slot = (q >> 1) & 1;
      if (q + 2 < NX) read_pair(q + 2, slot ^ 1);
      __builtin_amdgcn_sched_barrier(0);
      const f32x4v bq = bf[q >> 1];
      acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][0][0].x, bq[0], acc[q][0], 0, 0, 0);
      acc[q][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][0][1].x, bq[0], acc[q][1], 0, 0, 0);
      acc[q + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][1][0].x, bq[2], acc[q + 1][0], 0, 0, 0);
      acc[q + 1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][1][1].x, bq[2], acc[q + 1][1], 0, 0, 0);
      acc[q][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][0][0].y, bq[1], acc[q][0], 0, 0, 0);
      acc[q][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][0][1].y, bq[1], acc[q][1], 0, 0, 0);
      acc[q + 1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][1][0].y, bq[3], acc[q + 1][0], 0, 0, 0);
      acc[q + 1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ra[slot][1][1].y, bq[3], acc[q + 1][1], 0, 0, 0);
      if constexpr (!(DBG & 4)) bf[q >> 1] = load_b(sn, q >> 1);  // the register is free again: next step's slice, a step ahead
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  st.prefetch(0);
  st.commit(0);
#pragma unroll
  for (int q = 0; q < NX / 2; ++q) bf[q] = load_b(0, q);
#include "fc_wino_step_loop.inc"

  // epilogue: Y = A^T M A = sum over the point rows a of A^T[:, a] (x) (A^T M[a, :]).  A wave holds three of the six rows:
  // it reduces them to an m x m partial per (tile, channel); wave pairs (w, w + 4) swap partials through LDS -- wave w
  // finishes tile block 0, wave w + 4 block 1.  C/D layout of the 16x16 MFMA: column (channel) = lane & 15,
  // row (tile) = 4*(lane >> 4) + r.
  float *xch = reinterpret_cast<float *>(gfla_smem);  // [mb][nb][lane][4 r][m*m], written by the wave that does NOT own mb
  const int col = g.ntile * kWnN + nb * 16 + (lane & 15);
  float *ob = out + g.b * a.out_bs + col;
  auto finish = [&](auto half_tag) {
    constexpr int HALF = decltype(half_tag)::value;   // this wave's point rows 3*HALF.., and the tile block it finishes
    float part[2][4][M * M];
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float qv[3][M];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          float v[6], y[M];
#pragma unroll
          for (int e = 0; e < 6; ++e) v[e] = acc[a * 6 + e][mb][r];
          wn_at<M>(v, y);
#pragma unroll
          for (int j = 0; j < M; ++j) qv[a][j] = y[j];
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {
          float v[6], y[M];
#pragma unroll
          for (int a = 0; a < 6; ++a) v[a] = (a >= 3 * HALF && a < 3 * HALF + 3) ? qv[a - 3 * HALF][j] : 0.f;
          wn_at<M>(v, y);
#pragma unroll
          for (int i = 0; i < M; ++i) part[mb][r][i * M + j] = y[i];
        }
      }
    __syncthreads();  // the main loop's LDS is dead
    {
      float *dst = xch + (((1 - HALF) * 4 + nb) * 64 + lane) * 4 * M * M;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int e = 0; e < M * M; ++e) dst[r * M * M + e] = part[1 - HALF][r][e];
    }
    __syncthreads();
    const float *srcp = xch + ((HALF * 4 + nb) * 64 + lane) * 4 * M * M;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int slot_ = HALF * 16 + 4 * (lane >> 4) + r, tau = g.tile0 + slot_;
      if (slot_ >= a.geo.tpg || tau >= g.ntiles || col >= a.n_valid) continue;
      const int ty = tau / a.geo.TW, tx = tau - ty * a.geo.TW;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const int yo = M * ty + i;
        if (yo >= a.Ho) continue;
#pragma unroll
        for (int j = 0; j < M; ++j) {
          const int xo = M * tx + j;
          if (xo < a.Wv) ob[(int64_t)(yo * a.Wv + xo) * a.ldo] = part[HALF][r][i * M + j] + srcp[r * M * M + i * M + j];
        }
      }
    }
  };
  if (xh == 0) finish(Half0{});
  else finish(Half1{});
  if constexpr (DBG & 16) {
    stamp(4);
    if (stamps && lane == 0) {
      unsigned long long *o = stamps + ((int64_t)blockIdx.x * 8 + wave) * 6;
#pragma unroll
      for (int i = 0; i < 5; ++i) o[i] = tsum[i];
      o[5] = (unsigned long long)xh;
    }
  }
}

// epilogue: the partial outputs of the wave pairs
template <int KS>
constexpr unsigned wn32_exchange() { return (unsigned)(kWnThreads * 4 * Wn<KS>::M * Wn<KS>::M * 4); }

bool fc_wino_fits(int M, int Wv, int Wp, int k) {
  if (k != 3 && k != 5) return false;
  if (Wv <= 0 || Wv > Wp || M <= 0 || M % Wv) return false;
  const unsigned lds = k == 5 ? wn_lds_bytes<5>(wn_geometry<5>(M, Wv, Wp), false, wn32_exchange<5>())
                              : wn_lds_bytes<3>(wn_geometry<3>(M, Wv, Wp), false, wn32_exchange<3>());
  return lds <= kWnLdsLimit;
}

// out[b][r][n] = sum_{chunk, tap, c} X[b][chunk][pix(r) + tap][c] * w[...]  -- the contract of fc_conv (fc_conv_impl.h),
// with the weights given as the transformed U of fc_wino_pack_weights.  S = pixels per sample X may be read for.
static unsigned long long *g_wino_stamps = nullptr;  // timing probe buffer (gfla_fc_wino_debug_buffer; tools only)

template <int K_>
static int wn_launch(const WnConvJob *jobs, int njobs, int64_t B, int nch, hipStream_t stream) {
  WnLaunch L;
  const int st = wn_plan<K_>(jobs, njobs, nullptr, B, wn32_exchange<K_>(), L);
  if (st != GFLA_OK) return st;
  unsigned long long *stamps = g_wino_stamps;
#define GFLA_WINO_LAUNCH(D_, DB_) return wn_start(fc_wino_conv_kernel<K_, D_, DB_>, L, nch, stream, stamps);
  if (!L.db) GFLA_WINO_LAUNCH(0, false)
#ifdef GFLA_PROBES  // `make PROBES=1`: timing ablations of the k = 5 kernel (tuning key 20; their results are garbage, so
                    // a default build does not contain them and a stray key 20 cannot corrupt a forward / backward)
  switch (K_ == 5 ? tuning(GFLA_TUNE_WINO_PROBE) : 0) {
    case 1: GFLA_WINO_LAUNCH(1, true)
    case 2: GFLA_WINO_LAUNCH(2, true)
    case 4: GFLA_WINO_LAUNCH(4, true)
    case 8: GFLA_WINO_LAUNCH(8, true)
    case 3: GFLA_WINO_LAUNCH(3, true)
    case 16: GFLA_WINO_LAUNCH(16, true)
    case 5: GFLA_WINO_LAUNCH(5, true)
    case 13: GFLA_WINO_LAUNCH(13, true)
    default: break;
  }
#endif
  GFLA_WINO_LAUNCH(0, true)
#undef GFLA_WINO_LAUNCH
}

// one or two convolutions (same B, input chunks nch, k) in one launch; tuning key 21 = 2: one launch per job
int fc_wino_conv_jobs(const WnConvJob *jobs, int njobs, int64_t B, int nch, int k, hipStream_t stream) {
  if (B <= 0 || njobs <= 0) return GFLA_OK;
  if (njobs > 2) return GFLA_ERR_UNSUPPORTED;
  for (int j = 0; j < njobs; ++j)
    if (!fc_wino_fits(jobs[j].M, jobs[j].Wv, jobs[j].Wp, k)) return GFLA_ERR_UNSUPPORTED;
  if (njobs == 2 && tuning(GFLA_TUNE_WINO_LAUNCH) == 2) {
    const int st = fc_wino_conv_jobs(jobs, 1, B, nch, k, stream);
    return st != GFLA_OK ? st : fc_wino_conv_jobs(jobs + 1, 1, B, nch, k, stream);
  }
  return k == 5 ? wn_launch<5>(jobs, njobs, B, nch, stream) : wn_launch<3>(jobs, njobs, B, nch, stream);
}

int fc_wino_conv(const PackedDesc &X, const float *U, float *out, int64_t out_bs, int ldo, int n_valid, int64_t B, int nch,
                 int M, int Wv, int Wp, int64_t S, int k, hipStream_t stream) {
  const WnConvJob job{X, U, out, out_bs, ldo, n_valid, M, Wv, Wp, S};
  return fc_wino_conv_jobs(&job, 1, B, nch, k, stream);
}

// =====================================================================================================================
// Weight gradient in the Winograd domain (arithmetic mode 4).
//
//   dU[point][c][n] = sum over tiles  V[tile][c][point] * Zh[tile][n][point],   V = B^T d B (the forward's input transform),
//   Zh = A dY A^T (the m x m output-gradient tile lifted to the 6 x 6 points),   dW[n][c] = G^T dU[.][c][n] G  (k x k),
// i.e. the adjoint of Y = A^T [U .* V] A: 36 multiplies per (tile, c, n) instead of 100 (k = 5) / 144 (k = 3).
//
// Workgroup (8 waves) = one 16-channel chunk of the input x ALL 36 points x the 128 hidden channels (wave w: columns
// 16w..16w+15: 36 accumulators of 16x16) x a contiguous range of "units" (= up to SEG tiles of ONE tile row of one sample;
// equal ranges per split, one round of workgroups).  The reduction runs over tiles, four per v_mfma_f32_16x16x4_f32:
//   A = V[point][tile][c] from LDS, produced 16 tiles at a time by the conv kernel's transform (a thread = one (tile,
//       channel) item, three of the six point rows; two V buffers), read back as one ds_read_b128 per point and step;
//   B = Zh: every lane lifts its own (tile, hidden channel) dY values -- 4 (k = 5) or 16 (k = 3) floats straight from the
//       gradient map in global memory, one k step ahead -- to the 36 points IN REGISTERS (about 32 vector ops per k step);
//   the two halves of a step (multiply / transform the next 16 tiles) run in opposite order on the two waves of a SIMD.
// Partial sums per split leave as plain coalesced stores; fc_wino_wgrad_reduce adds the splits, applies G^T . G and writes
// conv0.weight.grad's layout.
constexpr int kWwPitch = 72;   // LDS bytes per raw pixel: 16 tiles' stride (8 / 16 pixels) lands on the other half of the banks
constexpr int kWwVFloats = 4 * 4 * 16 * kWnXi;           // one V buffer: [tile >> 2][tile & 3][channel][point]: a lane's 36
                                                         // A values of a k step are contiguous (nine ds_read_b128)

// A dY A^T for one (tile, channel): dy[i][j] (m x m) -> zh[36]
template <int M>
__device__ __forceinline__ void ww_lift(const float (&dy)[M][M], float (&zh)[kWnXi]) {
  float t[6][M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    if constexpr (M == 2) {
      const float a = dy[0][j], b = dy[1][j];
      t[0][j] = a, t[1][j] = a + b, t[2][j] = a - b, t[3][j] = a + 2.f * b, t[4][j] = a - 0.5f * b, t[5][j] = b;
    } else {
      const float a = dy[0][j], b = dy[1][j], c = dy[2][j], d = dy[3][j];
      t[0][j] = a;
      t[1][j] = a + b + c + d;
      t[2][j] = a - b + c - d;
      t[3][j] = a + 2.f * b + 4.f * c + 8.f * d;
      t[4][j] = a - 0.5f * b + 0.25f * c - 0.125f * d;
      t[5][j] = d;
    }
  }
#pragma unroll
  for (int a6 = 0; a6 < 6; ++a6) {
    if constexpr (M == 2) {
      const float a = t[a6][0], b = t[a6][1];
      zh[a6 * 6 + 0] = a, zh[a6 * 6 + 1] = a + b, zh[a6 * 6 + 2] = a - b, zh[a6 * 6 + 3] = a + 2.f * b;
      zh[a6 * 6 + 4] = a - 0.5f * b, zh[a6 * 6 + 5] = b;
    } else {
      const float a = t[a6][0], b = t[a6][1], c = t[a6][2], d = t[a6][3];
      zh[a6 * 6 + 0] = a;
      zh[a6 * 6 + 1] = a + b + c + d;
      zh[a6 * 6 + 2] = a - b + c - d;
      zh[a6 * 6 + 3] = a + 2.f * b + 4.f * c + 8.f * d;
      zh[a6 * 6 + 4] = a - 0.5f * b + 0.25f * c - 0.125f * d;
      zh[a6 * 6 + 5] = d;
    }
  }
}

// The skeleton -- two jobs per launch, the unit walker, the raw-row stager, the unit / step pipeline, the G^T dU G epilogue,
// the launcher -- is fc_wino_wgrad.h's; this kernel supplies the V layout, the lift of dY and the MFMA sequence.
// DBG (timing ablations, `make PROBES=1` builds only, tuning key 20 = 32 + bits; results are garbage): 1 no input transform,
// 2 no MFMAs / A reads, 4 no dY loads, 8 no lift of dY to the 36 points, 16 no raw staging
template <int KS, int DBG = 0, bool MR = false>
__global__ __launch_bounds__(kWnThreads, 2) void fc_wino_wgrad_kernel(WwKArgs a0, WwKArgs a1, int nsplit0, int cpad,
                                                                     int raw_stride) {
  const bool second = (int)blockIdx.y >= nsplit0;
  const WwKArgs a = ww_pick(second, a0, a1);
  const float *__restrict__ Z = a.Z;
  float *__restrict__ part = a.part;
  constexpr int M = Ww<KS>::M, PITCH = kWwPitch;
  extern __shared__ __attribute__((aligned(16))) unsigned char gfla_smem[];
  float *vbuf = reinterpret_cast<float *>(gfla_smem);            // [2][kWwVFloats]
  unsigned char *raw = gfla_smem + 2 * kWwVFloats * 4;           // [2][6][L][PITCH]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, xh = wave >> 2;
  const int cc = blockIdx.x, sp = (int)blockIdx.y - (second ? nsplit0 : 0);
  const int64_t u0 = a.total_units * sp / a.nsplit, u1 = a.total_units * (sp + 1) / a.nsplit;
  WwWalk<KS, MR, PITCH> walk;
  walk.init(a.geo, raw_stride);
  WwStage<KS, MR, PITCH, false> st;
  st.init(a, walk, cc, raw);

  f32x4v acc[kWnXi];
#pragma unroll
  for (int q = 0; q < kWnXi; ++q) acc[q] = f32x4v{0.f, 0.f, 0.f, 0.f};

  // transform item: tile (wave & 3) + 4 * (lane >> 4) of the step's 16, channel lane & 15, point rows 3*xh..
  const int tq = wave & 3, tks = lane >> 4, tc = lane & 15;
  const int tl = tq + 4 * tks;
  const int vpos = ((tks * 4 + tq) * 16 + tc) * kWnXi + xh * 18;   // float offset of V[ks][tq][c][first point of this half]
  auto transform = [&](auto half_tag, const WwUnit &un, int h, int rbuf, int vb) {
    constexpr int HALF = decltype(half_tag)::value;
    const unsigned char *src = walk.window(raw, un, h, tl, tc, rbuf);
    float *dst = vbuf + vb * kWwVFloats + vpos;
    const int row_pitch = walk.Lr;
    auto store_row = [&](int r, const float (&o)[6]) {
      float2 *d2 = reinterpret_cast<float2 *>(dst + r * 6);   // 8-byte aligned: 144-byte records, halves at +72, rows at +24
      d2[0] = make_float2(o[0], o[1]);
      d2[1] = make_float2(o[2], o[3]);
      d2[2] = make_float2(o[4], o[5]);
    };
#include "fc_wino_btdb3.inc"
  };

  // multiply: the step's k steps (4 tiles each); this lane's B operand = Zh of tile 4*ks + (lane >> 4), channel 16*wave + (lane & 15)
  const int kq = lane >> 4, n = wave * 16 + (lane & 15);
  auto load_dy = [&](const WwUnit &un, int h, int ks, float (&dy)[M][M]) {
    const int tile = h * 16 + 4 * ks + kq;
    const bool live = tile < un.nt;
    int tr, tcol;
    walk.tile_rc(live ? tile : 0, tr, tcol);
    const int xo0 = M * (un.tx0 + tcol);
    const float *zp = Z + un.b * a.z_bs + (a.z_lead + (int64_t)(M * (un.ty + tr)) * a.Wp + xo0) * kFcHidden + n;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) {
        dy[i][j] = (DBG & 4) ? 1.f : zp[(int64_t)(i * a.Wp + j) * kFcHidden];   // RAW: masked at use (mask_dy)
      }
  };
  // The masks are applied where the values are consumed, not where they are loaded: a select right behind the load made
  // every load_dy wait for its own round trip -- the "two k steps ahead" never happened (80 of the kernel's 385 us).
  auto mask_dy = [&](const WwUnit &un, int h, int ks, float (&dy)[M][M]) {
    const int tile = h * 16 + 4 * ks + kq;
    const bool live = tile < un.nt;
    int tr, tcol;
    walk.tile_rc(live ? tile : 0, tr, tcol);
    const int xo0 = M * (un.tx0 + tcol);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) {
        // columns Wo .. Wp-1 and the rows behind Ho are zero in the Z layout, but a partial tile of a 4 x 4 tiling can reach
        // column Wp = the next row's first output: masked
        dy[i][j] = (live && (M == 2 || xo0 + j < a.Wo)) ? dy[i][j] : 0.f;
      }
  };
  auto multiply = [&](const WwUnit &un, int h, int vb, const WwUnit &, int, bool) {
    const int nks = min(4, (un.nt - h * 16 + 3) >> 2);
    const float *va = vbuf + vb * kWwVFloats + (kq * 16 + (lane & 15)) * kWnXi;
    // the dY values run TWO k steps ahead of their use (global loads: an L2 round trip is about one k step of MFMAs)
    constexpr int AHEAD = M == 2 ? 2 : 1;
    float dy[AHEAD + 1][M][M];
#pragma unroll
    for (int a = 0; a < AHEAD; ++a)
      if (a < nks) load_dy(un, h, a, dy[a]);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks < nks) {  // wave-uniform
        if (ks + AHEAD < nks) load_dy(un, h, ks + AHEAD, dy[(ks + AHEAD) % (AHEAD + 1)]);
        float zh[kWnXi];
        mask_dy(un, h, ks, dy[ks % (AHEAD + 1)]);
        if constexpr (DBG & 8) {
#pragma unroll
          for (int q = 0; q < kWnXi; ++q) zh[q] = dy[ks % (AHEAD + 1)][q & 1][(q >> 1) & 1];
        } else {
          ww_lift<M>(dy[ks % (AHEAD + 1)], zh);
        }
        const f32x4v *vp = reinterpret_cast<const f32x4v *>(va + ks * 4 * 16 * kWnXi);
        if constexpr (DBG & 2) {
#pragma unroll
          for (int q = 0; q < kWnXi; ++q) acc[q][0] += zh[q];
        } else {
#pragma unroll
          for (int q4 = 0; q4 < kWnXi / 4; ++q4) {
            const f32x4v a4 = vp[q4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
              acc[q4 * 4 + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[e], zh[q4 * 4 + e], acc[q4 * 4 + e], 0, 0, 0);
          }
        }
      }
    }
  };

  constexpr bool T = !(DBG & 1), S = !(DBG & 16);
  auto first = [](const WwUnit &) {};
#include "fc_wino_wgrad_pipeline.inc"

  float *o = part + (((int64_t)sp * KS * KS) * cpad + cc * kFcChunk) * kFcHidden + wave * 16 + (lane & 15);
  auto unscaled = [](float v) { return v; };
#include "fc_wino_wgrad_epilogue.inc"
}

WwGeo ww_geometry(int Ho, int Wo, int k) {
  const int m = k == 5 ? 2 : 4, seg = k == 5 ? 32 : 16;
  WwGeo g;
  g.TH = (Ho + m - 1) / m;
  g.TW = (Wo + m - 1) / m;
  g.nseg = (g.TW + seg - 1) / seg;
  // Units of R whole tile rows (the MR instantiation) wherever that needs fewer 16-tile steps per sample than one row per
  // unit: the k = 3 layer at 32x22 has 6 tiles per row (5 rows = 30 of 32), the k = 5 layer at 64x44 has 22 / 24 (one row:
  // 16 + 6..8 of 32; two rows: 44..48 of 48 -- a quarter fewer steps).  Bounds: the unit's raw rows (the map's own pitch)
  // within kWwRawMax bytes and the staging registers of the instantiation.  Tuning key 29: 1 = one row per unit (round 3),
  // 2 = at most 16 tiles per unit.
  g.R = 1;
  if (g.nseg == 1 && tuning(GFLA_TUNE_WINO_WGRAD_UNITS) != 1) {
    const int pfm = (k == 5 ? 4 : 5) * kWnThreads;
    const int cap = tuning(GFLA_TUNE_WINO_WGRAD_UNITS) == 2 ? 16 : 1 << 20;
    auto steps = [&](int R) { return (g.TH / R) * ((R * g.TW + 15) / 16) + (g.TH % R ? ((g.TH % R) * g.TW + 15) / 16 : 0); };
    int best = 1, best_steps = steps(1);
    for (int R = 2; R <= g.TH && R * g.TW <= cap; ++R) {
      const int px = (m * R + 6 - m) * (m * g.TW + 6 - m);
      if (px * kWwPitch > kWwRawMax || px * 4 > pfm) break;
      if (steps(R) <= best_steps) best = R, best_steps = steps(R);
    }
    g.R = best;
  }
  g.ups = g.R > 1 ? (g.TH + g.R - 1) / g.R : g.TH * g.nseg;
  return g;
}

int fc_wino_wgrad_splits(int64_t B, int Ho, int Wo, int cpad, int k) {
  const WwGeo g = ww_geometry(Ho, Wo, k);
  const int64_t units = B * g.ups;
  // 8 waves per workgroup, two per SIMD: ONE workgroup per CU; one round of 256 workgroups
  int64_t s = tuning(GFLA_TUNE_FC_WGRAD_SPLITS) > 0 ? tuning(GFLA_TUNE_FC_WGRAD_SPLITS) : kNumCU / (cpad / kFcChunk);
  if (s < 1) s = 1;
  return (int)(s > units ? units : s);
}

// one or two weight gradients (same B, cpad, k) in one launch
int fc_wino_wgrad_jobs(const WwJob *jobs, int njobs, int cpad, int64_t B, int k, hipStream_t stream) {
  const unsigned v_bytes = kWwVFloats * 4;
#define GFLA_WW(K_, D_) \
  return ww_launch(jobs, njobs, cpad, B, k, kWwPitch, v_bytes, fc_wino_wgrad_kernel<K_, D_, false>, fc_wino_wgrad_kernel<K_, D_, true>, stream);
  if (k != 5) GFLA_WW(3, 0)
#ifdef GFLA_PROBES  // timing ablations (tuning key 20 = 32 + bits; results are garbage): `make PROBES=1` builds only
  switch (tuning(GFLA_TUNE_WINO_PROBE) >= 32 ? tuning(GFLA_TUNE_WINO_PROBE) - 32 : 0) {
    case 1: GFLA_WW(5, 1)
    case 2: GFLA_WW(5, 2)
    case 4: GFLA_WW(5, 4)
    case 8: GFLA_WW(5, 8)
    case 16: GFLA_WW(5, 16)
    case 12: GFLA_WW(5, 12)
    case 29: GFLA_WW(5, 29)
    default: break;
  }
#endif
  GFLA_WW(5, 0)
#undef GFLA_WW
}

int fc_wino_wgrad(const PackedDesc &X, const float *Z, int64_t z_bs, int64_t z_lead, float *part, int cpad, int64_t B, int Ho,
                  int Wo, int Wp, int64_t SX, int k, hipStream_t stream) {
  const WwJob job{X, Z, part, z_bs, z_lead, SX, Ho, Wo, Wp};
  return fc_wino_wgrad_jobs(&job, 1, cpad, B, k, stream);
}


// `part` holds nsplit slabs of k*k * cpad * 128 floats (the kernel's epilogue has applied G^T . G): the direct kernel's layout
int fc_wino_wgrad_reduce(float *part, int nsplit, float *grad_w0, int C, int c_off, int cpad, int k, hipStream_t stream) {
  if (k != 3 && k != 5) return GFLA_ERR_UNSUPPORTED;
  return fc_wgrad_reduce(part, nsplit, grad_w0, C, c_off, cpad, k, stream);
}

// source half (conv0 input channels C..2C-1) and target half (0..C-1) in one launch
int fc_wino_wgrad_reduce2(float *part_s, int nsplit_s, float *part_t, int nsplit_t, float *grad_w0, int C, int cpad, int k,
                          hipStream_t stream) {
  if (k != 3 && k != 5) return GFLA_ERR_UNSUPPORTED;
  return fc_wgrad_reduce2(part_s, nsplit_s, part_t, nsplit_t, grad_w0, C, cpad, k, stream);
}

}  // namespace gfla

extern "C" {
/* tools only: device buffer (workgroups x 8 waves x 6 uint64) that the DBG=16 instantiation of the Winograd kernel (tuning
 * key 20 = 16) fills with per-wave phase times in shader cycles; NULL switches it off */
int gfla_fc_wino_debug_buffer(void *buffer) {
#ifdef GFLA_PROBES
  gfla::g_wino_stamps = static_cast<unsigned long long *>(buffer);
  return GFLA_OK;
#else
  (void)buffer;   // the probe instantiations are not part of a default build (make PROBES=1)
  return GFLA_ERR_UNSUPPORTED;
#endif
}
}
