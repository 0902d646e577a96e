// What the four Winograd-domain kernels of the first FC layer share, each thing once (fc_wino.hip: float32 operands on
// v_mfma_f32_16x16x4_f32 -- fc_wino_conv_kernel, fc_wino_wgrad_kernel; fc_wino16.hip: the same domain with two-term f16
// operands on the f16 matrix cores -- fc_wino16_conv_kernel, fc_wino16_wgrad_kernel): the three transforms on the points
// {0, 1, -1, 2, -1/2, inf}, the B^T d B passes of a transform item (fc_wino_btdb3.inc), the two-term f16 split, and the
// skeleton of the two convolution kernels -- the geometry of a workgroup's tile group, the job select, the workgroup
// decode, the raw-span stager, the step loop (fc_wino_step_loop.inc), the LDS size and the launcher.  The skeleton of the two weight-gradient kernels is
// fc_wino_wgrad.h.  A kernel supplies its fragment layouts, the store of a transformed row, its `multiply` and its
// epilogue.  See fc_wino.hip for the formulation.
#pragma once

#include "fc_gemm.h"
#include <algorithm>

namespace gfla {

constexpr int kWnXi = 36;       // 6 x 6 points
constexpr int kWnTiles = 32;    // tiles per workgroup
constexpr int kWnN = 64;        // output channels per workgroup
constexpr int kWnVFloats = kWnXi * kWnTiles * 8;  // one V buffer: [point][tile][8 channels]
constexpr int kWnThreads = 512;
constexpr unsigned kWnLdsLimit = 160 * 1024;
constexpr int kWnPF = 5;        // 16-byte pieces of the raw span a thread holds in registers across half a step

typedef float f32x2v __attribute__((ext_vector_type(2)));

template <int KS>
struct Wn {
  static constexpr int M = KS == 5 ? 2 : 4;        // output tile edge
  // LDS bytes per raw pixel (16 channels + pad).  k = 5: tiles are 2 pixels = 40 words apart (banks 8 t + channel: two tiles
  // per bank among the 8 a wave reads).  k = 3: tiles are 4 pixels apart -- 80 words = 16 mod 32 with an 80-byte pitch (four
  // tiles per bank), 72 words = 8 mod 32 with 72 bytes -- and the smaller pitch is what lets the 32x22 layer's span fit TWO
  // raw buffers next to the V buffers (the single-buffer staging costs a barrier and an exposed copy per chunk).
  static constexpr int PITCH = KS == 5 ? 80 : 72;
};

// ---- the three transforms (points 0, 1, -1, 2, -1/2, inf) -----------------------------------------------------
// B^T (6 x 6)
__device__ __forceinline__ void wn_bt(const float (&d)[6], float (&o)[6]) {
  o[0] = d[0] + 1.5f * d[1] - 2.f * d[2] - 1.5f * d[3] + d[4];
  o[1] = -d[1] - 2.5f * d[2] - 0.5f * d[3] + d[4];
  o[2] = d[1] + 0.5f * d[2] - 2.5f * d[3] + d[4];
  o[3] = -0.5f * d[1] - d[2] + 0.5f * d[3] + d[4];
  o[4] = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
  o[5] = d[1] + 1.5f * d[2] - 2.f * d[3] - 1.5f * d[4] + d[5];
}
// The same six outputs as three PAIRS -- (1, 2), (3, 4), (0, 5) -- of packed-f32 fma chains: coefficient pairs are scalar
// constants, the inputs are broadcast by op_sel, so a row costs ~10 v_pk_fma_f32 (+ a few moves) instead of ~22 scalar ops
__device__ __forceinline__ void wn_bt_pk(const float (&d)[6], float (&o)[6]) {
  const f32x2v s1{d[1], d[1]}, s2{d[2], d[2]}, s3{d[3], d[3]}, s4{d[4], d[4]};
  const f32x2v p12 = s4 + f32x2v{-1.f, 1.f} * s1 + f32x2v{-2.5f, 0.5f} * s2 + f32x2v{-0.5f, -2.5f} * s3;
  const f32x2v p34 = s4 + f32x2v{-0.5f, 2.f} * s1 + f32x2v{-1.f, -1.f} * s2 + f32x2v{0.5f, -2.f} * s3;
  const f32x2v p05 = f32x2v{d[0], d[5]} + f32x2v{1.5f, 1.f} * s1 + f32x2v{-2.f, 1.5f} * s2 + f32x2v{-1.5f, -2.f} * s3 +
                     f32x2v{1.f, -1.5f} * s4;
  o[0] = p05[0], o[5] = p05[1], o[1] = p12[0], o[2] = p12[1], o[3] = p34[0], o[4] = p34[1];
}
// rows 3*HALF .. 3*HALF + 2 of B^T d
template <int HALF, typename T = float>
__device__ __forceinline__ void wn_bt3(const T (&d)[6], T (&o)[3]) {
  if constexpr (HALF == 0) {
    o[0] = d[0] + 1.5f * d[1] - 2.f * d[2] - 1.5f * d[3] + d[4];
    o[1] = -d[1] - 2.5f * d[2] - 0.5f * d[3] + d[4];
    o[2] = d[1] + 0.5f * d[2] - 2.5f * d[3] + d[4];
  } else {
    o[0] = -0.5f * d[1] - d[2] + 0.5f * d[3] + d[4];
    o[1] = 2.f * d[1] - d[2] - 2.f * d[3] + d[4];
    o[2] = d[1] + 1.5f * d[2] - 2.f * d[3] - 1.5f * d[4] + d[5];
  }
}
// A^T (m x 6)
template <int M>
__device__ __forceinline__ void wn_at(const float (&v)[6], float (&y)[M]) {
  y[0] = v[0] + v[1] + v[2] + v[3] + v[4];
  if constexpr (M == 2) {
    y[1] = v[1] - v[2] + 2.f * v[3] - 0.5f * v[4] + v[5];
  } else {
    y[1] = v[1] - v[2] + 2.f * v[3] - 0.5f * v[4];
    y[2] = v[1] + v[2] + 4.f * v[3] + 0.25f * v[4];
    y[3] = v[1] - v[2] + 8.f * v[3] - 0.125f * v[4] + v[5];
  }
}
// G (6 x r): G[i][j] = p_i^j / prod_{l != i} (p_i - p_l), last row = e_{r-1}
template <int KS>
__device__ __forceinline__ void wn_g(const float (&w)[KS], float (&o)[6]) {
  o[0] = w[0];
  o[5] = w[KS - 1];
  if constexpr (KS == 5) {
    o[1] = -(w[0] + w[1] + w[2] + w[3] + w[4]) * (1.f / 3.f);
    o[2] = (w[0] - w[1] + w[2] - w[3] + w[4]) * (1.f / 3.f);
    o[3] = (w[0] + 2.f * w[1] + 4.f * w[2] + 8.f * w[3] + 16.f * w[4]) * (1.f / 15.f);
    o[4] = (-16.f * w[0] + 8.f * w[1] - 4.f * w[2] + 2.f * w[3] - w[4]) * (1.f / 15.f);
  } else {
    o[1] = -(w[0] + w[1] + w[2]) * (1.f / 3.f);
    o[2] = (w[0] - w[1] + w[2]) * (1.f / 3.f);
    o[3] = (w[0] + 2.f * w[1] + 4.f * w[2]) * (1.f / 15.f);
    o[4] = (-16.f * w[0] + 8.f * w[1] - 4.f * w[2]) * (1.f / 15.f);
  }
}

// one weight set of fc_wino_pack_weights / fc_wino16_pack_weights (forward: in = conv0 input channel c_off + ci, out = hidden n;
// data gradient: in = hidden n, out = conv0 input channel c_off + co, taps flipped)
struct WnPackJob {
  float *U;
  int c_off, dgrad, n_in, n_out;
};
struct WnPackJobs {
  WnPackJob j[4];
};

struct WnGeo {
  int TH, TW, ngroups, span;  // tile grid, groups of up to 32 tiles per sample, raw pixels a group stages per chunk
  int tpg;                    // tiles per group: 32, or whole tile rows on narrow maps (below)
};

// span of the groups of `tpg` consecutive tiles: from the first pixel of a group's first tile row to the last pixel of its last
// tile's 6 x 6 window (groups start at multiples of tpg tiles, so few of them are the worst case)
template <int KS>
inline int wn_span(const WnGeo &g, int tpg, int Wp) {
  constexpr int m = Wn<KS>::M;
  const int ntiles = g.TH * g.TW, ngroups = (ntiles + tpg - 1) / tpg;
  int exact = 0;
  for (int grp = 0; grp < ngroups; ++grp) {
    const int t0 = grp * tpg, t1 = std::min(t0 + tpg, ntiles) - 1;
    const int r0 = t0 / g.TW, r1 = t1 / g.TW;
    int need = 0;
    for (int r = std::max(r0, r1 - 1); r <= r1; ++r) {   // the last pixel is the last tile's, or the previous row's last tile's
      const int c = r == r1 ? t1 - r1 * g.TW : g.TW - 1;
      need = std::max(need, (m * r + 5) * Wp + m * c + 5 + 1 - m * r0 * Wp);
    }
    exact = std::max(exact, need);
  }
  return exact;
}

template <int KS>
inline WnGeo wn_geometry(int M, int Wv, int Wp) {
  constexpr int m = Wn<KS>::M;
  WnGeo g;
  const int Ho = M / Wv;
  g.TH = (Ho + m - 1) / m;
  g.TW = (Wv + m - 1) / m;
  const int ntiles = g.TH * g.TW;
  g.tpg = kWnTiles;
  g.ngroups = (ntiles + kWnTiles - 1) / kWnTiles;
  g.span = wn_span<KS>(g, kWnTiles, Wp);
  // Narrow maps (the k = 3 layer at 32x22: 6 tiles of 4 x 4 per row): groups of WHOLE tile rows -- 30 of the 32 slots -- reach
  // one tile row less than 32 consecutive tiles that start mid-row, and that is what lets the span fit TWO raw buffers next
  // to the V buffers (610 -> 534 pixels at 32x22: 161.5 KB -> 151 KB; the single-buffer staging costs a barrier and an exposed
  // copy per chunk).  Taken when it wastes at most 4 slots and does not add a group.  Tuning key 44 = 1: always 32.
  const int whole = g.TW < kWnTiles ? (kWnTiles / g.TW) * g.TW : kWnTiles;
  if (whole != kWnTiles && whole >= kWnTiles - 4 && (ntiles + whole - 1) / whole == g.ngroups && tuning(GFLA_TUNE_WINO_GROUP_32) != 1) {
    const int sp = wn_span<KS>(g, whole, Wp);
    if (sp < g.span) g.tpg = whole, g.span = sp;
  }
  return g;
}

template <int KS>
inline unsigned wn_raw_bytes(const WnGeo &g) { return (unsigned)((g.span * Wn<KS>::PITCH + 15) & ~15); }

// double_raw: two raw buffers (the next chunk's pixels land while this chunk is transformed: no extra barrier);
// exchange: the bytes through which the kernel's epilogue swaps partial outputs
template <int KS>
inline unsigned wn_lds_bytes(const WnGeo &g, bool double_raw, unsigned exchange) {
  const unsigned main_loop = (unsigned)(2 * kWnVFloats * 4) + (double_raw ? 2u : 1u) * wn_raw_bytes<KS>(g);
  return main_loop > exchange ? main_loop : exchange;
}

// ---- two-term f16 operands (arithmetic mode 5: fc_wino16.hip) ------------------------------------------------------
typedef unsigned int u32x4w __attribute__((ext_vector_type(4)));
// power-of-two scale of a tensor that gets split into f16 terms, with `headroom` bits left for what the transform adds:
// B^T d B grows an input by at most 49 (6 bits), G w G^T a weight by at most 4.3 (3 bits)
__host__ __device__ __forceinline__ int wn16_scale_exp(uint32_t amax_bits, int headroom) {
  int se = fc_scale_exp(amax_bits) - headroom;
  return se < 2 ? 2 : se;
}
__device__ __forceinline__ float wn16_pow2(int biased) { return __uint_as_float((uint32_t)biased << 23); }
constexpr int kWn16HeadX = 6, kWn16HeadW = 3;

// (hi, lo) word of a value in three instructions: v_cvt_f16_f32, v_fma_mix_f32 (v * 1 - hi with hi read as f16: the exact
// remainder, no convert back), v_cvt_pk_f16_f32 of (v, remainder) -- RN16(v) again in the low half, RN16(remainder) in the
// high one.  (The plain C form compiles to five: two converts, a convert back, a subtract and an or.)
typedef _Float16 f16x2w __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t wn16_split(float v) {
  // (v made opaque: with the multiply that produced it in sight hipcc fuses it into the convert -- v_fma_mixlo_f16 of the
  // unrounded product -- and `h` is no longer the half the packed convert below stores)
  asm("" : "+v"(v));
  const _Float16 h = (_Float16)v;
  float rem;
  asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(rem) : "v"(v), "v"(h));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2v{v, rem}, f16x2w));
}

typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4v __attribute__((ext_vector_type(4)));
struct Half0 { static constexpr int value = 0; };
struct Half1 { static constexpr int value = 1; };
typedef Half1 Yes;
typedef Half0 No;

// ---- B^T d B of one transform item -------------------------------------------------------------------------------------
// fc_wino_btdb3.inc: the column and row passes of all four kernels, #included into each kernel's transform.  Text and not
// a function for the reason the loops are: as a function template handing each row to a store functor (or returning the 18
// values) it gave the same bits but perturbed hipcc's register allocation in kernels that sit at 256 VGPRs --
// fc_wino_conv_kernel<5, 0, false> spilled a dword, the multi-row float32 weight gradients and the single-buffer f16
// convolution gained a vmcnt(0) -- while the same text in the kernel body compiles to the previous revision's code.

// ---- the convolution kernels' skeleton -----------------------------------------------------------------------------------
// One launch carries up to TWO independent convolutions (the target and the source half of a layer: same weights' shape,
// different maps): workgroups [0, n0) belong to job 0, the rest to job 1.  A workgroup lives for ~1/6 of a launch, so a
// launch of 5.5 or 6.4 rounds of 256 workgroups spends its last round half empty; two jobs in one grid share that tail
// (L2, k = 5: 6 + 7 and 7 + 8 rounds become 12 and 14).
struct WnKArgs {
  PackedDesc X;
  const float *U;            // fc_wino_pack_weights' floats or fc_wino16_pack_weights' (hi, lo) words
  const uint32_t *amax_x;    // max |x| slot of the input (two-term f16 operands only)
  float *out;
  int64_t out_bs;
  int ldo, n_valid, Ho, Wv, Wp;
  WnGeo geo;
  int ntn;
  int64_t total_groups, S;
};

// the job's parameters: workgroup-uniform selects, field by field (scalar registers)
__device__ __forceinline__ PackedDesc wn_pick(bool second, const PackedDesc &a0, const PackedDesc &a1) {
  PackedDesc X;
  X.base = second ? a1.base : a0.base, X.split_stride = 0, X.batch_stride = second ? a1.batch_stride : a0.batch_stride;
  X.chunk_stride = second ? a1.chunk_stride : a0.chunk_stride, X.pix_stride = second ? a1.pix_stride : a0.pix_stride;
  return X;
}
__device__ __forceinline__ WnKArgs wn_pick(bool second, const WnKArgs &a0, const WnKArgs &a1) {
#define GFLA_PICK(f) a.f = second ? a1.f : a0.f
  WnKArgs a;
  a.X = wn_pick(second, a0.X, a1.X);
  GFLA_PICK(U), GFLA_PICK(amax_x), GFLA_PICK(out), GFLA_PICK(out_bs), GFLA_PICK(total_groups), GFLA_PICK(S);
  GFLA_PICK(ldo), GFLA_PICK(n_valid), GFLA_PICK(Ho), GFLA_PICK(Wv), GFLA_PICK(Wp), GFLA_PICK(ntn);
  GFLA_PICK(geo.TH), GFLA_PICK(geo.TW), GFLA_PICK(geo.ngroups), GFLA_PICK(geo.span), GFLA_PICK(geo.tpg);
#undef GFLA_PICK
  return a;
}

// workgroup -> (group of tiles, output-channel tile).  Ids x and x + 8 run on the same XCD: the workgroups that share one
// group's input pixels (different channel tiles) are neighbours in that XCD's queue (shared L2).
template <int KS>
struct WnGroup {
  int ntile, tile0, ntiles, p0;   // channel tile; first tile, tiles of the sample; first pixel of the staged span
  int64_t glin, b, avail;         // group of the launch's job, its sample; pixels of the sample behind p0 (the rest reads as zero)

  // x: the workgroup's id inside its job (n0 is a multiple of 8: id & 7 is still the XCD).  false: padding of the grid,
  // the workgroup returns; true: decode() follows
  __device__ __forceinline__ bool claim(const WnKArgs &a, int64_t x) {
    const int xcd = (int)(x & 7);
    const int64_t slot = x >> 3;
    ntile = (int)(slot % a.ntn);
    glin = (slot / a.ntn) * 8 + xcd;
    return glin < a.total_groups;
  }
  __device__ __forceinline__ void decode(const WnKArgs &a) {
    b = glin / a.geo.ngroups;
    const int grp = (int)(glin - b * a.geo.ngroups);
    ntiles = a.geo.TH * a.geo.TW;
    tile0 = grp * a.geo.tpg;
    const int ty_first = tile0 / a.geo.TW;
    p0 = Wn<KS>::M * ty_first * a.Wp;
    avail = a.S - p0;
  }
  // byte offset inside the raw span of the window of a transform item: tile slot tl, channel c8 of the 8-channel step
  __device__ __forceinline__ int toff(const WnKArgs &a, int tl, int c8) const {
    constexpr int M = Wn<KS>::M;
    const int tau = min(tile0 + min(tl, a.geo.tpg - 1), ntiles - 1);   // (slots behind the group's tiles repeat its last one)
    const int ty = tau / a.geo.TW, tx = tau - ty * a.geo.TW;
    return ((M * ty * a.Wp + M * tx) - p0) * Wn<KS>::PITCH + c8 * 4;
  }
};

// Raw span of one chunk: 16-byte pieces t, t + 512, ... go global -> registers -> LDS (LDS-DMA was measured and dropped:
// with a DMA in flight hipcc turns the counted vmcnt waits of the B-fragment stream into vmcnt(0)).  Addresses = a uniform
// base + a 32-bit per-lane offset; pixels behind the end of the sample read its last pixel and are stored as zeros.  Spans
// beyond kWnPF pieces per thread are loaded at the commit (large maps only).  SCALED: the pixels are multiplied by `scale`
// on their way into LDS (two-term f16 operands); otherwise their bits move as they are, no arithmetic.
template <int KS, bool DB, bool SCALED>
struct WnStage {
  static constexpr int PITCH = Wn<KS>::PITCH;
  const unsigned char *xg;   // first pixel of the span in chunk 0: workgroup-uniform
  unsigned char *raw;        // [1 or 2][span][PITCH]
  int64_t chunk_stride, avail;
  int pix_stride, raw_bytes, npieces, t;
  float scale;
  u32x4v pf[kWnPF];

  __device__ __forceinline__ void init(const WnKArgs &a, const WnGroup<KS> &g, unsigned char *raw_, float scale_ = 1.f) {
    xg = a.X.base + g.b * a.X.batch_stride + (int64_t)g.p0 * a.X.pix_stride;
    raw = raw_, chunk_stride = a.X.chunk_stride, avail = g.avail, pix_stride = a.X.pix_stride;
    raw_bytes = (a.geo.span * PITCH + 15) & ~15, npieces = a.geo.span * 4, t = threadIdx.x, scale = scale_;
  }
  __device__ __forceinline__ unsigned piece_off(int q) const {
    const int pix = q >> 2;
    return (unsigned)min((int64_t)pix, avail - 1) * (unsigned)pix_stride + (unsigned)(q & 3) * 16u;
  }
  __device__ __forceinline__ void piece_store(int q, u32x4v v, int cc) {
    const int pix = q >> 2;
    if constexpr (SCALED) {
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = pix >= avail ? 0.f : __uint_as_float(v[e]) * scale;
      float2 *d = reinterpret_cast<float2 *>(raw + (DB ? (cc & 1) * raw_bytes : 0) + pix * PITCH + (q & 3) * 16);
      d[0] = make_float2(f[0], f[1]);
      d[1] = make_float2(f[2], f[3]);
    } else {
      if (pix >= avail) v = u32x4v{0u, 0u, 0u, 0u};
      uint2 *d = reinterpret_cast<uint2 *>(raw + (DB ? (cc & 1) * raw_bytes : 0) + pix * PITCH + (q & 3) * 16);
      d[0] = make_uint2(v[0], v[1]);
      d[1] = make_uint2(v[2], v[3]);
    }
  }
  __device__ __forceinline__ void prefetch(int cc) {
    const unsigned char *base = xg + (int64_t)cc * chunk_stride;
#pragma unroll
    for (int i = 0; i < kWnPF; ++i) pf[i] = *reinterpret_cast<const u32x4v *>(base + piece_off(min(t + kWnThreads * i, npieces - 1)));
  }
  __device__ __forceinline__ void commit(int cc) {
#pragma unroll
    for (int i = 0; i < kWnPF; ++i) {
      // UNCONDITIONAL (threads behind the span rewrite its last piece with the same data, as they loaded it): with the store
      // under `if (q < npieces)` the consumer of pf[i] sat in a divergent branch, hipcc kept the register "pending" on the
      // skipped path and the NEXT prefetch -- which reuses pf[i]'s registers for its addresses right behind the multiply half
      // -- opened with s_waitcnt vmcnt(4) .. vmcnt(0): a wait for the B words requested a moment earlier (seen in the ISA,
      // round 6; the float32 kernel had carried it since round 3)
      piece_store(min(t + kWnThreads * i, npieces - 1), pf[i], cc);
    }
    const unsigned char *base = xg + (int64_t)cc * chunk_stride;
    for (int q = t + kWnThreads * kWnPF; q < npieces; q += kWnThreads)
      piece_store(q, *reinterpret_cast<const u32x4v *>(base + piece_off(q)), cc);
  }
};

// The step loop of the two kernels is fc_wino_step_loop.inc, #included into each kernel's body.  It is text and not a
// function on purpose: as a function template (lambdas for `multiply` and `transform`) hipcc merges the copies of the
// transform that the loop keeps in both arms of `if (stage_next)` -- the single-raw-buffer instantiations lose 15 ds_read /
// 9 ds_write and gain scratch -- i.e. it undoes the one-branch form the loop's own comment asks for.

// ---- one launch of one or two convolutions (same B, input chunks, k) -------------------------------------------------
struct WnLaunch {
  WnKArgs a[2];
  unsigned n0, grid, lds;
  bool db;   // two raw buffers: every job's span fits twice (tuning key 21 = 1: never)
};
// amax_x[j]: the max |x| slot of job j's input, or amax_x == NULL; exchange: see wn_lds_bytes
template <int KS>
inline int wn_plan(const WnConvJob *jobs, int njobs, const uint32_t *const *amax_x, int64_t B, unsigned exchange, WnLaunch &L) {
  int64_t wgs[2] = {0, 0};
  L.db = tuning(GFLA_TUNE_WINO_LAUNCH) != 1;
  L.lds = 0;
  for (int j = 0; j < njobs; ++j)
    L.db = L.db && wn_lds_bytes<KS>(wn_geometry<KS>(jobs[j].M, jobs[j].Wv, jobs[j].Wp), true, exchange) <= kWnLdsLimit;
  for (int j = 0; j < 2; ++j) {
    const int jj = j < njobs ? j : 0;
    const WnConvJob &J = jobs[jj];
    const WnGeo g = wn_geometry<KS>(J.M, J.Wv, J.Wp);
    const int ntn = (int)ceil_div(J.n_valid, kWnN);
    const int64_t groups = B * g.ngroups;
    L.a[j] = WnKArgs{J.X, J.U, amax_x ? amax_x[jj] : nullptr, J.out, J.out_bs, J.ldo, J.n_valid, J.M / J.Wv, J.Wv, J.Wp, g, ntn, groups, J.S};
    if (j < njobs) {
      wgs[j] = ceil_div(groups, 8) * 8 * ntn;
      L.lds = std::max(L.lds, wn_lds_bytes<KS>(g, L.db, exchange));
    }
  }
  if (wgs[0] + wgs[1] > 0x7fffffffLL || L.lds > kWnLdsLimit) return GFLA_ERR_UNSUPPORTED;
  L.n0 = (unsigned)wgs[0], L.grid = (unsigned)(wgs[0] + wgs[1]);
  return GFLA_OK;
}
// kern(a0, a1, n0, nch, extra...)
template <typename Kern, typename... Extra>
inline int wn_start(Kern kern, const WnLaunch &L, int nch, hipStream_t stream, Extra... extra) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.lds);
  kern<<<dim3(L.grid), kWnThreads, L.lds, stream>>>(L.a[0], L.a[1], L.n0, nch, extra...);
  return launch_status();
}

}  // namespace gfla
