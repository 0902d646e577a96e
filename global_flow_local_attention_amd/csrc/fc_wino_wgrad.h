// The skeleton of the two Winograd-domain weight-gradient kernels (fc_wino.hip: fc_wino_wgrad_kernel, float32 operands;
// fc_wino16.hip: fc_wino16_wgrad_kernel, two-term f16 operands), each thing once: the job select, the unit walker, the
// raw-row stager, the unit / step pipeline, the G^T dU G epilogue and the host launcher.  A kernel supplies its V and Zh
// fragment layouts, the store of a transformed row (fc_wino_btdb3.inc), and its `multiply`: load / mask / lift /
// split of dY and the MFMA sequence.  fc_wino.hip has the formulation.
#pragma once

#include "fc_wino_shared.h"

namespace gfla {

template <int KS>
struct Ww {
  static constexpr int M = KS == 5 ? 2 : 4;
  static constexpr int SEG = KS == 5 ? 32 : 16;          // tiles per unit
  static constexpr int L = M * SEG + 6 - M;              // raw pixels per row of a unit
  // multi-row units (narrow maps): up to SEGM tiles = two 16-tile steps, so that the second step's transform runs under
  // the first one's MFMAs; the unit's raw rows (its own pitch) must fit kWwRawMax bytes and PFM pieces per thread
  static constexpr int SEGM = 32;
  static constexpr int PFM = KS == 5 ? 4 : 5;
};
constexpr int kWwRawMax = 43 * 1024;   // per raw buffer: 2 V buffers (72 KB) + 2 x 43 KB = the 160 KB of a CU

struct WwGeo {
  int TH, TW, nseg;
  int R, ups;   // tile rows per unit (> 1: narrow maps, see ww_geometry), units per sample
};
WwGeo ww_geometry(int Ho, int Wo, int k);   // fc_wino.hip

struct WwUnit {
  int64_t b;
  int ty, tx0, ntx;   // first tile row, first tile column, tiles per row
  int nt;             // tiles of the unit = ntx * rows (rows > 1 only in the multi-row instantiation)
};

// One launch carries up to TWO weight gradients (the source and the target half of a layer): split indices [0, nsplit0)
// belong to job 0, the rest to job 1 -- each job is one round of workgroups, and in one grid the second round starts on a CU
// the moment the first one's workgroup there retires.
struct WwKArgs {
  PackedDesc X;
  const float *Z;
  float *part;
  int64_t z_bs, z_lead, total_units, SX;
  int Wp, Wo, nsplit;
  WwGeo geo;
};
// the job's parameters: workgroup-uniform selects (scalar registers)
__device__ __forceinline__ WwKArgs ww_pick(bool second, const WwKArgs &a0, const WwKArgs &a1) {
#define GFLA_PICK(f) a.f = second ? a1.f : a0.f
  WwKArgs a;
  a.X = wn_pick(second, a0.X, a1.X);
  GFLA_PICK(Z), GFLA_PICK(part), GFLA_PICK(z_bs), GFLA_PICK(z_lead), GFLA_PICK(total_units), GFLA_PICK(SX);
  GFLA_PICK(Wp), GFLA_PICK(Wo), GFLA_PICK(nsplit);
  GFLA_PICK(geo.TH), GFLA_PICK(geo.TW), GFLA_PICK(geo.nseg), GFLA_PICK(geo.R), GFLA_PICK(geo.ups);
#undef GFLA_PICK
  return a;
}

// ---- the unit walker -------------------------------------------------------------------------------------------------
// unit = up to SEG tiles of ONE tile row of one sample, or -- MR (multi-row units): on a map whose tile rows are at most half
// a unit (TW <= SEG / 2: the k = 3 layer at 32x22 has 6 tiles of 4x4 per row against units of 16) a unit of one tile row
// left the k steps mostly empty (6 of 16 tiles, one exposed transform per 6 tiles) and the direct kernel won (135 vs 172 us)
// -- R = SEG / TW whole tile rows: the raw rows are staged with the map's own pitch instead of the unit's maximum, tile t of
// the unit is (t / TW, t % TW).  The single-row instantiation keeps its compile-time pitch (every LDS offset of the transform
// an immediate).  PITCH: LDS bytes per raw pixel.
template <int KS, bool MR, int PITCH>
struct WwWalk {
  static constexpr int M = Ww<KS>::M, SEG = Ww<KS>::SEG, L = Ww<KS>::L;
  WwGeo geo;
  int Lr, raw_rows;    // raw row pitch in pixels and raw rows of a unit: the unit's maximum (compile time) or, multi-row, the map's own
  int RAW;             // bytes between the two raw buffers
  unsigned inv_ntx;    // t / TW = (t * inv) >> 16 for t < 2^8

  __device__ __forceinline__ void init(const WwGeo &g, int raw_stride) {
    geo = g;
    Lr = (MR && geo.R > 1) ? M * geo.TW + 6 - M : L;
    raw_rows = (MR && geo.R > 1) ? M * geo.R + 6 - M : 6;
    RAW = MR ? raw_stride : ((6 * L * PITCH + 15) & ~15);
    inv_ntx = (65536u + (unsigned)geo.TW - 1u) / (unsigned)geo.TW;
  }
  __device__ __forceinline__ WwUnit unit_of(int64_t u) const {
    WwUnit un;
    un.b = u / geo.ups;
    const int r = (int)(u - un.b * geo.ups);
    if (MR && geo.R > 1) {   // R whole tile rows
      un.ty = r * geo.R;
      un.tx0 = 0;
      un.ntx = geo.TW;
      un.nt = geo.TW * min(geo.R, geo.TH - un.ty);
    } else {
      un.ty = r / geo.nseg;
      un.tx0 = (r - un.ty * geo.nseg) * SEG;
      un.ntx = min(SEG, geo.TW - un.tx0);
      un.nt = un.ntx;
    }
    return un;
  }
  // tile t of a unit -> (tile row inside the unit, tile column)
  __device__ __forceinline__ void tile_rc(int t_, int &tr, int &tcol) const {
    if (MR && geo.R > 1) {
      tr = (int)(((unsigned)t_ * inv_ntx) >> 16);
      tcol = t_ - tr * geo.TW;
    } else {
      tr = 0;
      tcol = t_;
    }
  }
  // the 6 x 6 window of a transform item (tile tl of step h, channel tc) in raw buffer rbuf
  __device__ __forceinline__ const unsigned char *window(const unsigned char *raw, const WwUnit &un, int h, int tl, int tc, int rbuf) const {
    const int tile = min(h * 16 + tl, un.nt - 1);
    int tr, tcol;
    tile_rc(tile, tr, tcol);
    return raw + rbuf * RAW + ((M * tr) * Lr + M * tcol) * PITCH + tc * 4;
  }
};

// ---- the raw-row stager ----------------------------------------------------------------------------------------------
// raw rows of a unit: piece q -> (row = q / (4 Lr), pixel, part); global -> registers -> LDS (two b64 stores per piece).
// SCALED: multiplied by `scale` on the way into LDS (two-term f16 operands); otherwise the bits move as they are.
template <int KS, bool MR, int PITCH, bool SCALED>
struct WwStage {
  static constexpr int M = Ww<KS>::M;
  // 16-byte pieces of a unit's raw rows per thread
  static constexpr int PF1 = (6 * Ww<KS>::L * 4 + kWnThreads - 1) / kWnThreads;
  static constexpr int PF = MR ? (PF1 > Ww<KS>::PFM ? PF1 : Ww<KS>::PFM) : PF1;
  const unsigned char *base;
  unsigned char *raw;        // [2][rows][Lr][PITCH]
  int64_t batch_stride, chunk_off, SX;   // chunk_off: the workgroup's 16-channel chunk
  int pix_stride, Wp, Lr, RAW, npieces, t;
  float scale;
  u32x4v pf[PF];

  __device__ __forceinline__ void init(const WwKArgs &a, const WwWalk<KS, MR, PITCH> &w, int cc, unsigned char *raw_, float scale_ = 1.f) {
    base = a.X.base, chunk_off = (int64_t)cc * a.X.chunk_stride;
    raw = raw_, batch_stride = a.X.batch_stride, SX = a.SX, pix_stride = a.X.pix_stride, Wp = a.Wp;
    Lr = w.Lr, RAW = w.RAW, npieces = w.raw_rows * w.Lr * 4, t = threadIdx.x, scale = scale_;
  }
  __device__ __forceinline__ const unsigned char *piece_addr(const WwUnit &un, int q, int &ldso) const {
    const int row = q / (4 * Lr), rem = q - row * (4 * Lr), px = rem >> 2, prt = rem & 3;
    ldso = (row * Lr + px) * PITCH + prt * 16;
    const int64_t pix = (int64_t)(M * un.ty + row) * Wp + M * un.tx0 + px;
    return base + un.b * batch_stride + chunk_off + (pix < SX ? pix : SX - 1) * pix_stride + prt * 16;
  }
  __device__ __forceinline__ void prefetch(const WwUnit &un) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      int ldso;
      pf[i] = *reinterpret_cast<const u32x4v *>(piece_addr(un, min(t + kWnThreads * i, npieces - 1), ldso));
    }
  }
  __device__ __forceinline__ void commit(const WwUnit &un, int buf) {
#pragma unroll
    for (int i = 0; i < PF; ++i) {
      // unconditional, like the convolution kernels' commit (threads behind the unit's pieces rewrite the last one)
      const int q = min(t + kWnThreads * i, npieces - 1);
      int ldso;
      (void)piece_addr(un, q, ldso);
      if constexpr (SCALED) {
        float2 *d = reinterpret_cast<float2 *>(raw + buf * RAW + ldso);
        d[0] = make_float2(__uint_as_float(pf[i][0]) * scale, __uint_as_float(pf[i][1]) * scale);
        d[1] = make_float2(__uint_as_float(pf[i][2]) * scale, __uint_as_float(pf[i][3]) * scale);
      } else {
        uint2 *d = reinterpret_cast<uint2 *>(raw + buf * RAW + ldso);
        d[0] = make_uint2(pf[i][0], pf[i][1]);
        d[1] = make_uint2(pf[i][2], pf[i][3]);
      }
    }
  }
};

// ---- the unit / step pipeline ------------------------------------------------------------------------------------------
// fc_wino_wgrad_pipeline.inc, #included into each kernel's body.  It is text and not a function on purpose: as a function
// template (lambdas for `multiply` and `transform`) hipcc computes the 36 window addresses of the next unit's first transform
// once for both places that run it and keeps them in registers across the multiply half -- the multi-row instantiations
// lose their ds_read2 pairs (192 -> 273 ds_read) and spill (0 -> 100, 104 -> 236 bytes of scratch).

// ---- the epilogue ------------------------------------------------------------------------------------------------------
// fc_wino_wgrad_epilogue.inc (dW = G^T dU G per lane), #included into each kernel's body: as a function taking the
// accumulators (by reference, or through an accessor) it changed how hipcc allocates the registers of the step loop before
// it -- the f16 kernel's step gained 3-4 lgkmcnt(0) and measured 2-3 % slower in the two-job launch.

// ---- the launcher ------------------------------------------------------------------------------------------------------
// One or two weight gradients (same B, cpad, k) in one launch of `single` (one tile row per unit) or `multi` (the MR
// instantiation: some job has units of several tile rows): kern(a0, a1, nsplit0, cpad, raw_stride, extra...).  pitch, v_bytes:
// the kernel's LDS bytes per raw pixel and per V buffer.  part: fc_wino_wgrad_splits(...) slabs of k*k * cpad * 128 floats.
// X: packed f32 records; Z: the f32 (B, Sz, 128) Z-layout map.
template <typename Kern, typename... Extra>
inline int ww_launch(const WwJob *jobs, int njobs, int cpad, int64_t B, int k, int pitch, unsigned v_bytes, Kern single, Kern multi,
                     hipStream_t stream, Extra... extra) {
  if (k != 3 && k != 5) return GFLA_ERR_UNSUPPORTED;
  if (njobs > 2) return GFLA_ERR_UNSUPPORTED;
  if (B <= 0 || njobs <= 0) return GFLA_OK;
  WwKArgs a[2];
  int ns[2] = {0, 0};
  bool multirow = false;
  int raw_stride = 0;   // bytes of one raw buffer: the larger of the jobs' needs
  const int m = k == 5 ? 2 : 4, L = k == 5 ? Ww<5>::L : Ww<3>::L;
  for (int j = 0; j < 2; ++j) {
    const WwJob &J = jobs[j < njobs ? j : 0];
    if (J.X.pix_stride != 64) return GFLA_ERR_UNSUPPORTED;
    const WwGeo g = ww_geometry(J.Ho, J.Wo, k);
    const int nsplit = fc_wino_wgrad_splits(B, J.Ho, J.Wo, cpad, k);
    a[j] = WwKArgs{J.X, J.Z, J.part, J.z_bs, J.z_lead, B * g.ups, J.SX, J.Wp, J.Wo, nsplit, g};
    if (j < njobs) {
      ns[j] = nsplit;
      multirow = multirow || g.R > 1;
      const int need = ((g.R > 1 ? (m * g.R + 6 - m) * (m * g.TW + 6 - m) : 6 * L) * pitch + 15) & ~15;
      if (need > raw_stride) raw_stride = need;
    }
  }
  const unsigned lds = 2 * v_bytes + 2 * (unsigned)raw_stride;
  if (lds > kWnLdsLimit) return GFLA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(cpad / kFcChunk), (unsigned)(ns[0] + ns[1]));
  Kern kern = multirow ? multi : single;
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<grid, kWnThreads, lds, stream>>>(a[0], a[1], ns[0], cpad, raw_stride, extra...);
  return launch_status();
}

}  // namespace gfla
