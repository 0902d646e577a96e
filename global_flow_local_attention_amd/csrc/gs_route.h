// Routing policy of the gather/scatter ops (block_extractor and its unfold form, resample2d, local_attn_aggregate with
// source_bwd): ONE pure host function per entry-point family maps (shape, storage / accumulator size, kernel size,
// dilation, wanted gradients, workspace present or not, current tuning keys) to
//   the route (which kernel generation runs), the launch geometry of that route, and the side conditions its launcher
//   needs (zero-fill first, LDS kernel as the matrix-core product's device-side fallback, FIX / TAB).
// The launchers (block_extractor.hip, resample2d.hip, local_attn_aggregate.hip) are argument checks, `route = ...`,
// `switch (route.path)`; the host-side queries (gs_route.hip) read the same functions.  Nothing here touches the device.
// The route tables are in DESIGN.md section 3.2.  The routing keys 0, 2, 3, 6, 7, 22, 23, 30 and 38 are read in this file only.
#pragma once

#include <type_traits>

#include "agg_stream.h"
#include "be_bwd_lds.h"
#include "be_fwd_pix.h"
#include "be_fwd_wrow.h"
#include "be_tile.h"

namespace gfla {

// ---- template selection --------------------------------------------------------------------------------------------------
// f(std::integral_constant<int, K>) for K = k in [LO, HI]; anything else takes HI, as a switch's default would.
template <int LO, int HI, typename F>
inline void k_dispatch(int k, F &&f) {
  if constexpr (LO >= HI) {
    f(std::integral_constant<int, HI>{});
  } else {
    if (k == LO) f(std::integral_constant<int, LO>{});
    else k_dispatch<LO + 1, HI>(k, f);
  }
}
// Run the statements with `constexpr int NAME` = KV for KV in [LO, HI] (the compile-time kernel sizes of a family).
#define GFLA_K_SWITCH(NAME, LO, HI, KV, ...) \
  ::gfla::k_dispatch<LO, HI>(KV, [&](auto gfla_k_) { constexpr int NAME = decltype(gfla_k_)::value; __VA_ARGS__; })
// Run the statements with `constexpr bool WIN` = the planes are row windows (PlaneGeo::margin >= 0), not whole.
#define GFLA_WIN_SWITCH(MARGIN, ...)                                   \
  do {                                                                 \
    if ((MARGIN) < 0) { constexpr bool WIN = false; __VA_ARGS__; }     \
    else { constexpr bool WIN = true; __VA_ARGS__; }                   \
  } while (0)

inline bool grid_ok(int64_t blocks) { return blocks <= 0x7fffffffLL; }
inline int64_t plane_blocks(int64_t B, const PlaneGeo &g) { return B * g.ngroups * g.split; }

// ---- shared tests --------------------------------------------------------------------------------------------------------
// LDS bytes per plane element of a backward pass by the gradients wanted: a double scatter plane for grad_source, a gather
// plane of the arithmetic type for grad_flow.
inline int wanted_plane_bytes(bool need_src, bool need_flow, int acc_size) {
  return (need_src ? (int)sizeof(lds_acc_t) : 0) + (need_flow ? acc_size : 0);
}
// LDS bytes per plane element of the ops of big_geometry (tile_map.h): 0 block_extractor forward, 2 resample2d forward and 4 its
// d/d input2 keep a gather plane of the arithmetic type, 3 resample2d d/d input1 a double scatter plane, 1 block_extractor
// backward both.  It is what the regime test weighs against the budget and what a window element of both gradients costs.
inline int big_plane_bytes(int op, int acc_size) {
  return op == 1 ? wanted_plane_bytes(true, true, acc_size) : op == 3 ? wanted_plane_bytes(true, false, acc_size) : acc_size;
}
// The regime of the big-plane kernels of `op`: few planes (the planes-in-LDS / windowed kernels get fewer than ~4 workgroups
// per CU out of batch x channel groups), each beyond the LDS budget.  tuning key 30: 1 = never (round 1's windowed kernels),
// 2 = always (tests drive the kernels at small shapes).  The routes below and out[0] of gfla_big_plane_geometry ask here.
inline bool big_plane_regime(int op, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int acc_size) {
  const int t = tuning(GFLA_TUNE_BIG_PLANE);
  if (t == 1) return false;
  if (t == 2) return true;
  return Hs * Ws * (int64_t)big_plane_bytes(op, acc_size) > lds_budget() && B * C < 4 * kNumCU;
}
// What gfla_big_plane_geometry answers for `op` (include/gfla_hip.h: out[10]): the regime by the routes' own predicate, then
// the geometry of big_geometry.
inline void big_plane_answer(int op, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int span, int acc_size,
                             int64_t *out) {
  const BigGeo g = big_geometry(op, B, C, H, W, span, big_plane_bytes(op, acc_size));
  const int64_t v[10] = {big_plane_regime(op, B, C, Hs, Ws, acc_size) ? 1 : 0, g.tg.th, g.tg.tw, g.tg.ntx, g.tg.nty, g.tg.threads,
                         g.G, g.ngroups, g.lds_bytes, g.nwg};
  for (int i = 0; i < 10; ++i) out[i] = v[i];
}
// A double scatter plane and a gather plane of the arithmetic type per source position within the budget: what the
// backward kernels that keep both whole need (unfold / aggregation / source_bwd; the only ones 16-bit storage has).
inline bool scatter_gather_planes_fit(int64_t Hs, int64_t Ws, int acc_size) {
  return Hs * Ws * (int64_t)wanted_plane_bytes(true, true, acc_size) <= lds_budget();
}
// Policy, not correctness.  Tuning keys 3 and 8 = 1 switch the aggregation stream kernels off (round 1's kernels: the tests'
// reference).
inline bool agg_stream_enabled() { return tuning(GFLA_TUNE_AGG) != 1 && tuning(GFLA_TUNE_AGG_STREAM) != 1; }
// The aggregation takes them from k = 5: k = 3 has 16 patch words per output instead of 36, and there the per-group setup
// of agg_fwd_lds_kernel costs less than the extra coefficient pass (23 us against 20 + 5 at the bench shape); key 8 = 2
// forces them for every odd k.  (resample2d's d/d input2 has no such break-even: agg_stream_enabled() alone.)
inline bool agg_stream_wanted(int k) { return agg_stream_enabled() && (k >= 5 || tuning(GFLA_TUNE_AGG_STREAM) == 2); }

// ---- geometry of the planes-in-LDS launchers -----------------------------------------------------------------------------
// Either the whole plane (plane_geometry) or a row window (band_geometry; tuning key 7 = 1: never).
inline PlaneGeo lds_geometry(int64_t H, int64_t W, int bytes_per_elem, int64_t B, int64_t C, int64_t Hf,
                             int64_t items_per_row, int k_span, int chunk = 0) {
  PlaneGeo g = plane_geometry(H * W, bytes_per_elem, B, C, Hf * items_per_row, true, chunk);
  if (g.G > 0) return g;
  if (tuning(GFLA_TUNE_NO_WINDOWS) == 1) return g;  // windows disabled
  return band_geometry(H, W, bytes_per_elem, B, C, Hf, items_per_row, k_span);
}
// acc_size = sizeof(Num<T>::acc), elem_size = sizeof(T).  Unfold forward: whole gather planes only.
inline PlaneGeo unfold_fwd_geometry(int acc_size, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf) {
  return plane_geometry(Hs * Ws, acc_size, B, C, Hf * Wf, true);
}
// resample2d: forward and d/d input2 gather from planes of the arithmetic type, d/d input1 scatters into double planes.
// 16-bit storage: the scatter planes are whole and have one owner each (the flush is a plain read-modify-write).
inline PlaneGeo rs_gather_geometry(int acc_size, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int k,
                                   int dil, int chunk) {
  return lds_geometry(Hi, Wi, acc_size, B, C, H, W, (k - 1) * dil + 1, chunk);
}
inline PlaneGeo rs_scatter_geometry(int elem_size, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int k,
                                    int dil) {
  return elem_size == 2 ? plane_geometry(Hi * Wi, sizeof(lds_acc_t), B, C, H * W, false)
                        : lds_geometry(Hi, Wi, sizeof(lds_acc_t), B, C, H, W, (k - 1) * dil + 1);
}
// be_bwd_lds_kernel.  The factored / unfold forms are only produced for planes that fit; the tensor form may window.
// 16-bit storage (elem_size 2): whole planes, one owner per plane (no atomics on the planes).
inline PlaneGeo be_bwd_lds_geometry(int mode, int elem_size, int acc_size, bool need_src, bool need_flow, int64_t B, int64_t C,
                                    int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf, int K) {
  const int bytes = wanted_plane_bytes(need_src, need_flow, acc_size);
  const bool half = elem_size == 2;
  return (mode == kGoutTensor && !half) ? lds_geometry(Hs, Ws, bytes, B, C, Hf, Wf, K + 3, 1)
                                        : plane_geometry(Hs * Ws, bytes, B, C, Hf * Wf, !half, 1);
}

// ---- geometry of the global-memory kernels: thread <-> (b, channel chunk, item) ------------------------------------------
struct Geo {
  int cpt, ncg, sp_blocks;
  int64_t blocks;
};
inline Geo chunk_geometry(int64_t B, int64_t C, int64_t items, int max_cpt, int64_t want_waves) {
  Geo g;
  g.sp_blocks = (int)ceil_div(items, kBlock);
  int cpt = tuning(GFLA_TUNE_GLOBAL_CPT) > 0 ? tuning(GFLA_TUNE_GLOBAL_CPT)
                                             : pick_channels_per_thread((int64_t)g.sp_blocks * kBlock, C, B, max_cpt, want_waves);
  if (cpt > C) cpt = (int)C;
  g.cpt = cpt;
  g.ncg = (int)ceil_div(C, cpt);
  g.blocks = (int64_t)g.sp_blocks * g.ncg * B;
  return g;
}
constexpr int64_t kFillWaves = 4 * kNumCU * kWavesPerCU, kHalfFillWaves = 2 * kNumCU * kWavesPerCU;

// big-plane gathers of resample2d from global memory (rs_fwd_big_kernel / rs_bwd2_big_kernel): all channels per thread
// unless that leaves fewer than 20 waves per CU (tuning key 33)
struct BigGatherGeo {
  int cpt, ncg, nsp;
  int64_t nwg;
};
inline BigGatherGeo big_gather_geometry(int64_t B, int64_t C, int64_t H, int64_t W) {
  const int64_t nsp = ceil_div(H * W, kBlock), want = 20 * kNumCU;
  int64_t cpt = C;
  if (tuning(GFLA_TUNE_BIG_GATHER_CPW) > 0) cpt = tuning(GFLA_TUNE_BIG_GATHER_CPW) < C ? tuning(GFLA_TUNE_BIG_GATHER_CPW) : C;
  else while (cpt > 1 && B * nsp * (kBlock / 64) * ceil_div(C, cpt) < want) cpt = ceil_div(cpt, 2);
  const int64_t ncg = ceil_div(C, cpt);
  return BigGatherGeo{(int)cpt, (int)ncg, (int)nsp, B * nsp * ncg};
}

// ==== block_extractor forward =============================================================================================
// Rows and keys: DESIGN.md 3.2.  Why auto picks as it does: few planes far beyond the LDS budget (BASELINE configs[1]) take
// parallelism from pixel blocks, not planes (be_tile.h); the wave-per-flow-row kernel writes contiguous pieces whatever the
// width (4.6-5.6 TB/s), the lane-per-pixel kernel reaches 5.2 TB/s only where its output rows are whole 128-byte lines.
enum class BeFwdPath { kUnsupported, kGpix, kTile, kWrow, kPix, kLds, kRows };
struct BeFwdRoute {
  BeFwdPath path;
  BeGpixGeo gpix;  // kGpix (tuning key 38 = 1: the big-plane regime's first version)
  BigGeo big;      // kTile
  WrowGeo wrow;    // kWrow
  PixGeo pix;      // kPix
  PlaneGeo lds;    // kLds: be_fwd_lds_kernel<T, V, WIN = lds.margin >= 0>
  Geo rows;        // kRows
};
// V = outputs per lane of round 1's kernels (what the alignment of `out` and k * Wf allow)
inline BeFwdRoute be_fwd_route(int elem_size, int acc_size, int V, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf,
                               int64_t Wf, int k) {
  BeFwdRoute r{};
  const int variant = tuning(GFLA_TUNE_BE_FWD);
  if (elem_size >= 4 && k >= 2 && k <= 5) {
    if (variant == 0 && big_plane_regime(0, B, C, Hs, Ws, acc_size) && Hs * Ws <= 0x3fffffffLL) {
      if (tuning(GFLA_TUNE_BIG_GATHER_V1) == 1) {
        r.gpix = be_gpix_geometry(B, C, Hf, Wf, k, acc_size);
        if (grid_ok(r.gpix.nwg)) return r.path = BeFwdPath::kGpix, r;
      } else {
        r.big = big_geometry(0, B, C, Hf, Wf, k + 1, acc_size);
        if (grid_ok(r.big.nwg)) return r.path = BeFwdPath::kTile, r;
      }
    }
    // small output planes (<= 32 KB: a whole plane is a few hundred lines that one workgroup writes within microseconds)
    // stream slightly faster from the lane-per-pixel kernel: (32,256,32,22) k=3 40 us against 41-45
    const bool small_plane = (int64_t)k * k * Hf * Wf * elem_size <= 32 * 1024 && Wf <= 64;
    if (variant == 4 || (variant == 0 && !small_plane)) {
      r.wrow = wrow_geometry(B, C, Hs, Ws, Hf, Wf, k, acc_size, elem_size);
      if (r.wrow.G > 0 && grid_ok(B * r.wrow.ngroups) && grid_ok((int64_t)k * k * Hf * Wf)) return r.path = BeFwdPath::kWrow, r;
    }
    if (variant != 1 && variant != 2 && variant != 4) {
      r.pix = pix_geometry(be_pix_chunk(acc_size, k), B, C, Hs, Ws, Hf, Wf, k, acc_size);
      if (r.pix.G > 0 && grid_ok(B * r.pix.ngroups * r.pix.split)) return r.path = BeFwdPath::kPix, r;
    }
  }
  if (variant != 1) {
    // work items = output positions; one flow row = k output rows of (k*Wf)/V positions
    r.lds = lds_geometry(Hs, Ws, acc_size, B, C, Hf, (int64_t)k * ((k * Wf) / V), k + 1, 1);
    if (r.lds.G > 0) return r.path = grid_ok(plane_blocks(B, r.lds)) ? BeFwdPath::kLds : BeFwdPath::kUnsupported, r;
  }
  r.rows = chunk_geometry(B, C, k * Hf * ((k * Wf) / V), 16, kFillWaves);
  return r.path = grid_ok(r.rows.blocks) ? BeFwdPath::kRows : BeFwdPath::kUnsupported, r;
}

// ==== block_extractor backward (gradient of a (B,C,kH,kW) tensor) =========================================================
// 16-bit storage has no atomics: the planes-in-LDS kernel (whole planes, one owner each) or nothing, whatever key 2 says.
enum class BeBwdPath { kUnsupported, kTile, kLds, kGlobal, kElem };
struct BeBwdRoute {
  BeBwdPath path;
  BigGeo big;    // kTile: flow-pixel tiles with bounding-box windows (be_tile.h)
  PlaneGeo lds;  // kLds: be_bwd_lds_kernel<..., kGoutTensor, WIN = lds.margin >= 0>
  Geo global;    // kGlobal: be_bwd_pix_kernel
};
// the kernel sizes with a compile-time instantiation; gfla_lds_plane_geometry op 0 answers from here for every k <= 5
inline BeBwdRoute be_bwd_fixed_k_route(int elem_size, int acc_size, bool need_src, bool need_flow, int64_t B, int64_t C,
                                       int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf, int k) {
  BeBwdRoute r{};
  const bool half = elem_size == 2;
  if (tuning(GFLA_TUNE_BE_BWD) != 1 && !half && big_plane_regime(1, B, C, Hs, Ws, acc_size)) {
    r.big = big_geometry(1, B, C, Hf, Wf, k + 1, wanted_plane_bytes(need_src, need_flow, acc_size));
    if (Hs * Ws <= 0x3fffffffLL && grid_ok((int64_t)k * Hf * k * Wf) && grid_ok(r.big.nwg)) return r.path = BeBwdPath::kTile, r;
  }
  if (tuning(GFLA_TUNE_BE_BWD) != 1 || half) {
    r.lds = be_bwd_lds_geometry(kGoutTensor, elem_size, acc_size, need_src, need_flow, B, C, Hs, Ws, Hf, Wf, k);
    if (r.lds.G > 0) return r.path = grid_ok(plane_blocks(B, r.lds)) ? BeBwdPath::kLds : BeBwdPath::kUnsupported, r;
  }
  if (half) return r;  // 16-bit storage: the planes-in-LDS kernel only (global atomics need f32 / f64)
  r.global = chunk_geometry(B, C, Hf * Wf, 16, kHalfFillWaves);
  return r.path = grid_ok(r.global.blocks) ? BeBwdPath::kGlobal : BeBwdPath::kUnsupported, r;
}
inline BeBwdRoute be_bwd_route(int elem_size, int acc_size, bool need_src, bool need_flow, int64_t B, int64_t C, int64_t Hs,
                               int64_t Ws, int64_t Hf, int64_t Wf, int k) {
  if (k >= 2 && k <= 5) return be_bwd_fixed_k_route(elem_size, acc_size, need_src, need_flow, B, C, Hs, Ws, Hf, Wf, k);
  BeBwdRoute r{};  // any other kernel size: one thread per grad_out element, the reference's decomposition
  if (elem_size != 2 && grid_ok(ceil_div(B * C * (k * Hf) * (k * Wf), kBlock))) r.path = BeBwdPath::kElem;
  return r;
}

// ==== planes-in-LDS kernels that need whole planes: unfold forward / backward, source_bwd ================================
// G = 0: not taken (k > 5, planes beyond the budget, or a grid that overflows).  mode = kGoutUnfold / kGoutAttn /
// kGoutUnfoldAttn for the backward forms (be_bwd_lds_kernel), whose entry points check scatter_gather_planes_fit first.
inline PlaneGeo unfold_fwd_route(int acc_size, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf, int k) {
  PlaneGeo g = k <= 5 ? unfold_fwd_geometry(acc_size, B, C, Hs, Ws, Hf, Wf) : PlaneGeo{0, 0, 1, 0, 0, -1};
  if (!grid_ok(plane_blocks(B, g))) g.G = 0;
  return g;
}
inline PlaneGeo whole_plane_bwd_route(int mode, int elem_size, int acc_size, bool need_src, bool need_flow, int64_t B, int64_t C,
                                      int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf, int k) {
  PlaneGeo g = k <= 5 ? be_bwd_lds_geometry(mode, elem_size, acc_size, need_src, need_flow, B, C, Hs, Ws, Hf, Wf, k)
                      : PlaneGeo{0, 0, 1, 0, 0, -1};
  if (!grid_ok(plane_blocks(B, g))) g.G = 0;
  return g;
}

// ==== resample2d forward ==================================================================================================
enum class RsFwdPath { kUnsupported, kBigTile, kBigGather, kLds, kGlobal };
struct RsFwdRoute {
  RsFwdPath path;
  BigGeo big;           // kBigTile: rs_gather_tile_kernel<T, KH, 0>
  BigGatherGeo gather;  // kBigGather: rs_fwd_big_kernel
  PlaneGeo lds;         // kLds: rs_lds_kernel<T, KH, 0, WIN = lds.margin >= 0>
  Geo global;           // kGlobal: rs_fwd_kernel
};
inline RsFwdRoute rs_fwd_route(int elem_size, int acc_size, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                               int k, int dil) {
  RsFwdRoute r{};
  if (tuning(GFLA_TUNE_RS) != 1) {
    if (big_plane_regime(2, B, C, Hi, Wi, acc_size)) {
      if (tuning(GFLA_TUNE_BIG_GATHER_V1) != 1 && elem_size >= 4 && Hi * Wi <= 0x3fffffffLL) {
        r.big = big_geometry(2, B, C, H, W, (k - 1) * dil + 1, acc_size);
        if (grid_ok(r.big.nwg)) return r.path = RsFwdPath::kBigTile, r;
      }
      r.gather = big_gather_geometry(B, C, H, W);
      if (grid_ok(r.gather.nwg)) return r.path = RsFwdPath::kBigGather, r;
    }
    r.lds = rs_gather_geometry(acc_size, B, C, Hi, Wi, H, W, k, dil, 1);
    if (r.lds.G > 0) return r.path = grid_ok(plane_blocks(B, r.lds)) ? RsFwdPath::kLds : RsFwdPath::kUnsupported, r;
  }
  r.global = chunk_geometry(B, C, H * W, 16, kFillWaves);
  return r.path = grid_ok(r.global.blocks) ? RsFwdPath::kGlobal : RsFwdPath::kUnsupported, r;
}

// ==== resample2d backward: d/d input1 (scatter) and d/d input2 (gather), both forms of the entry point ====================
// The path is one decision for both gradients (the planes-in-LDS kernels run only where BOTH their geometries exist); rows and
// keys: DESIGN.md 3.2.
// product: with scratch, dilation 1, f32, outside the big regime, d/d input1 is first offered to the matrix-core product
//   (patch_mfma.hip).  lds_fallback: the LDS scatter kernel exists, so the product decides ON THE DEVICE and the scatter
//   kernel is enqueued behind it as its fallback.  A product that declines (GFLA_ERR_UNSUPPORTED, nothing enqueued) is
//   followed by the route for product_allowed = false, and so is a product that took d/d input1 alone (want1 = false then).
// zero_fill: flag bit 1 of `trunc` = grad_in1 arrives uninitialised.  Honoured by the kernels where every element has
//   exactly one writer -- whole scatter planes with one owner each (split == 1, margin < 0), or the product alone -- and
//   zero-filled by the launcher (which then clears the bit) otherwise.
enum class RsBwdPath { kUnsupported, kBig, kLds, kGlobal };
struct RsBwdRoute {
  RsBwdPath path;
  bool product, lds_fallback, zero_fill;
  bool fix, tab;           // kLds scatter
  bool gather_tiles;       // kBig: rs_gather_tile_kernel<MODE 2> (else rs_bwd2_big_kernel)
  bool stream;             // kLds gather: agg_ga_stream_kernel<T, 3, 1> launched from `plan`
  BigGeo big1, big2;       // kBig: scatter tiles / gather tiles
  BigGatherGeo gather;     // kBig, !gather_tiles
  PlaneGeo lds1, lds2;     // kLds: scatter planes / gather planes
  AggStreamPlan plan;
  Geo global1, global2;    // kGlobal
};
inline RsBwdRoute rs_bwd_route(int elem_size, int acc_size, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                               int k, int dil, int trunc, bool want1, bool want2, bool workspace, bool product_allowed = true) {
  RsBwdRoute r{};
  const bool half = elem_size == 2, f32 = elem_size == 4, float_acc = acc_size == 4;
  const int span = (k - 1) * dil + 1;
  const bool big = !half && tuning(GFLA_TUNE_RS) != 1 && big_plane_regime(3, B, C, Hi, Wi, acc_size);
  r.lds1 = rs_scatter_geometry(elem_size, B, C, Hi, Wi, H, W, k, dil);
  r.lds2 = rs_gather_geometry(acc_size, B, C, Hi, Wi, H, W, k, dil, 0);
  const bool lds = (tuning(GFLA_TUNE_RS) != 1 || half) && r.lds1.G > 0 && r.lds2.G > 0;
  r.product = product_allowed && f32 && want1 && workspace && dil == 1 && tuning(GFLA_TUNE_RS) != 1 && !big;
  r.lds_fallback = r.product && lds;  // adaptive only where the LDS-atomic kernel exists as the device-side fallback
  if (big && Hi * Wi <= 0x3fffffffLL) {
    r.path = RsBwdPath::kBig;
    r.gather_tiles = tuning(GFLA_TUNE_BIG_GATHER_V1) != 1;
    r.big1 = big_geometry(3, B, C, H, W, span, big_plane_bytes(3, acc_size));
    r.big2 = big_geometry(4, B, C, H, W, span, acc_size);
    r.gather = big_gather_geometry(B, C, H, W);
    if ((want1 && !grid_ok(r.big1.nwg)) || (want2 && !grid_ok(r.gather_tiles ? r.big2.nwg : r.gather.nwg)))
      r.path = RsBwdPath::kUnsupported;
  } else if (lds) {
    r.path = RsBwdPath::kLds;
    r.fix = float_acc && !(f32 && tuning(GFLA_TUNE_RS_BWD1_PLANES) == 1);
    r.tab = f32 && workspace && k / 2 == 2 && Hi <= 65535 && Wi <= 65535 && tuning(GFLA_TUNE_RS_BWD1_PLANES) == 0;
    // B C H W < 2^31: a bound the streaming route has always had (the kernel indexes the flow map in 64 bits; dropping it
    // would move calls onto another kernel)
    r.stream = float_acc && k == 4 && dil == 1 && tuning(GFLA_TUNE_RS_BWD2_NO_STREAM) != 1 && agg_stream_enabled() &&
               agg_stream_shape_ok(B, C, Hi, Wi, 3, true) && B * C * H * W < (1LL << 31) &&
               agg_stream_plan(B, C, Hi, Wi, H, W, 3, r.plan);
    if ((want1 && !grid_ok(plane_blocks(B, r.lds1))) || (want2 && !r.stream && !grid_ok(plane_blocks(B, r.lds2))))
      r.path = RsBwdPath::kUnsupported;
  } else if (!half) {
    r.path = RsBwdPath::kGlobal;
    r.global1 = chunk_geometry(B, C, H * W, 16, kFillWaves);
    r.global2 = chunk_geometry(B, C, H * W, 512, kHalfFillWaves);
    if ((want1 && !grid_ok(r.global1.blocks)) || (want2 && !grid_ok(r.global2.blocks))) r.path = RsBwdPath::kUnsupported;
  }
  const bool sole_writer = (r.path == RsBwdPath::kLds && r.lds1.split == 1 && r.lds1.margin < 0) || (r.product && !r.lds_fallback);
  r.zero_fill = want1 && (trunc & 2) != 0 && !sole_writer;
  return r;
}

// ==== local_attn_aggregate forward ========================================================================================
// kStream: coefficient table + streaming kernel; the table lives in the caller's workspace.
enum class AggFwdPath { kUnsupported, kStream, kLds, kGlobal };
struct AggFwdRoute {
  AggFwdPath path;
  AggStreamPlan plan;  // kStream
  PlaneGeo lds;        // kLds: agg_fwd_lds_kernel
  Geo global;          // kGlobal: agg_fwd_kernel
};
inline AggFwdRoute agg_fwd_route(int acc_size, bool workspace, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W,
                                 int k) {
  AggFwdRoute r{};
  if (acc_size == 4 && workspace && agg_stream_wanted(k) && agg_stream_shape_ok(B, C, Hs, Ws, k, true) &&
      agg_stream_plan(B, C, Hs, Ws, H, W, k, r.plan))
    return r.path = AggFwdPath::kStream, r;
  if (tuning(GFLA_TUNE_AGG) != 1) {
    r.lds = plane_geometry(Hs * Ws, acc_size, B, C, H * W, true, kAggChunk);
    if (r.lds.G > 0) return r.path = grid_ok(plane_blocks(B, r.lds)) ? AggFwdPath::kLds : AggFwdPath::kUnsupported, r;
  }
  r.global = chunk_geometry(B, C, H * W, 32, kFillWaves);
  return r.path = grid_ok(r.global.blocks) ? AggFwdPath::kGlobal : AggFwdPath::kUnsupported, r;
}

// ==== local_attn_aggregate backward =======================================================================================
// d/d a_ij [+ d/d flow] pass (launch_agg_ga): the streaming kernel (float arithmetic; no coefficient pass here, so no bound
// on B), else agg_ga_lds_kernel with the channels split until the launch has >= 4 workgroups per CU.
enum class AggGaPath { kUnsupported, kStream, kLds };
struct AggGaRoute {
  AggGaPath path;
  AggStreamPlan plan;                       // kStream
  int G, nsuper, CS, ntiles;                // kLds
  int64_t blocks, padded;                   // (the XCD remap needs a multiple of 8 workgroups)
  unsigned lds_bytes;
};
inline AggGaRoute agg_ga_route(int acc_size, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int k) {
  AggGaRoute r{};
  if (acc_size == 4 && agg_stream_wanted(k) && agg_stream_shape_ok(B, C, Hs, Ws, k, false) &&
      agg_stream_plan(B, C, Hs, Ws, H, W, k, r.plan))
    return r.path = AggGaPath::kStream, r;
  const int64_t ntiles = ceil_div(H * W, 512);
  int64_t G = lds_budget() / (Hs * Ws * (int64_t)acc_size);
  if (G < 1) return r;
  if (G > C) G = C;
  int64_t nsuper = 1;
  while (B * ntiles * nsuper < 4 * kNumCU && nsuper * 2 * G <= C) nsuper *= 2;
  const int64_t CS = ceil_div(C, nsuper);
  nsuper = ceil_div(C, CS);
  if (G > CS) G = CS;
  r.G = (int)G, r.nsuper = (int)nsuper, r.CS = (int)CS, r.ntiles = (int)ntiles;
  r.blocks = B * nsuper * ntiles;
  r.padded = ceil_div(r.blocks, kNumXCD) * kNumXCD;
  r.lds_bytes = (unsigned)(G * Hs * Ws * acc_size);
  if (grid_ok(r.blocks)) r.path = AggGaPath::kLds;
  return r;
}
// kLds: (1) grad_source + grad_flow = block_extractor backward of the factored gradient a_ij * g_c / k^2 (be_bwd_lds_kernel,
// whole planes), (2) grad_logits from the d/d a_ij pass.  kGlobal: agg_bwd_kernel (f32 / f64 only).  key 3 = 1 forces the
// global kernel -- except for 16-bit storage, which exists for the planes-in-LDS kernels only.
// product (f32, scratch, grad_source wanted, key 3 != 1, gather planes fit or nothing else wanted): d/d source is first
// offered to the matrix-core product (patch_mfma.hip); d/d flow then comes out of the d/d a_ij pass, which holds the patch
// sums it needs.  lds_fallback: as for resample2d, the LDS scatter kernel (grad_source only: `fallback`) behind the product.
// A product that declines is followed by `path`.
enum class AggBwdPath { kUnsupported, kLds, kGlobal };
struct AggBwdRoute {
  AggBwdPath path;
  bool product, lds_fallback;
  PlaneGeo scatter, fallback;  // be_bwd_lds_kernel<..., kGoutAttn, false>: kLds (wanted gradients) / behind the product
  Geo global;
};
inline AggBwdRoute agg_bwd_route(int elem_size, int acc_size, bool need_src, bool need_flow, bool need_logits, bool workspace,
                                 int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int k) {
  AggBwdRoute r{};
  const bool half = elem_size == 2, fit = scatter_gather_planes_fit(Hs, Ws, acc_size);
  r.product = elem_size == 4 && need_src && workspace && tuning(GFLA_TUNE_AGG) != 1 &&
              (Hs * Ws * (int64_t)acc_size <= lds_budget() || (!need_flow && !need_logits));
  r.lds_fallback = r.product && fit;
  if (r.lds_fallback) r.fallback = whole_plane_bwd_route(kGoutAttn, elem_size, acc_size, true, false, B, C, Hs, Ws, H, W, k);
  if ((tuning(GFLA_TUNE_AGG) != 1 || half) && fit) {
    r.path = AggBwdPath::kLds;
    if (need_src || need_flow) {
      r.scatter = whole_plane_bwd_route(kGoutAttn, elem_size, acc_size, need_src, need_flow, B, C, Hs, Ws, H, W, k);
      if (r.scatter.G == 0) r.path = AggBwdPath::kUnsupported;
    }
  } else if (!half) {
    r.global = chunk_geometry(B, C, H * W, 32, kHalfFillWaves);
    if (grid_ok(r.global.blocks)) r.path = AggBwdPath::kGlobal;
  }
  return r;
}

}  // namespace gfla
