// Host-side queries of the gather/scatter ops' routing (no GPU needed: the CPU tests sweep them, the Python layer routes
// 16-bit training by the two *_supported answers).  Every answer comes from the route function the launcher of that
// family executes (gs_route.h), under the tuning keys as they are right now.
#include "gs_route.h"

extern "C" {
/* Launch geometry of the planes-in-LDS kernels (include/gfla_lds_plane.h).  G = 0: the route does not take the family's
 * planes-in-LDS kernel for this call.  Ops 0-3 are be_bwd_lds_kernel by the form of its gradient (kGoutTensor, kGoutAttn,
 * kGoutUnfold, kGoutUnfoldAttn).  Op 0 answers for every k <= 5 from the route of the compile-time kernel sizes; k = 1 has no
 * instantiation of the tensor form (gfla_block_extractor_bwd_* takes the per-element kernel there) and is answered as the
 * query always has. */
int gfla_lds_plane_geometry(int op, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int k, int dilation,
                            int elem_size, int needs, int64_t *out) {
  using namespace gfla;
  if (!out) return GFLA_ERR_NULL_POINTER;
  if (op < 0 || op > 7 || B <= 0 || C <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || k < 1 || dilation < 1 ||
      (elem_size != 2 && elem_size != 4 && elem_size != 8) || (op <= 3 && (needs & 3) == 0) || (op >= 5 && k < 2))
    return GFLA_ERR_BAD_SHAPE;
  const int acc = elem_size == 8 ? 8 : 4;
  const bool need_src = (needs & 1) != 0, need_flow = (needs & 2) != 0;
  PlaneGeo g{0, 0, 1, 0, 0, -1};
  if (op == 0) {
    if (k <= 5) {
      const BeBwdRoute r = be_bwd_fixed_k_route(elem_size, acc, need_src, need_flow, B, C, Hs, Ws, H, W, k);
      if (r.path == BeBwdPath::kLds) g = r.lds;
    }
  } else if (op <= 3) {
    g = whole_plane_bwd_route(op, elem_size, acc, need_src, need_flow, B, C, Hs, Ws, H, W, k);
  } else if (op == 4) {
    g = unfold_fwd_route(acc, B, C, Hs, Ws, H, W, k);
  } else if (op == 5) {
    const RsFwdRoute r = rs_fwd_route(elem_size, acc, B, C, Hs, Ws, H, W, k, dilation);
    if (r.path == RsFwdPath::kLds) g = r.lds;
  } else {
    const RsBwdRoute r = rs_bwd_route(elem_size, acc, B, C, Hs, Ws, H, W, k, dilation, 0, true, true, false);
    if (r.path == RsBwdPath::kLds) g = op == 6 ? r.lds1 : r.lds2;
  }
  const int64_t v[6] = {g.G, g.ngroups, g.split, g.per, g.margin, g.lds_bytes};
  for (int i = 0; i < 6; ++i) out[i] = g.G > 0 ? v[i] : 0;
  return GFLA_OK;
}

/* Launch geometry of the big-plane tile kernels (csrc/tile_map.h).
 * op: 0 block_extractor forward, 1 block_extractor backward (both gradients), 2 resample2d forward, 3 resample2d d/d input1,
 * 4 resample2d d/d input2.  (H, W) = the flow / output grid, (Hs, Ws) = the source plane, span = taps per axis (kernel_size
 * + 1 for block_extractor, (kernel_size - 1) * dilation + 1 for resample2d), elem_size 4 / 8.
 * out[10] = in the regime by default (0 / 1), tile rows, tile columns, tiles along x, tiles along y, threads per workgroup,
 * channels per workgroup, channel groups, dynamic LDS bytes requested, workgroups. */
int gfla_big_plane_geometry(int op, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int span,
                            int elem_size, int64_t *out) {
  if (!out) return GFLA_ERR_NULL_POINTER;
  if (op < 0 || op > 4 || B <= 0 || C <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || span < 1 || (elem_size != 4 && elem_size != 8))
    return GFLA_ERR_BAD_SHAPE;
  gfla::big_plane_answer(op, B, C, Hs, Ws, H, W, span, elem_size, out);
  return GFLA_OK;
}
/* The workgroup -> work-item remap of those kernels (a bijection of [0, nwg) that hands the blocks of each of the 8 XCDs a
 * contiguous range); -1 outside [0, nwg). */
int64_t gfla_xcd_swizzle(int64_t block, int64_t nwg) {
  return (block < 0 || block >= nwg) ? -1 : gfla::xcd_swizzle(block, nwg);
}

/* 1 when gfla_block_extractor_unfold_bwd_<storage> and gfla_local_attn_source_bwd_<storage> take source planes of Hs x Ws at
 * this kernel size (elem_size 2 / 4 / 8): the entry points' own test, then the route on a single plane. */
int gfla_unfold_supported(int64_t Hs, int64_t Ws, int k, int elem_size) {
  const int acc = elem_size == 8 ? 8 : 4;
  return (k >= 1 && Hs > 0 && Ws > 0 && gfla::scatter_gather_planes_fit(Hs, Ws, acc) &&
          gfla::whole_plane_bwd_route(gfla::kGoutUnfold, elem_size, acc, true, true, 1, 1, Hs, Ws, Hs, Ws, k).G > 0) ? 1 : 0;
}
/* 1 when gfla_local_attn_aggregate_bwd_<storage> takes source planes of Hs x Ws (elem_size 2 = bf16 / f16, 4 = f32, 8 = f64).
 * f32 / f64 always do (global-memory kernels behind the planes-in-LDS ones); 16-bit storage exists for the planes-in-LDS
 * kernels only.  The host side asks here instead of duplicating the budget. */
int gfla_aggregate_bwd_supported(int64_t Hs, int64_t Ws, int elem_size) {
  if (Hs <= 0 || Ws <= 0 || (elem_size != 2 && elem_size != 4 && elem_size != 8)) return 0;
  const int acc = elem_size == 8 ? 8 : 4;
  return gfla::agg_bwd_route(elem_size, acc, true, true, true, false, 1, 1, Hs, Ws, Hs, Ws, 1).path != gfla::AggBwdPath::kUnsupported;
}
}
