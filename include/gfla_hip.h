/*
 * gfla_hip.h -- C ABI of libgfla_hip.so, the MI355X (gfx950) implementation of the
 * Global-Flow-Local-Attention feature-warping hot path.
 *
 * This is the drop-in boundary.  Each entry point replaces one `forward`/`backward` of the
 * reference's three pybind modules (paths relative to the reference checkout):
 *
 *   block_extractor_cuda      model/networks/block_extractor/block_extractor_cuda.cc:5-33
 *   local_attn_reshape_cuda   model/networks/local_attn_reshape/local_attn_reshape_cuda.cc:5-29
 *   resample2d_cuda           model/networks/resample2d_package/resample2d_cuda.cc:6-33
 *
 * plus one fused entry point pair for the softmax -> reshape -> multiply -> avg_pool tail of
 * ExtractorAttn.forward (model/networks/base_function.py:803,808-809), which the reference runs
 * as four separate torch/custom ops.
 *
 * Conventions (all entry points):
 *   - plain device pointers + sizes; no torch types; tensors are contiguous NCHW, exactly what
 *     the reference wrappers assert (block_extractor.py:9-10, local_attn_reshape.py:9,
 *     resample2d.py:10-11);
 *   - the caller owns every buffer (the reference allocates outputs in Function.forward,
 *     block_extractor.py:21, local_attn_reshape.py:18, resample2d.py:19); the library never
 *     allocates, never synchronises, never touches the host copy of the data;
 *   - `stream` is a hipStream_t (NULL = the null stream); kernels are enqueued asynchronously
 *     on it, the way the reference enqueues on the current torch stream
 *     (block_extractor_kernel.cu:197);
 *   - return 0 on success, a negative gfla_status otherwise (the reference returns 1 always and
 *     swallows launch errors, block_extractor_cuda.cc:11, block_extractor_kernel.cu:215);
 *   - suffix = storage type: _f32, _f64 (the two types the reference dispatches,
 *     AT_DISPATCH_FLOATING_TYPES), _bf16 and _f16 (new, 16-bit storage: forward AND backward, fp32 arithmetic inside,
 *     reductions over channels returned in float32).  bf16 / f16 buffers are raw uint16_t bit patterns; f16 is IEEE
 *     binary16 (stores round to nearest even, overflow to +-inf, subnormals kept);
 *   - pointer placement: a tensor pointer need only be aligned to its element type.  An entry point computes the same
 *     result wherever its tensors lie (a contiguous view that starts inside a larger buffer is as good as a fresh
 *     allocation; the 16-byte vector paths are chosen per pointer, DESIGN.md "Pointer placement" lists per op what is
 *     bit-equal to the aligned call), reads nothing before the first and writes nothing behind the last element of a
 *     buffer.  A pointer that is not aligned to its element type is refused with GFLA_ERR_UNSUPPORTED before anything is
 *     launched by the entry points that inspect their pointers (instance norm, the generator convolutions); elsewhere it
 *     is outside the ABI.  Workspaces (`workspace`, `scratch`, `packed`) are different: they want the alignment their
 *     entry point states, 256 bytes where it states none -- what every allocator of device memory returns.
 */
#ifndef GFLA_HIP_H_
#define GFLA_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gfla_status {
  GFLA_OK = 0,
  GFLA_ERR_NULL_POINTER = -1,   /* a required buffer is NULL */
  GFLA_ERR_BAD_SHAPE = -2,      /* non-positive dimension, kernel_size < 1, C != k*k ... */
  GFLA_ERR_UNSUPPORTED = -3,    /* shape is valid but outside what the kernels index */
  GFLA_ERR_LAUNCH = -4          /* hipGetLastError() reported a failure after the launch */
} gfla_status;

typedef void *gfla_stream_t; /* hipStream_t */

/* Bumped whenever an entry point is added or a signature changes.
 *   1: round 1 (the three ops + aggregate)   2: round 2 (fc_*, *_ws, bf16 backward, max_cosine, correctness_map)
 *   3: round 3 (gfla_path_count, process-global tuning, arithmetic mode 4)
 *   4: round 3 (gfla_fc_kernel_f32 which = 6 / 7; the scatter workspace also carries resample2d's tap records)
 *   5: round 4 (gfla_aggregate_bwd_supported, gfla_mask_blend_*; tuning keys 24, 25 and 27; path id GFLA_PATH_BE_FWD_PIX)
 *   6: round 4 (gfla_convert_multi)
 *   7: round 5 (path ids 13-17, tuning keys 30-41: the big-plane kernels of csrc/tile_map.h; gfla_big_plane_geometry,
 *      gfla_xcd_swizzle)
 *   8: round 6 (arithmetic mode 5 of gfla_fc_*: Winograd domain with two-term f16 operands on the f16 matrix cores,
 *      csrc/fc_wino16.hip; path ids 18 / 19; tuning keys 43, 46, 49, 52); float16 storage (the _f16 entry points,
 *      gfla_fc_forward_f16, gfla_convert_multi flags 2 / 3, path id 21) only ADDS symbols and ids and keeps 8; so do
 *      gfla_max_cosine_fwd_f16 / _bf16, gfla_correctness_map_{fwd,bwd}_f16 / _bf16, gfla_affine_reg_*,
 *      gfla_gram_l1_* and gfla_flow_warp_* */
#define GFLA_ABI_VERSION 8
int gfla_abi_version(void);
const char *gfla_status_string(int status);

/* Tuning knobs (benchmarks / tests only; defaults are chosen per shape).  Process-global.  gfla_set_tuning returns the
 * old value; a key that is no enumerator is accepted and changes nothing (no kernel reads it; outside 0 .. 63 it is not
 * even stored and 0 comes back).  Every key defaults to 0.  The kernels read a key by its name (csrc:
 * tuning(GFLA_TUNE_X)); Python sees TUNE_X and refuses a number that is no enumerator.  Each entry: what it selects, its
 * values, [who reads it]. */
enum gfla_tuning_key {
  /* block_extractor forward kernel.  0 auto (few planes beyond the LDS budget -> the tile kernels, see BIG_PLANE; planes
   * in LDS when they fit: flow rows of up to 64 pixels -> the wave-per-flow-row kernel, csrc/be_fwd_wrow.h, small output
   * planes and wider rows -> the lane-per-pixel kernel, csrc/be_fwd_pix.h), 1 force the global-gather kernel, 2 force
   * round 1's planes-in-LDS kernel (lane = four consecutive outputs), 3 force the lane-per-pixel kernel, 4 force the
   * wave-per-flow-row kernel.  [gs_route.h: be_fwd_route] */
  GFLA_TUNE_BE_FWD = 0,
  /* channels per thread of the global-memory kernels (0 auto).  [gs_route.h: chunk_geometry] */
  GFLA_TUNE_GLOBAL_CPT = 1,
  /* block_extractor backward.  0 auto, 1 force the global-atomics kernel (16-bit storage has none and keeps the
   * planes-in-LDS kernel).  [gs_route.h: be_bwd_fixed_k_route] */
  GFLA_TUNE_BE_BWD = 2,
  /* local_attn_aggregate forward / backward.  0 auto, 1 force the global kernels: no stream kernels, no matrix-core
   * product (16-bit storage keeps the planes-in-LDS backward).  [gs_route.h: agg_stream_enabled, agg_fwd_route,
   * agg_bwd_route] */
  GFLA_TUNE_AGG = 3,
  /* cap on G, the channel planes one workgroup keeps in LDS (0 auto).  [lds_plane.h: plane_geometry -- every
   * planes-in-LDS kernel; be_fwd_pix.h: pix_geometry; be_fwd_wrow.h: wrow_geometry; agg_stream.h: agg_stream_geometry,
   * where it caps CH, the planes of one staged chunk] */
  GFLA_TUNE_G_CAP = 4,
  /* split (0 auto).  [lds_plane.h: plane_geometry and be_fwd_pix.h: pix_geometry -- workgroups sharing one (b, channel
   * group); ignored where a kernel cannot split: the 16-bit backward kernels flush each plane from one owner
   * (block_extractor / aggregation / unfold backward, resample2d d/d input1) and keep split = 1.  max_cosine.hip: splitM,
   * the units the source positions of one (b, target tile) are cut into.  agg_stream.h: agg_stream_geometry -- ns, the
   * channel ranges] */
  GFLA_TUNE_SPLIT = 5,
  /* resample2d forward / backward.  0 auto, 1 force the global kernels: no tile kernels, no matrix-core product (16-bit
   * storage keeps the planes-in-LDS backward).  [gs_route.h: rs_fwd_route, rs_bwd_route] */
  GFLA_TUNE_RS = 6,
  /* row windows for planes larger than the LDS budget.  0 on, 1 off (the global kernels).  [gs_route.h: lds_geometry] */
  GFLA_TUNE_NO_WINDOWS = 7,
  /* aggregation stream kernels (csrc/agg_stream.h).  0 auto (the aggregation from k = 5; resample2d d/d input2 at k = 4),
   * 1 off (round 1's kernels: the tests' reference), 2 the aggregation takes them for every odd k.  [gs_route.h:
   * agg_stream_enabled, agg_stream_wanted] */
  GFLA_TUNE_AGG_STREAM = 8,
  /* stream kernels: threads per workgroup, 64 per tile (0 auto; multiples of 64 up to 64 x kAggStreamWaves).
   * [agg_stream.h: agg_stream_geometry] */
  GFLA_TUNE_AGG_STREAM_THREADS = 9,
  /* LDS budget per workgroup in KB (0 = 64; 16 .. 160).  [lds_plane.h: lds_budget -- every planes-in-LDS / window / tile
   * geometry and the big-plane regime.  be_fwd_wrow.h: wrow_geometry keeps its own 78 KB (two workgroups per CU) unless
   * the key is >= 16, then takes this budget] */
  GFLA_TUNE_LDS_KB = 10,
  /* direct FC convolutions: row blocks of 32 output pixels per tile (0 auto; kFcMinRowBlocks .. kFcMaxRowBlocks).
   * [fc_conv_impl.h: pick_conv_tiling] */
  GFLA_TUNE_FC_ROW_BLOCKS = 11,
  /* FC weight gradients: partial sums (workgroups) per input chunk (0 auto).  [fc_gemm.hip: fc_wgrad_splits;
   * fc_wino.hip: fc_wino_wgrad_splits] */
  GFLA_TUNE_FC_WGRAD_SPLITS = 12,
  /* matrix-core scatter: source rows per band (0 auto: 96 / Ws, up to six 32-column blocks for wide planes).
   * [patch_mfma.hip: pm_geometry] */
  GFLA_TUNE_PM_BAND_ROWS = 13,
  /* matrix-core scatter (d/d source of the aggregation, resample2d d/d input1).  0 where it measured faster, 1 never
   * (the LDS-atomic kernels), 2 wherever the shape is supported.  [patch_mfma.hip: pm_auto, pm_supported] */
  GFLA_TUNE_PM = 14,
  /* matrix-core scatter, adaptive dispatch: source rows a flow tile may reach on average before the LDS-atomic fallback
   * takes over (0 = 2.6 x the rows reached under a constant flow; >= 100000 = always the matrix-core path).
   * [patch_mfma.hip: pm_limit] */
  GFLA_TUNE_PM_LIMIT_ROWS = 15,
  /* stream kernels: tile width 8, 16 or 32 (anything else: the width that wastes the fewest lanes).  [agg_stream.h:
   * agg_stream_geometry] */
  GFLA_TUNE_AGG_STREAM_TILE_W = 16,
  /* stream kernels, experiment: pitch of a staged row pair in words (a multiple of 4, >= 2 Ws; anything else: auto).
   * [agg_stream.h: agg_stream_geometry] */
  GFLA_TUNE_AGG_STREAM_PITCH = 17,
  /* Retired -- accepted and ignored.  Keys 19, 43, 49 and 52 selected FC kernels that later rounds measured and
   * replaced (the direct weight gradient in mode 4; in mode 5 the two-term f16 Winograd kernels for the k = 3 data
   * gradient and for every convolution, the float32 k = 5 weight gradient).  The FC kernel plan is a function of the
   * call's shape and mode alone (csrc/fc_block.hip: fc_plan). */
  GFLA_TUNE_RETIRED_19 = 19,
  /* timing ablations of the Winograd kernels -- only in `make PROBES=1` builds (results are garbage;
   * tools/probe_wino.py); a default build ignores the key.  Bits 1 .. 16: the float32 k = 5 convolution; 32 + bits: the
   * float32 k = 5 weight gradient; 64 + bits: the two-term f16 k = 5 weight gradient.  [fc_wino.hip: wn_launch,
   * fc_wino_wgrad_jobs; fc_wino16.hip: fc_wino16_wgrad_jobs] */
  GFLA_TUNE_WINO_PROBE = 20,
  /* Winograd convolutions.  1 a single raw buffer in LDS, never two; 2 one launch per half instead of both halves in
   * one, which also separates the two weight-gradient kernels of a layer again.  [fc_wino_shared.h: wn_plan;
   * fc_wino.hip: fc_wino_conv_jobs; fc_wino16.hip: fc_wino16_conv_jobs; fc_block.hip: fc_plan] */
  GFLA_TUNE_WINO_LAUNCH = 21,
  /* resample2d d/d input2 at k = 4.  0 the stream kernel, 1 the planes-in-LDS gather.  [gs_route.h: rs_bwd_route] */
  GFLA_TUNE_RS_BWD2_NO_STREAM = 22,
  /* resample2d d/d input1, planes-in-LDS scatter (float32).  0 fixed point + tap records (with scratch), 1 double planes
   * (round 1), 2 fixed point without the table.  [gs_route.h: rs_bwd_route] */
  GFLA_TUNE_RS_BWD1_PLANES = 23,
  /* be_fwd_pix_kernel / be_fwd_wrow_kernel: threads per workgroup (0 auto; multiples of 64 up to 1024; a count the
   * wave-per-flow-row kernel's LDS cannot hold sends the call to the next kernel).  [be_fwd_pix.h: pix_geometry;
   * be_fwd_wrow.h: wrow_geometry] */
  GFLA_TUNE_BE_FWD_THREADS = 24,
  /* be_fwd_pix_kernel: 1 = non-temporal output stores (A/B only: half the rate).  [be_fwd_pix.h: launch_fwd_pix] */
  GFLA_TUNE_BE_FWD_PIX_NT = 25,
  /* timing ablations of the two round-4 block_extractor forward kernels -- only in `make PROBES=1` builds (results are
   * garbage); a default build ignores the key.  Bit 0 = no patch reads, bit 1 = no output stores.  [be_fwd_pix.h:
   * launch_fwd_pix; be_fwd_wrow.h: launch_fwd_wrow] */
  GFLA_TUNE_BE_FWD_PROBE = 27,
  /* Winograd-domain weight gradient, work units.  0 whole tile rows per unit where that needs fewer 16-tile steps
   * (csrc/fc_wino_wgrad.h: MR), 1 one tile row per unit everywhere (round 3), 2 whole tile rows of at most 16 tiles.
   * [fc_wino.hip: ww_geometry] */
  GFLA_TUNE_WINO_WGRAD_UNITS = 29,
  /* big-plane kernels (few planes, each beyond the LDS budget: csrc/tile_map.h).  0 auto, 1 never (round 1's row-window
   * kernels), 2 always (tests drive them at small shapes).  [gs_route.h: big_plane_regime] */
  GFLA_TUNE_BIG_PLANE = 30,
  /* rows of a tile of the big-plane kernels but block_extractor's forward (0 auto: 16; resample2d d/d input2 8; rows x
   * columns at most 512 pixels).  [tile_map.h: tile_geometry] */
  GFLA_TUNE_TILE_ROWS = 31,
  /* columns of such a tile (0 auto: 32; resample2d forward 16; at most 512).  [tile_map.h: tile_geometry] */
  GFLA_TUNE_TILE_COLS = 32,
  /* first-version gathers of the big-plane regime (BIG_GATHER_V1): channels per wave / thread (0 auto).  [be_tile.h:
   * big_channels_per_wave; gs_route.h: big_gather_geometry] */
  GFLA_TUNE_BIG_GATHER_CPW = 33,
  /* channels per workgroup of the scatter tiles -- block_extractor backward, resample2d d/d input1 (0 auto: 8, 4 for
   * block_extractor at k >= 5, halved while the launch is short of workgroups).  [tile_map.h: big_geometry through
   * tile_channels] */
  GFLA_TUNE_SCATTER_TILE_CHANNELS = 34,
  /* rows of a tile of block_extractor's forward (0 auto: 8; rows x columns at most 512 pixels).  [tile_map.h:
   * row_tile_geometry] */
  GFLA_TUNE_BE_FWD_TILE_ROWS = 35,
  /* columns of such a tile (0 auto: 32).  [tile_map.h: row_tile_geometry] */
  GFLA_TUNE_BE_FWD_TILE_COLS = 36,
  /* channels per workgroup of the gather tiles -- block_extractor forward, resample2d forward and d/d input2 (0 auto:
   * 8, 8, 16, halved while the launch is short of workgroups).  [tile_map.h: big_geometry through tile_channels] */
  GFLA_TUNE_GATHER_TILE_CHANNELS = 37,
  /* 1 = the first version of the big-plane gathers (taps read from global memory, no LDS window): block_extractor
   * forward, resample2d forward and d/d input2.  [gs_route.h: be_fwd_route, rs_fwd_route, rs_bwd_route] */
  GFLA_TUNE_BIG_GATHER_V1 = 38,
  /* timing ablations of the tile kernels -- only in `make PROBES=1` builds (results are garbage); a default build
   * ignores the key.  [tile_map.h: tile_probe_bits] */
  GFLA_TUNE_TILE_PROBE = 39,
  /* block_extractor's forward tiles, float arithmetic: channels evaluated together per pixel, 1, 2 or 4 (anything else:
   * auto).  [be_tile.h: launch_fwd_tile] */
  GFLA_TUNE_BE_FWD_TILE_CHUNK = 40,
  /* 1 = block_extractor's backward tiles without the cross-lane fold of the patch rows (csrc/be_tile.h: BeLinks).
   * [be_tile.h: launch_be_bwd_tile] */
  GFLA_TUNE_BE_BWD_TILE_NO_FOLD = 41,
  GFLA_TUNE_RETIRED_43 = 43, /* retired, see RETIRED_19: accepted and ignored */
  /* Winograd convolutions: 1 = groups of 32 tiles always, never whole tile rows on narrow maps.  [fc_wino_shared.h:
   * wn_geometry] */
  GFLA_TUNE_WINO_GROUP_32 = 44,
  /* 1 = gfla_fc_backward_f32 scatters the gradient of the convolved source map with global float atomics (round 2)
   * instead of the owner-computes kernel of round 6 (csrc/fc_sample.hip: fc_scatter_own_kernel).  [fc_block.hip:
   * fc_plan] */
  GFLA_TUNE_FC_SCATTER_ATOMICS = 46,
  GFLA_TUNE_RETIRED_49 = 49, /* retired, see RETIRED_19: accepted and ignored */
  GFLA_TUNE_RETIRED_52 = 52  /* retired, see RETIRED_19: accepted and ignored */
};
int gfla_set_tuning(int key, int value);

/* Dispatch trace (tests): number of times a kernel path has been enqueued by this process, from any host thread
 * (autograd runs backward on its own worker threads).  -1 for an unknown id. */
enum gfla_path {
  GFLA_PATH_BE_BWD_LDS = 0,     /* block_extractor backward: planes-in-LDS kernel */
  GFLA_PATH_BE_BWD_GLOBAL = 1,  /* block_extractor backward: global-atomics kernel (tuning key 2) */
  GFLA_PATH_FC_FWD_MODE0 = 2,   /* gfla_fc_forward_f32 in arithmetic mode 0 .. 4 = ids 2 .. 6 */
  GFLA_PATH_FC_FWD_MODE1 = 3,
  GFLA_PATH_FC_FWD_MODE2 = 4,
  GFLA_PATH_FC_FWD_MODE3 = 5,
  GFLA_PATH_FC_FWD_MODE4 = 6,
  GFLA_PATH_FC_BWD_MODE0 = 7,   /* gfla_fc_backward_f32, ids 7 .. 11 */
  GFLA_PATH_FC_BWD_MODE1 = 8,
  GFLA_PATH_FC_BWD_MODE2 = 9,
  GFLA_PATH_FC_BWD_MODE3 = 10,
  GFLA_PATH_FC_BWD_MODE4 = 11,
  GFLA_PATH_BE_FWD_PIX = 12,   /* block_extractor forward: lane = flow pixel, padded planes in LDS (round 4) */
  GFLA_PATH_BE_FWD_GPIX = 13,  /* round 5, few planes beyond the LDS budget (csrc/tile_map.h): block_extractor forward */
  GFLA_PATH_BE_BWD_TILE = 14,  /*   block_extractor backward, flow-pixel tiles with bounding-box LDS windows */
  GFLA_PATH_RS_FWD_BIG = 15,   /*   resample2d forward */
  GFLA_PATH_RS_BWD1_TILE = 16, /*   resample2d d/d input1, tiles with bounding-box LDS windows */
  GFLA_PATH_RS_BWD2_BIG = 17,  /*   resample2d d/d input2 */
  GFLA_PATH_FC_FWD_MODE5 = 18, /* round 6: gfla_fc_forward_f32 / gfla_fc_backward_f32 in arithmetic mode 5 */
  GFLA_PATH_FC_BWD_MODE5 = 19,
  GFLA_PATH_GEMM_F64 = 20,     /* gfla_gemm_f64 (float64 FC layers of ExtractorAttn on the FP64 matrix cores) */
  GFLA_PATH_FC_PACK_F16 = 21,  /* gfla_fc_forward_f16: activation records packed straight from the float16 maps */
  GFLA_PATH_COUNT = 22
};
int64_t gfla_path_count(int path);

/* Round 5, host logic of the big-plane tile kernels (csrc/tile_map.h), for tests -- no GPU needed.
 * gfla_big_plane_geometry: op 0 block_extractor forward, 1 block_extractor backward, 2 resample2d forward, 4 resample2d d/d input2,
 *   3 resample2d d/d input1; (H, W) the flow / output grid, (Hs, Ws) the source plane, span = taps per axis; out[10] = in the
 *   regime by default, tile rows, tile columns, tiles along x, tiles along y, threads per workgroup, channels per workgroup,
 *   channel groups, dynamic LDS bytes requested, workgroups.
 * gfla_xcd_swizzle: the block -> work item remap of those kernels (a bijection of [0, nwg)); -1 outside the range. */
int gfla_big_plane_geometry(int op, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int span,
                            int elem_size, int64_t *out);
int64_t gfla_xcd_swizzle(int64_t block, int64_t nwg);

/* ---- block_extractor ---------------------------------------------------------------------
 * forward : replaces block_extractor_cuda.forward(source, flow_field, output, kernel_size)
 *           (block_extractor_cuda.cc:5-12 -> block_extractor_kernel.cu:20-85)
 *   source (B,C,Hs,Ws)   flow (B,2,Hf,Wf): channel 0 = x, 1 = y displacement in source pixels
 *   out    (B,C,k*Hf,k*Wf), fully overwritten (need not be zeroed)
 * backward: replaces block_extractor_cuda.backward(source, flow_field, grad_output, grad_source,
 *           grad_flow_field, kernel_size) (block_extractor_cuda.cc:14-25 -> .cu:89-170)
 *   grad_source (B,C,Hs,Ws) is ACCUMULATED into and must arrive zeroed, as in the reference
 *   (block_extractor.py:35); grad_flow (B,2,Hf,Wf) likewise.  Either may be NULL to skip that
 *   gradient (the reference always computes both).                                             */
#define GFLA_DECL_BLOCK_EXTRACTOR(SFX, T)                                                          \
  int gfla_block_extractor_fwd_##SFX(const T *source, const T *flow, T *out, int64_t B, int64_t C, \
                                     int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf,               \
                                     int kernel_size, gfla_stream_t stream);
GFLA_DECL_BLOCK_EXTRACTOR(f32, float)
GFLA_DECL_BLOCK_EXTRACTOR(f64, double)
GFLA_DECL_BLOCK_EXTRACTOR(bf16, uint16_t)
GFLA_DECL_BLOCK_EXTRACTOR(f16, uint16_t)
#undef GFLA_DECL_BLOCK_EXTRACTOR

#define GFLA_DECL_BLOCK_EXTRACTOR_BWD(SFX, T)                                                      \
  int gfla_block_extractor_bwd_##SFX(const T *source, const T *flow, const T *grad_out,            \
                                     T *grad_source, T *grad_flow, int64_t B, int64_t C,           \
                                     int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf,               \
                                     int kernel_size, gfla_stream_t stream);
GFLA_DECL_BLOCK_EXTRACTOR_BWD(f32, float)
GFLA_DECL_BLOCK_EXTRACTOR_BWD(f64, double)
#undef GFLA_DECL_BLOCK_EXTRACTOR_BWD

/* ---- block_extractor, "unfold" layout (new; what the fused ExtractorAttn feeds its first FC layer) ----
 * Same samples as gfla_block_extractor_fwd, arranged as out (B, C*k*k, Hf, Wf) with channel index
 * c*k*k + i*k + j = tap (i,j) of source channel c, i.e. out_unfold[b, c*k*k+i*k+j, yf, xf] ==
 * out[b, c, yf*k+i, xf*k+j].  In this layout the stride-k convolution of ExtractorAttn
 * (base_function.py:800) is the batched GEMM  W(128, C*k*k) @ out_unfold[b](C*k*k, Hf*Wf)  and all
 * kernel traffic is coalesced along the pixel index.  layout = 1 stores (C*k*k, B, Hf, Wf) instead,
 * so the whole batch is ONE GEMM  W(128, C*k*k) @ out_unfold(C*k*k, B*Hf*Wf)  (and one each for the
 * data and weight gradients).  backward takes the gradient in the same layout;
 * grad_source / grad_flow accumulate (pass zeroed buffers), either may be NULL.
 * Only for kernel_size <= 5 and source planes that fit the LDS budget: gfla_unfold_supported() says
 * so (1/0); otherwise the entry points return GFLA_ERR_UNSUPPORTED and the caller uses the reference
 * layout.                                                                                          */
int gfla_unfold_supported(int64_t Hs, int64_t Ws, int kernel_size, int elem_size);
#define GFLA_DECL_UNFOLD_FWD(SFX, T)                                                               \
  int gfla_block_extractor_unfold_fwd_##SFX(const T *source, const T *flow, T *out_unfold,         \
                                            int64_t B, int64_t C, int64_t Hs, int64_t Ws,          \
                                            int64_t Hf, int64_t Wf, int kernel_size, int layout,   \
                                            gfla_stream_t stream);
GFLA_DECL_UNFOLD_FWD(f32, float)
GFLA_DECL_UNFOLD_FWD(f64, double)
GFLA_DECL_UNFOLD_FWD(bf16, uint16_t)
GFLA_DECL_UNFOLD_FWD(f16, uint16_t)
#undef GFLA_DECL_UNFOLD_FWD

#define GFLA_DECL_UNFOLD_BWD(SFX, T)                                                               \
  int gfla_block_extractor_unfold_bwd_##SFX(const T *source, const T *flow, const T *grad_unfold,  \
                                            T *grad_source, T *grad_flow, int64_t B, int64_t C,    \
                                            int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf,        \
                                            int kernel_size, int layout, gfla_stream_t stream);
GFLA_DECL_UNFOLD_BWD(f32, float)
GFLA_DECL_UNFOLD_BWD(f64, double)
#undef GFLA_DECL_UNFOLD_BWD

/* ---- local_attn_reshape ------------------------------------------------------------------
 * forward : replaces local_attn_reshape_cuda.forward(inputs, output, kernel_size)
 *           (local_attn_reshape_cuda.cc:5-11 -> local_attn_reshape_kernel.cu:20-61)
 *   in (B,k*k,H,W) -> out (B,1,k*H,k*W): out[b,0,ys*k+i,xs*k+j] = in[b,i*k+j,ys,xs]; bit-exact
 * backward: replaces local_attn_reshape_cuda.backward(inputs, grad_output, grad_inputs, k)
 *           (local_attn_reshape_cuda.cc:13-21 -> .cu:65-108); the inverse permutation.
 *   grad_in is fully OVERWRITTEN (the reference atomically adds into a zeroed buffer; the map
 *   is a bijection so the result is identical).                                                */
#define GFLA_DECL_RESHAPE(SFX, T)                                                                  \
  int gfla_local_attn_reshape_fwd_##SFX(const T *in, T *out, int64_t B, int64_t H, int64_t W,      \
                                        int kernel_size, gfla_stream_t stream);                    \
  int gfla_local_attn_reshape_bwd_##SFX(const T *grad_out, T *grad_in, int64_t B, int64_t H,       \
                                        int64_t W, int kernel_size, gfla_stream_t stream);
GFLA_DECL_RESHAPE(f32, float)
GFLA_DECL_RESHAPE(f64, double)
GFLA_DECL_RESHAPE(bf16, uint16_t)
GFLA_DECL_RESHAPE(f16, uint16_t)
#undef GFLA_DECL_RESHAPE

/* ---- resample2d --------------------------------------------------------------------------
 * forward : replaces resample2d_cuda.forward(input1, input2, output, kernel_size, dilation)
 *           (resample2d_cuda.cc:6-14 -> resample2d_kernel.cu:20-95)
 *   in1 (B,C,Hi,Wi)   in2 (B,3,H,W) = (dx, dy, sigma)   out (B,C,H,W), fully overwritten
 * backward: replaces resample2d_cuda.backward(input1, input2, gradOutput, gradInput1,
 *           gradInput2, kernel_size, dilation) (resample2d_cuda.cc:16-26 -> .cu:98-202, :204-330)
 *   grad_in1 (B,C,Hi,Wi) is ACCUMULATED into, must arrive zeroed (resample2d.py:32);
 *   grad_in2 (B,3,H,W) must arrive zeroed as well.  Either may be NULL.
 *   trunc_compat is a flag word.  Bit 0 set reproduces the reference's `xf - int(xf)` in the input1 gradient
 *   (resample2d_kernel.cu:137-138); clear uses floor, which is the true gradient of the forward.  Bit 1 set
 *   (GFLA_RESAMPLE_OVERWRITE_IN1): grad_in1 may arrive UNINITIALISED and is overwritten -- by plain stores where every
 *   element has exactly one writer, after an internal zero fill where the kernels have to accumulate with atomics.       */
#define GFLA_RESAMPLE_TRUNC_COMPAT 1
#define GFLA_RESAMPLE_OVERWRITE_IN1 2
#define GFLA_DECL_RESAMPLE_FWD(SFX, T)                                                             \
  int gfla_resample2d_fwd_##SFX(const T *in1, const T *in2, T *out, int64_t B, int64_t C,          \
                                int64_t Hi, int64_t Wi, int64_t H, int64_t W, int kernel_size,     \
                                int dilation, gfla_stream_t stream);
GFLA_DECL_RESAMPLE_FWD(f32, float)
GFLA_DECL_RESAMPLE_FWD(f64, double)
GFLA_DECL_RESAMPLE_FWD(bf16, uint16_t)
GFLA_DECL_RESAMPLE_FWD(f16, uint16_t)
#undef GFLA_DECL_RESAMPLE_FWD

#define GFLA_DECL_RESAMPLE_BWD(SFX, T)                                                             \
  int gfla_resample2d_bwd_##SFX(const T *in1, const T *in2, const T *grad_out, T *grad_in1,        \
                                T *grad_in2, int64_t B, int64_t C, int64_t Hi, int64_t Wi,         \
                                int64_t H, int64_t W, int kernel_size, int dilation,               \
                                int trunc_compat, gfla_stream_t stream);
GFLA_DECL_RESAMPLE_BWD(f32, float)
GFLA_DECL_RESAMPLE_BWD(f64, double)
#undef GFLA_DECL_RESAMPLE_BWD

/* ---- local-attention softmax + aggregate (fused) -------------------------------------------
 * Replaces, in ExtractorAttn.forward (base_function.py:804-810), the chain
 *   Softmax(dim=1) (:803) -> LocalAttnReshape (:808) -> attn * block_source -> avg_pool2d (:809)
 * together with the block_source extraction that feeds the product (:805), without ever
 * materialising the (B,C,kH,kW) product:
 *   out[b,c,y,x] = (1/k^2) * sum_{i,j} a[b,i*k+j,y,x] * bilinear(source[b,c], tap_ij(flow[b,:,y,x]))
 *   a = softmax over the k*k channel of `logits` if apply_softmax != 0, else `logits` as given
 *   (ExtractorAttn swaps the softmax for the plain nonlinearity when built with softmax=None,
 *   base_function.py:794).
 *   source (B,C,Hs,Ws)  flow (B,2,H,W)  logits (B,k*k,H,W)  out (B,C,H,W)
 *   attn_out (B,k*k,H,W) optional (NULL to skip): the post-softmax weights, i.e. what
 *   hook_attn_param returns as attn_param_ (base_function.py:815,818) and what backward needs.
 * backward: given grad_out (B,C,H,W) and the saved `attn` (post-softmax), produces
 *   grad_source (B,C,Hs,Ws; accumulated, must arrive zeroed), grad_flow (B,2,H,W; zeroed) and
 *   grad_logits (B,k*k,H,W; zeroed) -- the gradient w.r.t. the pre-softmax logits when
 *   apply_softmax != 0, else w.r.t. the weights.  Any of the three may be NULL.                 */
#define GFLA_DECL_AGGREGATE_FWD(SFX, T)                                                            \
  int gfla_local_attn_aggregate_fwd_##SFX(const T *source, const T *flow, const T *logits, T *out, \
                                          T *attn_out, int64_t B, int64_t C, int64_t Hs,           \
                                          int64_t Ws, int64_t H, int64_t W, int kernel_size,       \
                                          int apply_softmax, gfla_stream_t stream);
GFLA_DECL_AGGREGATE_FWD(f32, float)
GFLA_DECL_AGGREGATE_FWD(f64, double)
GFLA_DECL_AGGREGATE_FWD(bf16, uint16_t)
GFLA_DECL_AGGREGATE_FWD(f16, uint16_t)
#undef GFLA_DECL_AGGREGATE_FWD

/* Forward with scratch (f32 / bf16 / f16 storage): softmax, tap geometry and the (k+1)x(k+1) patch coefficients of every
 * flow pixel are computed ONCE (a table of (k+1)(k+2) floats + one word per pixel in `workspace`,
 * gfla_aggregate_fwd_workspace_bytes(B, H, W, k) bytes, 16-byte aligned) instead of once per channel group, and the
 * aggregation reads patch rows from LDS with paired 64-bit reads.  workspace == NULL, even k or Ws < k + 1: the
 * plain entry point's kernels.  Same results up to f32 summation order (the coefficient of a patch word is summed
 * over its taps before it meets the source value).                                                            */
int64_t gfla_aggregate_fwd_workspace_bytes(int64_t B, int64_t H, int64_t W, int kernel_size);
/* 1 when gfla_local_attn_aggregate_bwd_<storage> takes Hs x Ws source planes (elem_size 2 / 4 / 8 bytes); bf16 storage
 * is limited to planes that fit the LDS accumulators (round 4; replaces a constant duplicated on the host side) */
int gfla_aggregate_bwd_supported(int64_t Hs, int64_t Ws, int elem_size);
/* host-side launch geometry of that path (no GPU needed; tests): out[9] = channels per chunk, channels per range,
 * ranges, tile groups, threads, LDS row-pair pitch in words, tile width, tiles per sample, dynamic LDS bytes */
int gfla_aggregate_fwd_geometry(int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int kernel_size,
                                int64_t *out);
int gfla_local_attn_aggregate_fwd_ws_f32(const float *source, const float *flow, const float *logits, float *out,
                                         float *attn_out, void *workspace, int64_t B, int64_t C, int64_t Hs,
                                         int64_t Ws, int64_t H, int64_t W, int kernel_size, int apply_softmax,
                                         gfla_stream_t stream);
int gfla_local_attn_aggregate_fwd_ws_bf16(const uint16_t *source, const uint16_t *flow, const uint16_t *logits,
                                          uint16_t *out, uint16_t *attn_out, void *workspace, int64_t B, int64_t C,
                                          int64_t Hs, int64_t Ws, int64_t H, int64_t W, int kernel_size,
                                          int apply_softmax, gfla_stream_t stream);
int gfla_local_attn_aggregate_fwd_ws_f16(const uint16_t *source, const uint16_t *flow, const uint16_t *logits,
                                         uint16_t *out, uint16_t *attn_out, void *workspace, int64_t B, int64_t C,
                                         int64_t Hs, int64_t Ws, int64_t H, int64_t W, int kernel_size,
                                         int apply_softmax, gfla_stream_t stream);

#define GFLA_DECL_AGGREGATE_BWD(SFX, T)                                                            \
  int gfla_local_attn_aggregate_bwd_##SFX(const T *source, const T *flow, const T *attn,           \
                                          const T *grad_out, T *grad_source, T *grad_flow,         \
                                          T *grad_logits, int64_t B, int64_t C, int64_t Hs,        \
                                          int64_t Ws, int64_t H, int64_t W, int kernel_size,       \
                                          int apply_softmax, gfla_stream_t stream);
GFLA_DECL_AGGREGATE_BWD(f32, float)
GFLA_DECL_AGGREGATE_BWD(f64, double)
#undef GFLA_DECL_AGGREGATE_BWD


/* bf16 storage for the backward entry points (mixed-precision features): feature-map gradients (grad_source,
 * grad_in1) are bf16 and accumulated into like their f32 counterparts; every gradient that is a REDUCTION over channels
 * -- grad_flow (B,2,H,W), grad_logits (B,k*k,H,W), grad_in2 (B,3,H,W) -- is float32 (accumulated across workgroups with
 * float atomics; 8 mantissa bits would not survive C*k*k terms).  Planes must fit LDS (the attention-layer shapes do);
 * anything else returns GFLA_ERR_UNSUPPORTED.  Accumulation is f32 / f64-in-LDS exactly as in the f32 entry points. */
int gfla_block_extractor_bwd_bf16(const uint16_t *source, const uint16_t *flow, const uint16_t *grad_out,
                                  uint16_t *grad_source, float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws,
                                  int64_t Hf, int64_t Wf, int kernel_size, gfla_stream_t stream);
int gfla_block_extractor_unfold_bwd_bf16(const uint16_t *source, const uint16_t *flow, const uint16_t *grad_unfold,
                                         uint16_t *grad_source, float *grad_flow, int64_t B, int64_t C, int64_t Hs,
                                         int64_t Ws, int64_t Hf, int64_t Wf, int kernel_size, int layout,
                                         gfla_stream_t stream);
int gfla_local_attn_aggregate_bwd_bf16(const uint16_t *source, const uint16_t *flow, const uint16_t *attn,
                                       const uint16_t *grad_out, uint16_t *grad_source, float *grad_flow,
                                       float *grad_logits, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H,
                                       int64_t W, int kernel_size, int apply_softmax, gfla_stream_t stream);
int gfla_local_attn_source_bwd_bf16(const uint16_t *source, const uint16_t *flow, const uint16_t *grad_unfold,
                                    const uint16_t *attn, const uint16_t *grad_out, uint16_t *grad_source,
                                    float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H,
                                    int64_t W, int kernel_size, int layout, gfla_stream_t stream);
int gfla_resample2d_bwd_bf16(const uint16_t *in1, const uint16_t *in2, const uint16_t *grad_out, uint16_t *grad_in1,
                             float *grad_in2, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W,
                             int kernel_size, int dilation, int trunc_compat, gfla_stream_t stream);

/* f16 storage for the same backward entry points: the bf16 signatures and rules, IEEE binary16 feature maps. */
#define GFLA_DECL_BWD16(SFX, T)                                                                                        \
  int gfla_block_extractor_bwd_##SFX(const T *source, const T *flow, const T *grad_out, T *grad_source, float *grad_flow, \
                                     int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf, int64_t Wf,               \
                                     int kernel_size, gfla_stream_t stream);                                             \
  int gfla_block_extractor_unfold_bwd_##SFX(const T *source, const T *flow, const T *grad_unfold, T *grad_source,        \
                                            float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t Hf,  \
                                            int64_t Wf, int kernel_size, int layout, gfla_stream_t stream);              \
  int gfla_local_attn_aggregate_bwd_##SFX(const T *source, const T *flow, const T *attn, const T *grad_out,             \
                                          T *grad_source, float *grad_flow, float *grad_logits, int64_t B, int64_t C,    \
                                          int64_t Hs, int64_t Ws, int64_t H, int64_t W, int kernel_size,                 \
                                          int apply_softmax, gfla_stream_t stream);                                      \
  int gfla_local_attn_source_bwd_##SFX(const T *source, const T *flow, const T *grad_unfold, const T *attn,             \
                                       const T *grad_out, T *grad_source, float *grad_flow, int64_t B, int64_t C,        \
                                       int64_t Hs, int64_t Ws, int64_t H, int64_t W, int kernel_size, int layout,        \
                                       gfla_stream_t stream);                                                            \
  int gfla_resample2d_bwd_##SFX(const T *in1, const T *in2, const T *grad_out, T *grad_in1, float *grad_in2, int64_t B, \
                                int64_t C, int64_t Hi, int64_t Wi, int64_t H, int64_t W, int kernel_size, int dilation,  \
                                int trunc_compat, gfla_stream_t stream);
GFLA_DECL_BWD16(f16, uint16_t)
#undef GFLA_DECL_BWD16

/* ---- scatters as block-sparse products on the matrix cores (csrc/patch_mfma.hip) -----------------------------
 * The two backward passes that scatter into a feature plane -- the aggregation's d/d source and resample2d's
 * d/d input1 (resample2d_kernel.cu:98-202; replaces its atomicAdd scatter) -- spread each flow pixel's gradient over
 * a dense patch with channel-independent weights: a sparse x dense product.  The *_ws entry points take scratch for
 * the per-pixel patch table (gfla_scatter_workspace_bytes(B, H, W, entries): entries = (k+1)^2 for the aggregation,
 * k*k for resample2d; 256-byte aligned; may be NULL = the LDS-atomic kernels of the plain entry points) and multiply
 * the tiled sparse matrix on v_mfma_f32_32x32x2_f32 with output-stationary accumulators: no atomics, fixed summation
 * order.  With a workspace the aggregation's d/d flow comes out of the d/d logits pass.  Same accumulate-into
 * contract as the plain entry points; unsupported shapes (plane rows wider than 192, dilation != 1) fall back.   */
int64_t gfla_scatter_workspace_bytes(int64_t B, int64_t H, int64_t W, int patch_entries);
int gfla_local_attn_aggregate_bwd_ws_f32(const float *source, const float *flow, const float *attn,
                                         const float *grad_out, float *grad_source, float *grad_flow,
                                         float *grad_logits, void *workspace, int64_t B, int64_t C, int64_t Hs,
                                         int64_t Ws, int64_t H, int64_t W, int kernel_size, int apply_softmax,
                                         gfla_stream_t stream);
int gfla_resample2d_bwd_ws_f32(const float *in1, const float *in2, const float *grad_out, float *grad_in1,
                               float *grad_in2, void *workspace, int64_t B, int64_t C, int64_t Hi, int64_t Wi,
                               int64_t H, int64_t W, int kernel_size, int dilation, int trunc_compat,
                               gfla_stream_t stream);

/* ---- everything in ExtractorAttn that flows back into block_source(source, flow), in ONE pass ----------
 * block_source receives two gradient streams (base_function.py:805-809): through the first FC layer
 * (grad_unfold, in the unfold layout above; may be NULL) and through the attention-weighted aggregation
 * (attn (B,k*k,H,W) post-softmax and grad_out (B,C,H,W): attn[b,ij,p]*grad_out[b,c,p]/k^2, never
 * materialised; both may be NULL together).  Their sum is scattered into grad_source / grad_flow
 * (accumulated; pass zeroed buffers; either may be NULL).  The reference runs the block_extractor
 * backward kernel twice for this (once per stream, plus the reshape/multiply/avg-pool backward).      */
#define GFLA_DECL_SOURCE_BWD(SFX, T)                                                               \
  int gfla_local_attn_source_bwd_##SFX(const T *source, const T *flow, const T *grad_unfold,       \
                                       const T *attn, const T *grad_out, T *grad_source,           \
                                       T *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, \
                                       int64_t H, int64_t W, int kernel_size, int layout,          \
                                       gfla_stream_t stream);
GFLA_DECL_SOURCE_BWD(f32, float)
GFLA_DECL_SOURCE_BWD(f64, double)
#undef GFLA_DECL_SOURCE_BWD

/* ---- tail of ExtractorAttn's fully_connect_layer: nonlinearity + 1x1 convolution (base_function.py:799-803)
 *   logits[b,q,p] = b1[q] + sum_o w1[q,o] * lrelu(hs[b,o,p] + ht[b,o,p] + b0[o], slope)
 * hs: the source half of the first FC convolution, addressed as hs[b*hs_sb + o*hs_so + p] (so both the
 * GEMM's (Hc,B,HW) and the plain (B,Hc,HW) layout are accepted); ht: the target half, (B,Hc,HW) contiguous;
 * b0 (Hc) and b1 (KK) may be NULL; w1 (KK,Hc); logits (B,KK,HW) is overwritten.  KK in {1,4,9,16,25};
 * slope = 0 gives ReLU.  backward: given g_logits (B,KK,HW) overwrites g_hs (hs's addressing), g_ht
 * (B,Hc,HW; may be NULL) with the gradient w.r.t. hs/ht (identical values, two layouts) and act (B,Hc,HW;
 * may be NULL) with the activations (for dW1 = sum_b g_logits_b act_b^T, left to the caller's GEMM) and
 * bias_partials (B * ceil(HW / 64), Hc + KK; may be NULL) with one row per workgroup: its sums of the
 * hidden gradient (-> d b0) followed by its sums of g_logits (-> d b1); the caller adds the rows up.    */
#define GFLA_DECL_FC_TAIL(SFX, T)                                                                    \
  int gfla_fc_tail_fwd_##SFX(const T *hs, int64_t hs_sb, int64_t hs_so, const T *ht, const T *b0,   \
                             const T *w1, const T *b1, T *logits, int64_t B, int64_t Hc, int64_t HW, \
                             int KK, double slope, gfla_stream_t stream);                           \
  int gfla_fc_tail_bwd_##SFX(const T *hs, int64_t hs_sb, int64_t hs_so, const T *ht, const T *b0,   \
                             const T *w1, const T *g_logits, T *g_hs, T *g_ht, T *act,              \
                             T *bias_partials, int64_t B, int64_t Hc, int64_t HW, int KK,           \
                             double slope, gfla_stream_t stream);
GFLA_DECL_FC_TAIL(f32, float)
GFLA_DECL_FC_TAIL(f64, double)
#undef GFLA_DECL_FC_TAIL

/* ---- first FC layer of ExtractorAttn on the matrix cores (csrc/fc_gemm.hip, fc_sample.hip, fc_block.hip) -----
 * Replaces, in ExtractorAttn.forward (model/networks/base_function.py:799-807),
 *   block_source = extractor(source, flow); block_target = extractor(target, 0)
 *   logits = Conv2d(128, k*k, 1)(nonlinearity(Conv2d(2C, 128, k, stride k)(cat(block_target, block_source))))
 * i.e. the two BlockExtractor launches, the cat and both convolutions of fully_connect_layer (its softmax stays
 * with gfla_local_attn_aggregate_*).  Neither block tensor is built:  FC0(source half) = bilinear sample, at
 * p + flow(p), of conv_kxk(replicate-extended source, W[:, C:]) -- exact, because all k*k taps of a position share
 * one fractional offset -- and FC0(target half) = conv_kxk(replicate-padded target, W[:, :C]); the convolutions
 * are implicit GEMMs on MFMA, hand-written for gfx950.
 *   source, target (B,C,H,W)  flow (B,2,H,W)  w0 = conv0.weight (128, 2C, k, k)  b0 (128) or NULL
 *   w1 = conv1.weight (k*k, 128)  b1 (k*k) or NULL  logits (B,k*k,H,W), overwritten.  fp32; k in {3, 5}.
 *   slope: LeakyReLU negative slope (0 = ReLU).
 *   mode: arithmetic of the contraction -- 4: float32 throughout in the Winograd domain (F(2x2,5x5) / F(4x4,3x3) on the
 *   points {0, 1, -1, 2, -1/2, inf}: 36 multiplies per 6x6 tile instead of 100 / 144, v_mfma_f32_16x16x4_f32; the
 *   host-side default, csrc/fc_wino.hip); 0: v_mfma_f32_32x32x2_f32, direct convolution (a k-ordered f32 fma chain per
 *   output); 3: operands as three f16 terms, six cross products, f32 accumulate (every product term above 2^-32 kept:
 *   f32-grade); 2: two f16 terms, three products (2^-21 per product); 1: one f16 term (exact for bf16 values).
 *   workspace: gfla_fc_workspace_bytes(..., which = 0) bytes, 256-byte aligned; forward fills it and backward
 *   reads it (packed inputs, convolved source map, hidden activations).  scratch: (..., which = 1) bytes.
 * backward: given grad_logits, overwrites whichever of grad_source, grad_target (B,C,H,W), grad_flow (B,2,H,W),
 *   grad_w0, grad_b0, grad_w1, grad_b1 is not NULL (no buffer needs zeroing).  flags: GFLA_FC_ACCUMULATE_SOURCE /
 *   GFLA_FC_ACCUMULATE_FLOW add into grad_source / grad_flow instead (they then hold the gradient another path of the
 *   same block already produced, e.g. the aggregation's).
 * gfla_fc_supported(C, H, W, k, mode): 1 if the shape is handled (the convolution's input tile must fit LDS).  */
#define GFLA_FC_ACCUMULATE_SOURCE 1
#define GFLA_FC_ACCUMULATE_FLOW 2
int gfla_fc_supported(int64_t C, int64_t H, int64_t W, int kernel_size, int mode);
int64_t gfla_fc_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int kernel_size, int mode,
                                int which);
int gfla_fc_forward_f32(const float *source, const float *target, const float *flow, const float *w0,
                        const float *b0, const float *w1, const float *b1, void *workspace, float *logits,
                        int64_t B, int64_t C, int64_t H, int64_t W, int kernel_size, double slope, int mode,
                        gfla_stream_t stream);
int gfla_fc_backward_f32(void *workspace, const float *flow, const float *w1, const float *grad_logits,
                         void *scratch, float *grad_source, float *grad_target, float *grad_flow, float *grad_w0,
                         float *grad_b0, float *grad_w1, float *grad_b1, int64_t B, int64_t C, int64_t H,
                         int64_t W, int kernel_size, double slope, int mode, int flags, gfla_stream_t stream);
/* float16 FEATURES: the forward of arithmetic mode 1 with the activation records packed straight from the f16 maps (an f16
 * value IS one f16 term: written unscaled, no max |x| pass over the features, no float32 copy of source or target).
 * source, target (B,C,H,W) f16; flow (B,2,H,W) float32 (the sampling tail and the backward read it in float32); w0, b0,
 * w1, b1, logits float32.  The workspace is mode 1's (gfla_fc_workspace_bytes(..., 1, 0)) and gfla_fc_backward_f32(...,
 * mode = 1, ...) takes it as it stands.  Dispatch trace: GFLA_PATH_FC_FWD_MODE1 and GFLA_PATH_FC_PACK_F16. */
int gfla_fc_forward_f16(const uint16_t *source, const uint16_t *target, const float *flow, const float *w0,
                        const float *b0, const float *w1, const float *b1, void *workspace, float *logits,
                        int64_t B, int64_t C, int64_t H, int64_t W, int kernel_size, double slope, gfla_stream_t stream);
/* Pieces of the above for the parity tests.  gfla_fc_geometry: out[0..12] = Hp, Wp, Ho, Wo, pad_top, pad_left, M,
 * Md, lead, Sx, Sz, Mg, Mdg of one half (is_source: the source half is extended by k-1, the target half padded by
 * k/2).  gfla_fc_conv_fwd: out (B, Mg, 128) = the convolved map of one half, row yo*Wo + xo.  gfla_fc_conv_bwd:
 * from z (B, Sz, 128), the gradient of that map in "Z layout" (row lead + yo*Wp + xo, zero elsewhere), grad_x
 * (B,C,H,W) and grad_w0 (128,2C,k,k; the other half zero); needs the workspace of gfla_fc_conv_fwd.
 * gfla_fc_tr_probe: raw result of ds_read_b64_tr_b16 for an LDS image and 64 per-lane byte offsets.            */
int gfla_fc_geometry(int64_t H, int64_t W, int kernel_size, int is_source, int64_t *out);
int gfla_fc_conv_fwd_f32(const float *x, const float *w0, int is_source, void *workspace, float *out, int64_t B,
                         int64_t C, int64_t H, int64_t W, int kernel_size, int mode, gfla_stream_t stream);
int gfla_fc_conv_bwd_f32(const float *z, int is_source, void *workspace, void *scratch, float *grad_x,
                         float *grad_w0, int64_t B, int64_t C, int64_t H, int64_t W, int kernel_size, int mode,
                         gfla_stream_t stream);
/* gfla_fc_kernel: ONE internal kernel of the path on the state a forward + backward of the same shape left in
 * workspace / scratch, for per-kernel timing (bench.py, profiles).  which: 0 / 1 convolution forward of the source /
 * target half, 2 / 3 data-gradient convolution, 4 / 5 weight gradient; modes 4 / 5 only: 6 / 7 = the forward / data-gradient
 * convolutions of both halves in ONE launch, 8 = both Winograd-domain weight gradients in one launch, the way
 * gfla_fc_forward / gfla_fc_backward issue them.                                                                  */
int gfla_fc_kernel_f32(int which, void *workspace, void *scratch, int64_t B, int64_t C, int64_t H, int64_t W,
                       int kernel_size, int mode, gfla_stream_t stream);
int gfla_fc_tr_probe(const int16_t *image, int n_halves, const int32_t *offsets, int16_t *out,
                     gfla_stream_t stream);
/* tools only: a device buffer (workgroups x 8 waves x 6 uint64) that the timing instantiation of the Winograd
 * convolution kernel (arithmetic mode 4, tuning key 20 = 16) fills with per-wave phase times in shader cycles;
 * NULL switches it off.                                                                                          */
int gfla_fc_wino_debug_buffer(void *buffer);

/* ---- gradient of the replicate padding in front of the target half of ExtractorAttn's first FC layer ---
 * block_target = extractor(target, zero flow) (base_function.py:806) is the replicate-padded unfold of
 * target; its half of the FC layer runs as a stride-1 convolution of the padded target.  Given the gradient
 * w.r.t. the padded tensor (planes, H+top+bottom, W+left+right), overwrites grad_in (planes, H, W): border
 * strips are folded onto the edge pixels (a gather, no atomics).                                          */
int gfla_replicate_pad_bwd_f32(const float *grad_padded, float *grad_in, int64_t planes, int64_t H,
                               int64_t W, int pad_left, int pad_right, int pad_top, int pad_bottom,
                               gfla_stream_t stream);
int gfla_replicate_pad_bwd_f64(const double *grad_padded, double *grad_in, int64_t planes, int64_t H,
                               int64_t W, int pad_left, int pad_right, int pad_top, int pad_bottom,
                               gfla_stream_t stream);

/* ---- float64 GEMM on the FP64 matrix cores (csrc/gemm_f64.hip): ExtractorAttn's FC layers in float64 -----------
 *   C[m,n] = beta*C[m,n] + sum_k A[m,k] * B[k,n],   beta 0 or 1 (beta 0 never reads C).
 * Each operand is a strided VIEW given by 12 int64 (host memory, read during the call):
 *   {row d0, d1, d2, s0, s1, s2,  col d0, d1, d2, s0, s1, s2}
 * the logical row index r = (r0*d1 + r1)*d2 + r2 sits at element offset r0*s0 + r1*s1 + r2*s2 from the operand's
 * pointer (likewise the column), so d0*d1*d2 must equal the extent (M / K for A, K / N for B, M / N for C); every
 * d >= 1.  C must not overlap A or B, and distinct (row, col) of C must be distinct elements.
 * split_k: 0 auto, 1 off, s > 1 about s slices of K (each a multiple of 16 long) summed in a fixed order by a second
 * pass: results are bit-identical from run to run.  workspace: gfla_gemm_f64_workspace_bytes(M, N, K, split_k) bytes
 * (may be 0: then NULL is fine), 8-byte aligned; -1 for negative arguments.
 * NULL -> -1; negative extents, beta other than 0 / 1, a view that does not tile its extent -> -2; extents beyond
 * 2^31 -> -3. */
int64_t gfla_gemm_f64_workspace_bytes(int64_t M, int64_t N, int64_t K, int split_k);
int gfla_gemm_f64(double *c, const int64_t *c_view, const double *a, const int64_t *a_view, const double *b,
                  const int64_t *b_view, int64_t M, int64_t N, int64_t K, int beta, int split_k, void *workspace,
                  gfla_stream_t stream);

/* ---- best-match cosine similarity of the sampling-correctness loss ----------------
 * Replaces, in PerceptualCorrectness.calculate_loss (external_function.py:255-268),
 *   source_norm = source / (||source||_c + eps); target_norm = target / (||target||_c + eps)
 *   correction = bmm(source_norm^T, target_norm)          [B, Ns, Nt], materialised by the reference
 *   correction_max, max_indices = max(correction, dim=1)
 * source (B,C,Ns), target (B,C,Nt): contiguous views of the NCHW feature maps.  out_max (B,Nt) and
 * out_idx (B,Nt; int32 row of the maximum, may be NULL) are fully overwritten.  `workspace` is caller-
 * provided scratch of gfla_max_cosine_workspace_bytes(B, Ns, Nt) bytes, 16-byte aligned (the inverse
 * norms and the packed running maxima live there).  fp32 only (exact-f32 MFMA); the [Ns,Nt] matrix is
 * never written.  Non-finite features behave as in the reference: a position with a NaN or an inf among its channels
 * normalises to NaN, every similarity it takes part in is NaN, and such a column's out_max is NaN with out_idx the row of
 * its first NaN, as torch.max(dim=1) returns it.  out_idx is in [0, Ns) for every input.
 * Ties: where several source rows share a column's maximum, out_idx is the LOWEST such row -- whatever the split of the
 * source range (tuning key 5), the staging path and the storage type (the per-lane scan takes a later row only if it is
 * strictly greater; the lane, wave and unit merges prefer the lower row on equal values).  A zero target vector gives
 * (0.0, row 0).  tests/test_loss_exact_gpu.py holds all three entry points to this on inputs full of exact ties. */
int64_t gfla_max_cosine_workspace_bytes(int64_t B, int64_t Ns, int64_t Nt);
int gfla_max_cosine_fwd_f32(const float *source, const float *target, void *workspace, float *out_max,
                            int32_t *out_idx, int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps,
                            gfla_stream_t stream);
/* The same on 16-bit storage (float16 / bfloat16 bit patterns), source and target of one type: v_mfma_f32_32x32x16_f16 /
 * _bf16 with float32 accumulators.  A product of two 16-bit values is exact in float32, so the result is that of the
 * float32 entry on the up-cast inputs up to the order of the float32 sums.  The target tile of a unit stays in the LDS
 * and the source streams past it; no float32 or transposed copy of either map is made.  out_max float32, out_idx
 * int32, eps, NaN handling and the workspace (gfla_max_cosine_workspace_bytes) as above. */
int gfla_max_cosine_fwd_f16(const uint16_t *source, const uint16_t *target, void *workspace, float *out_max,
                            int32_t *out_idx, int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps,
                            gfla_stream_t stream);
int gfla_max_cosine_fwd_bf16(const uint16_t *source, const uint16_t *target, void *workspace, float *out_max,
                             int32_t *out_idx, int64_t B, int64_t C, int64_t Ns, int64_t Nt, double eps,
                             gfla_stream_t stream);

/* ---- per-position map of the sampling-correctness loss (external_function.py:275-276) -----------------
 *   loss_map[b,n] = exp(-cosine_similarity(warped[b,:,n], target[b,:,n]) / (best[b,n] + eps))
 * warped, target (B,C,N) contiguous; best (B,N) = gfla_max_cosine_fwd's out_max; eps_cos = the eps of
 * F.cosine_similarity (1e-8), eps = the loss's own (1e-8).  forward overwrites loss_map (B,N) and
 * stats (B,N,3) = (cos, |warped|, |target|), which backward reads back.  backward overwrites any of
 * grad_warped (B,C,N), grad_target (B,C,N), grad_best (B,N) that is not NULL, given grad_map (B,N).    */
int gfla_correctness_map_fwd_f32(const float *warped, const float *target, const float *best,
                                 float *loss_map, float *stats, int64_t B, int64_t C, int64_t N,
                                 double eps_cos, double eps, gfla_stream_t stream);
int gfla_correctness_map_bwd_f32(const float *warped, const float *target, const float *best,
                                 const float *stats, const float *loss_map, const float *grad_map,
                                 float *grad_warped, float *grad_target, float *grad_best, int64_t B,
                                 int64_t C, int64_t N, double eps_cos, double eps, gfla_stream_t stream);
/* 16-bit target map (float16 / bfloat16 storage), float32 warped map: the target is read as stored, never up-cast.
 * best, loss_map, stats, grad_map, grad_best and grad_warped stay float32; grad_target is written in the storage type
 * (float32 arithmetic, one rounding at the store). */
int gfla_correctness_map_fwd_f16(const float *warped, const uint16_t *target, const float *best,
                                 float *loss_map, float *stats, int64_t B, int64_t C, int64_t N,
                                 double eps_cos, double eps, gfla_stream_t stream);
int gfla_correctness_map_bwd_f16(const float *warped, const uint16_t *target, const float *best,
                                 const float *stats, const float *loss_map, const float *grad_map,
                                 float *grad_warped, uint16_t *grad_target, float *grad_best, int64_t B,
                                 int64_t C, int64_t N, double eps_cos, double eps, gfla_stream_t stream);
int gfla_correctness_map_fwd_bf16(const float *warped, const uint16_t *target, const float *best,
                                 float *loss_map, float *stats, int64_t B, int64_t C, int64_t N,
                                 double eps_cos, double eps, gfla_stream_t stream);
int gfla_correctness_map_bwd_bf16(const float *warped, const uint16_t *target, const float *best,
                                 const float *stats, const float *loss_map, const float *grad_map,
                                 float *grad_warped, uint16_t *grad_target, float *grad_best, int64_t B,
                                 int64_t C, int64_t N, double eps_cos, double eps, gfla_stream_t stream);

/* Storage-type conversion of up to four contiguous tensors in one launch (unused jobs: n = 0).  to_bf16 = 0: bfloat16 ->
 * float32 (exact); 1: float32 -> bfloat16, round to nearest even.  The bf16 feature path of ExtractorAttn widens three
 * operands and narrows three gradients per call; at the face model's batch every one of them was a launch of its own. */
int gfla_convert_multi(const void *src0, void *dst0, int64_t n0, const void *src1, void *dst1, int64_t n1, const void *src2,
                       void *dst2, int64_t n2, const void *src3, void *dst3, int64_t n3, int to_bf16, gfla_stream_t stream);
/* to_bf16 (the flag word above) also takes GFLA_CONVERT_F16_TO_F32 (float16 -> float32, exact) and GFLA_CONVERT_F32_TO_F16
 * (float32 -> float16, round to nearest even, overflow to +-inf, subnormals kept).  0 and 1 keep their meaning. */
#define GFLA_CONVERT_F16_TO_F32 2
#define GFLA_CONVERT_F32_TO_F16 3

/* ---- mask blend of the face model's attention pair (generator.py:496-499; csrc/mask_blend.hip, round 4) ----
 *   y = (out*(1-mask_p) + attn_p*mask_p) + (out*(1-mask_r) + attn_r*mask_r)
 * out, attn_p, attn_r, y: (B,C,HW) contiguous; mask_p, mask_r: (B,1,HW).  Forward: the op-by-op result bit for bit (every
 * intermediate rounded to the storage type).  Backward: any gradient pointer may be NULL; g_mask_p / g_mask_r are FLOAT32
 * (B,1,HW), ACCUMULATED into (pass zeroed buffers) whatever the storage type. */
int gfla_mask_blend_fwd_f32(const float *out, const float *attn_p, const float *attn_r, const float *mask_p,
                            const float *mask_r, float *y, int64_t B, int64_t C, int64_t HW, gfla_stream_t stream);
int gfla_mask_blend_fwd_bf16(const uint16_t *out, const uint16_t *attn_p, const uint16_t *attn_r, const uint16_t *mask_p,
                             const uint16_t *mask_r, uint16_t *y, int64_t B, int64_t C, int64_t HW, gfla_stream_t stream);
int gfla_mask_blend_bwd_f32(const float *out, const float *attn_p, const float *attn_r, const float *mask_p,
                            const float *mask_r, const float *grad_y, float *g_out, float *g_attn_p, float *g_attn_r,
                            float *g_mask_p, float *g_mask_r, int64_t B, int64_t C, int64_t HW, gfla_stream_t stream);
int gfla_mask_blend_bwd_bf16(const uint16_t *out, const uint16_t *attn_p, const uint16_t *attn_r, const uint16_t *mask_p,
                             const uint16_t *mask_r, const uint16_t *grad_y, uint16_t *g_out, uint16_t *g_attn_p,
                             uint16_t *g_attn_r, float *g_mask_p, float *g_mask_r, int64_t B, int64_t C, int64_t HW,
                             gfla_stream_t stream);
int gfla_mask_blend_fwd_f16(const uint16_t *out, const uint16_t *attn_p, const uint16_t *attn_r, const uint16_t *mask_p,
                            const uint16_t *mask_r, uint16_t *y, int64_t B, int64_t C, int64_t HW, gfla_stream_t stream);
int gfla_mask_blend_bwd_f16(const uint16_t *out, const uint16_t *attn_p, const uint16_t *attn_r, const uint16_t *mask_p,
                            const uint16_t *mask_r, const uint16_t *grad_y, uint16_t *g_out, uint16_t *g_attn_p,
                            uint16_t *g_attn_r, float *g_mask_p, float *g_mask_r, int64_t B, int64_t C, int64_t HW,
                            gfla_stream_t stream);

/* ---- affine regularisation loss of a flow field (external_function.py:31-77; csrc/affine_reg.hip) ----------------------
 *   loss = 1/(B L) sum over b, the two axes and the L = (H-k+1)(W-k+1) valid k x k windows of |f - P f|^2
 * f = the flow patch of one axis, P f = the least-squares plane through it.  This is the reference's u^T M u on the
 * sampling grid u = flow + coordinates (M = I - P annihilates the coordinates), evaluated without the grid.
 * flow (B,2,H,W) contiguous, read in its storage type (widened exactly at the load); the differences inside a window, the
 * plane fit and every sum after it are float64 for every storage type (float32 loses the gradient of a nearly affine
 * flow: csrc/affine_reg.hip), so a 16- or 32-bit result is rounded once, at its store.  `loss`: ONE device scalar, float32 (float64 for _f64), = loss_x + loss_y as the reference returns it.
 * `grad_loss`: one DEVICE scalar of the loss's type (d/d loss from upstream, a GradScaler's scale included; no host
 * sync); grad_flow (B,2,H,W) in the flow's storage type, fully overwritten, rounded once at the store.
 * `workspace`: gfla_affine_reg_workspace_bytes(B, H, W, k) bytes, 8-byte aligned, uninitialised: forward keeps its
 * per-workgroup partial sums there.  Backward re-fits the windows from `flow` and does not read it (it may be NULL).
 * No atomics: partial sums are reduced in a fixed order, loss and gradient are bit-identical from call to call.
 * NULL -> -1; non-positive sizes, H < k or W < k -> -2; k outside 2..7 -> GFLA_ERR_UNSUPPORTED (k = 1 has no projector:
 * A^T A is singular), as are H or W > 16384 and B > 32767.  gfla_affine_reg_workspace_bytes returns the same codes.
 * Additive: GFLA_ABI_VERSION stays 8. */
int64_t gfla_affine_reg_workspace_bytes(int64_t B, int64_t H, int64_t W, int k);
int gfla_affine_reg_fwd_f32(const float *flow, void *workspace, float *loss, int64_t B, int64_t H, int64_t W, int k,
                            gfla_stream_t stream);
int gfla_affine_reg_fwd_f64(const double *flow, void *workspace, double *loss, int64_t B, int64_t H, int64_t W, int k,
                            gfla_stream_t stream);
int gfla_affine_reg_fwd_f16(const uint16_t *flow, void *workspace, float *loss, int64_t B, int64_t H, int64_t W, int k,
                            gfla_stream_t stream);
int gfla_affine_reg_fwd_bf16(const uint16_t *flow, void *workspace, float *loss, int64_t B, int64_t H, int64_t W, int k,
                             gfla_stream_t stream);
int gfla_affine_reg_bwd_f32(const float *flow, const float *grad_loss, void *workspace, float *grad_flow, int64_t B,
                            int64_t H, int64_t W, int k, gfla_stream_t stream);
int gfla_affine_reg_bwd_f64(const double *flow, const double *grad_loss, void *workspace, double *grad_flow, int64_t B,
                            int64_t H, int64_t W, int k, gfla_stream_t stream);
int gfla_affine_reg_bwd_f16(const uint16_t *flow, const float *grad_loss, void *workspace, uint16_t *grad_flow, int64_t B,
                            int64_t H, int64_t W, int k, gfla_stream_t stream);
int gfla_affine_reg_bwd_bf16(const uint16_t *flow, const float *grad_loss, void *workspace, uint16_t *grad_flow, int64_t B,
                             int64_t H, int64_t W, int k, gfla_stream_t stream);

/* ---- style term of VGGLoss: L1 distance of two Gram matrices (external_function.py:121-160; csrc/gram_l1.hip) ---------
 *   F = x viewed as (B,C,N), N = H W;   G(x) = F F^T / (N C);   D = G(x) - G(y);   loss = mean |D| over the B C^2 entries
 * x, y (B,C,N) contiguous, one storage type, read as stored: float16 / bfloat16 products are exact in the float32
 * accumulators of the matrix cores, G(x) and G(y) are summed separately and in the same order (x == y gives D = 0 and
 * loss = 0 exactly), scaled and subtracted in float32.  `diff`: D (B,C,C) float32, fully overwritten, symmetric bit for
 * bit.  `loss`: ONE device scalar, float32.  `workspace`: gfla_gram_l1_workspace_bytes(B, C, N) bytes, 16-byte aligned,
 * uninitialised (partial tiles of the chunks N is split into, and the per-workgroup sums of |D|).
 * Backward: grad_feat = (negate ? -1 : +1) grad_loss 2 / (B C^3 N) sign(D) feat, in feat's storage type, fully
 * overwritten, rounded once at the store; negate = 0 for d/dx (feat = x), 1 for d/dy (feat = y).  `grad_loss`: one DEVICE
 * float32 scalar (no host sync).  sign(D) is exact in every storage type.
 * No atomics: loss, D and gradients are bit-identical from call to call.  Any B, C, N >= 1 (ragged C and N are
 * zero-filled); NULL -> -1; non-positive sizes -> -2; B > 16384, C > 4096 or N > 2^24 -> GFLA_ERR_UNSUPPORTED, nothing is
 * launched.  gfla_gram_l1_workspace_bytes returns the same codes.  Additive: GFLA_ABI_VERSION stays 8. */
int64_t gfla_gram_l1_workspace_bytes(int64_t B, int64_t C, int64_t N);
int gfla_gram_l1_fwd_f32(const float *x, const float *y, void *workspace, float *diff, float *loss, int64_t B, int64_t C,
                         int64_t N, gfla_stream_t stream);
int gfla_gram_l1_fwd_f16(const uint16_t *x, const uint16_t *y, void *workspace, float *diff, float *loss, int64_t B,
                         int64_t C, int64_t N, gfla_stream_t stream);
int gfla_gram_l1_fwd_bf16(const uint16_t *x, const uint16_t *y, void *workspace, float *diff, float *loss, int64_t B,
                          int64_t C, int64_t N, gfla_stream_t stream);
int gfla_gram_l1_bwd_f32(const float *feat, const float *diff, const float *grad_loss, float *grad_feat, int64_t B,
                         int64_t C, int64_t N, int negate, gfla_stream_t stream);
int gfla_gram_l1_bwd_f16(const uint16_t *feat, const float *diff, const float *grad_loss, uint16_t *grad_feat, int64_t B,
                         int64_t C, int64_t N, int negate, gfla_stream_t stream);
int gfla_gram_l1_bwd_bf16(const uint16_t *feat, const float *diff, const float *grad_loss, uint16_t *grad_feat, int64_t B,
                          int64_t C, int64_t N, int negate, gfla_stream_t stream);

/* ---- bilinear flow warp (external_function.py:309-319, base_function.py:490-506, poseflownet_model.py:86-103;
 * csrc/flow_warp.hip) --------------------------------------------------------------------------------------------------
 *   out[b,c,y,x] = bilinear(source[b,c], ix, iy),   ix = (x + gx flow_x) mx,   iy = (y + gy flow_y) my   (source pixels)
 * with zero padding: a corner outside the map contributes 0 -- grid_sample(bilinear, zeros, align_corners=True) without
 * the normalised grid.  The four scalars select the reference's convention (csrc/flow_warp.hip lists the three).
 * source (B,C,Hs,Ws) contiguous, read in its storage type; flow (B,2,H,W), out (B,C,H,W) and grad_out float32 (float64
 * for _f64).  Position, weights and interpolation run in the flow's precision; out is rounded once, at the store.
 * Backward: either output may be NULL.  grad_flow (B,2,H,W), fully overwritten: one writer per element, the sum over
 * channels in a fixed order inside the workgroup (float64), no atomics, bit-identical from call to call.  grad_source
 * (B,C,Hs,Ws) in the FLOW's precision (float32 for 16-bit sources: the caller rounds it to the storage type once): the
 * entry point zero-fills it itself and accumulates with float atomics -- the one output that is not bit-reproducible.
 * NULL -> -1; non-positive sizes -> -2; Hs Ws, H W or the number of workgroups (B ceil(H W / 64) ceil(C / 32)) beyond
 * 2^31 - 1 -> GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive: GFLA_ABI_VERSION stays 8. */
int gfla_flow_warp_fwd_f32(const float *source, const float *flow, float *out, int64_t B, int64_t C, int64_t Hs, int64_t Ws,
                           int64_t H, int64_t W, double gx, double gy, double mx, double my, gfla_stream_t stream);
int gfla_flow_warp_fwd_f64(const double *source, const double *flow, double *out, int64_t B, int64_t C, int64_t Hs,
                           int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                           gfla_stream_t stream);
int gfla_flow_warp_fwd_f16(const uint16_t *source, const float *flow, float *out, int64_t B, int64_t C, int64_t Hs,
                           int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                           gfla_stream_t stream);
int gfla_flow_warp_fwd_bf16(const uint16_t *source, const float *flow, float *out, int64_t B, int64_t C, int64_t Hs,
                            int64_t Ws, int64_t H, int64_t W, double gx, double gy, double mx, double my,
                            gfla_stream_t stream);
int gfla_flow_warp_bwd_f32(const float *source, const float *flow, const float *grad_out, float *grad_source,
                           float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                           double gy, double mx, double my, gfla_stream_t stream);
int gfla_flow_warp_bwd_f64(const double *source, const double *flow, const double *grad_out, double *grad_source,
                           double *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                           double gy, double mx, double my, gfla_stream_t stream);
int gfla_flow_warp_bwd_f16(const uint16_t *source, const float *flow, const float *grad_out, float *grad_source,
                           float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                           double gy, double mx, double my, gfla_stream_t stream);
int gfla_flow_warp_bwd_bf16(const uint16_t *source, const float *flow, const float *grad_out, float *grad_source,
                            float *grad_flow, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, double gx,
                            double gy, double mx, double my, gfla_stream_t stream);

/* ---- VGG19 feature extractor (external_function.py:323-444): 3x3 convolution + bias + ReLU and 2x2 max pooling --------
 * (csrc/conv3x3.hip, csrc/maxpool2x2.hip).  T: the storage type of the activations, float32 / float16 / bfloat16; sums are
 * float32 on the matrix cores (v_mfma_f32_32x32x2_f32 / 32x32x16_f16 / 32x32x16_bf16), 16-bit results are rounded to
 * nearest even once.  Stride 1, zero padding 1, NCHW contiguous, any B, Cin, Cout, H, W >= 1.
 *   fwd:       y (B,Cout,H,W) = max(0, conv3x3(x (B,Cin,H,W), w) + bias); bias: Cout float32 values.
 *   bwd_data:  grad_x (B,Cin,H,W) = conv3x3(grad_y [y > 0], w mirrored and transposed); y is the saved forward output.
 *              The weights are frozen in the reference: there is no weight gradient.
 *   `packed`:  gfla_conv3x3_packed_bytes(Cout, Cin, layout, sizeof(T)) bytes, 16-byte aligned, written by
 *              gfla_conv3x3_pack_weights_<T> from w (Cout,Cin,3,3) stored as src_type 0 float32 / 1 float16 / 2 bfloat16
 *              and rounded once to T: [tap][chunk of 32 / sizeof(T) reduction channels][channels padded to 32][chunk],
 *              zero-padded.  layout 0 is what fwd reads, layout 1 (taps mirrored, Cin and Cout swapped) what bwd_data
 *              reads.
 * maxpool2x2: stride 2, floor mode, y (B,C,H/2,W/2); an odd last row / column is dropped and gets a zero gradient.  The
 * backward finds the winner again from the saved input x (first maximum in scan order, as F.max_pool2d) and writes every
 * element of grad_x exactly once.  H or W of 1 (empty output) is valid: fwd launches nothing, bwd writes zeros.
 * No atomics: everything here is bit-identical from call to call.  NULL -> -1; non-positive sizes, layout or src_type out
 * of range -> -2; H W > 2^31 - 1, B > 65535 or more than 65536 channels -> GFLA_ERR_UNSUPPORTED, nothing is launched.
 * Additive: GFLA_ABI_VERSION stays 8. */
int64_t gfla_conv3x3_packed_bytes(int64_t Cout, int64_t Cin, int layout, int elem_size);
#define GFLA_DECL_CONV3X3(SFX, T)                                                                                        \
  int gfla_conv3x3_relu_fwd_##SFX(const T *x, const void *packed, const float *bias, T *y, int64_t B, int64_t Cin,       \
                                  int64_t Cout, int64_t H, int64_t W, gfla_stream_t stream);                             \
  int gfla_conv3x3_relu_bwd_data_##SFX(const T *grad_y, const T *y, const void *packed_grad, T *grad_x, int64_t B,       \
                                       int64_t Cin, int64_t Cout, int64_t H, int64_t W, gfla_stream_t stream);           \
  int gfla_conv3x3_pack_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin, int layout,  \
                                      gfla_stream_t stream);
GFLA_DECL_CONV3X3(f32, float)
GFLA_DECL_CONV3X3(f16, uint16_t)
GFLA_DECL_CONV3X3(bf16, uint16_t)
#undef GFLA_DECL_CONV3X3

#define GFLA_DECL_MAXPOOL2X2(SFX, T)                                                                                     \
  int gfla_maxpool2x2_fwd_##SFX(const T *x, T *y, int64_t B, int64_t C, int64_t H, int64_t W, gfla_stream_t stream);     \
  int gfla_maxpool2x2_bwd_##SFX(const T *x, const T *grad_y, T *grad_x, int64_t B, int64_t C, int64_t H, int64_t W,      \
                                gfla_stream_t stream);
GFLA_DECL_MAXPOOL2X2(f32, float)
GFLA_DECL_MAXPOOL2X2(f16, uint16_t)
GFLA_DECL_MAXPOOL2X2(bf16, uint16_t)
#undef GFLA_DECL_MAXPOOL2X2

/* ---- fused InstanceNorm2d (+ affine) + LeakyReLU / ReLU (base_function.py:334-556: the `norm_layer(C) -> nonlinearity`
 * pair in front of every convolution of the generators' blocks; csrc/instance_norm.hip) ---------------------------------
 * Per plane (b, c) of N = H W values, x (B,C,H,W) contiguous in its storage type, arithmetic in float32 (float64 for _f64):
 *   mean, rstd = 1 / sqrt(biased variance + eps),  z = (x - mean) rstd gamma[c] + beta[c],  y = z > 0 ? z : slope z
 * gamma / beta: C values in the ARITHMETIC type, or NULL (1 / 0).  act = 0: y = z (plain instance norm); slope = 0: ReLU.
 * mean, rstd: B C values in the arithmetic type, written by fwd and read by bwd.  The variance is a centred sum of squares
 * over values held in registers (Chan's update across the workgroups of a split plane), never E[x^2] - mean^2.
 * bwd: z is recomputed from x (z == 0 takes the slope side); dx (B,C,H,W), dgamma (C), dbeta (C) may each be NULL and are
 * fully overwritten otherwise.  Per-plane sums go to the workspace and are added over b in ascending order: no atomics,
 * every result is bit-identical from call to call.
 * `workspace`: gfla_instance_norm_workspace_bytes(B, C, H, W, sizeof(T)) bytes, 8-byte aligned, uninitialised, for fwd and
 * for bwd.  x, y (x, dy, dx) may lie anywhere (aligned to their element): the head / vectors / tail split of a span follows
 * x's address and the other tensors are accessed at the same element offsets.
 * gfla_instance_norm_geometry: the launch plan, host only: out[0..6] = regime (0 wave per plane, 1 workgroup per plane, 2
 * split plane), threads per workgroup, planes per workgroup, workgroups per plane, values per thread, LDS bytes, workgroups
 * per launch.  It depends on (B C, H W, elem_size) only.
 * NULL -> -1; non-positive sizes, H W == 1, elem_size not 2 / 4 / 8 -> -2; H W or B C beyond 2^31 - 1, more than 4096
 * workgroups per plane -> GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive: GFLA_ABI_VERSION stays 8. */
int gfla_instance_norm_geometry(int64_t B, int64_t C, int64_t H, int64_t W, int elem_size, int is_backward, int64_t *out);
int64_t gfla_instance_norm_workspace_bytes(int64_t B, int64_t C, int64_t H, int64_t W, int elem_size);
int gfla_instance_norm_fwd_f32(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd, void *workspace,
                               int64_t B, int64_t C, int64_t H, int64_t W, double eps, double slope, int act,
                               gfla_stream_t stream);
int gfla_instance_norm_bwd_f32(const float *x, const float *dy, const float *gamma, const float *beta, const float *mean, const float *rstd,
                               float *dx, float *dgamma, float *dbeta, void *workspace, int64_t B, int64_t C, int64_t H, int64_t W,
                               double slope, int act, gfla_stream_t stream);
int gfla_instance_norm_fwd_f64(const double *x, const double *gamma, const double *beta, double *y, double *mean, double *rstd, void *workspace,
                               int64_t B, int64_t C, int64_t H, int64_t W, double eps, double slope, int act,
                               gfla_stream_t stream);
int gfla_instance_norm_bwd_f64(const double *x, const double *dy, const double *gamma, const double *beta, const double *mean, const double *rstd,
                               double *dx, double *dgamma, double *dbeta, void *workspace, int64_t B, int64_t C, int64_t H, int64_t W,
                               double slope, int act, gfla_stream_t stream);
int gfla_instance_norm_fwd_f16(const uint16_t *x, const float *gamma, const float *beta, uint16_t *y, float *mean, float *rstd, void *workspace,
                               int64_t B, int64_t C, int64_t H, int64_t W, double eps, double slope, int act,
                               gfla_stream_t stream);
int gfla_instance_norm_bwd_f16(const uint16_t *x, const uint16_t *dy, const float *gamma, const float *beta, const float *mean, const float *rstd,
                               uint16_t *dx, float *dgamma, float *dbeta, void *workspace, int64_t B, int64_t C, int64_t H, int64_t W,
                               double slope, int act, gfla_stream_t stream);
int gfla_instance_norm_fwd_bf16(const uint16_t *x, const float *gamma, const float *beta, uint16_t *y, float *mean, float *rstd, void *workspace,
                               int64_t B, int64_t C, int64_t H, int64_t W, double eps, double slope, int act,
                               gfla_stream_t stream);
int gfla_instance_norm_bwd_bf16(const uint16_t *x, const uint16_t *dy, const float *gamma, const float *beta, const float *mean, const float *rstd,
                               uint16_t *dx, float *dgamma, float *dbeta, void *workspace, int64_t B, int64_t C, int64_t H, int64_t W,
                               double slope, int act, gfla_stream_t stream);

/* ---- narrow 3x3 convolution heads with fused surroundings (base_function.py:650-670 `Output`; generator.py:203-209,
 * 237-242 the flow and mask heads; csrc/head_conv3x3.hip) -----------------------------------------------------------------
 *   a = pre_act ? leaky_relu(x, pre_slope) : x;  s = conv3x3(pad(a), w) + bias;  y_c = post_c(s_c)
 * x (B,Cin,H,W) contiguous in its storage type T (float32 / float16 / bfloat16), read as stored; w (Cout,Cin,3,3) and bias
 * (Cout, or NULL) are float32; sums are float32, a 16-bit result is rounded once.  Stride 1, one pixel of padding,
 * pad_mode 0 zeros / 1 reflect (-1 -> 1, H -> H-2), output H x W.  1 <= Cout <= 8, any Cin, B.  post_c: bit c of tanh_mask
 * -> tanh, bit c of sigmoid_mask -> sigmoid, neither -> identity.  Output channels [0, C0) go to y0 (B,C0,H,W), [C0, Cout)
 * to y1 (B,Cout-C0,H,W); y1 may be NULL when C0 == Cout.  Neither the activated nor the padded map exists in memory.
 * bwd: grad_y0 / grad_y1 may each be NULL (= zero); the post-activation's derivative is taken from the saved outputs y0 /
 * y1 (1 - y^2, y (1 - y)).  grad_x (B,Cin,H,W) in T, grad_w (Cout,Cin,3,3) and grad_b (Cout) in float32 may each be NULL
 * and are fully overwritten otherwise; x == 0 takes the slope side.  grad_x is owner-computes (reflect: the pad ring is
 * folded onto rows / columns 1 and H-2 / W-2); grad_w / grad_b recompute a from x, leave per-slab partials in `workspace`
 * (gfla_head_conv3x3_workspace_bytes bytes, 4-byte aligned, uninitialised; needed only with grad_w or grad_b) and a second
 * launch adds them in slab order: no atomics, no memset, every result is bit-identical from call to call.
 * gfla_head_conv3x3_geometry (host only): out[0..6] = tile width, tile height, threads per workgroup, tiles per plane of
 * the forward (is_backward = 0) or the grad_x kernel (1); rows per slab, slabs, channel groups of the grad_w kernel.
 * NULL -> -1; non-positive sizes, Cout > 8, C0 outside [1, Cout], mask bits beyond Cout or in both masks, pad_mode not
 * 0 / 1, reflect with H or W < 2, elem_size not 2 / 4 -> -2; H W beyond 2^31 - 1 or more workgroups than a launch takes
 * -> GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive: GFLA_ABI_VERSION stays 8. */
int64_t gfla_head_conv3x3_workspace_bytes(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int elem_size);
int gfla_head_conv3x3_geometry(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int is_backward, int64_t *out);
int gfla_head_conv3x3_fwd_f32(const float *x, const float *w, const float *bias, float *y0, float *y1, int64_t B, int64_t Cin,
                               int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act, double pre_slope,
                               int tanh_mask, int sigmoid_mask, gfla_stream_t stream);
int gfla_head_conv3x3_bwd_f32(const float *x, const float *w, const float *y0, const float *y1, const float *grad_y0,
                               const float *grad_y1, float *grad_x, float *grad_w, float *grad_b, void *workspace, int64_t B,
                               int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act,
                               double pre_slope, int tanh_mask, int sigmoid_mask, gfla_stream_t stream);
int gfla_head_conv3x3_fwd_f16(const uint16_t *x, const float *w, const float *bias, uint16_t *y0, uint16_t *y1, int64_t B, int64_t Cin,
                               int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act, double pre_slope,
                               int tanh_mask, int sigmoid_mask, gfla_stream_t stream);
int gfla_head_conv3x3_bwd_f16(const uint16_t *x, const float *w, const uint16_t *y0, const uint16_t *y1, const uint16_t *grad_y0,
                               const uint16_t *grad_y1, uint16_t *grad_x, float *grad_w, float *grad_b, void *workspace, int64_t B,
                               int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act,
                               double pre_slope, int tanh_mask, int sigmoid_mask, gfla_stream_t stream);
int gfla_head_conv3x3_fwd_bf16(const uint16_t *x, const float *w, const float *bias, uint16_t *y0, uint16_t *y1, int64_t B, int64_t Cin,
                               int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act, double pre_slope,
                               int tanh_mask, int sigmoid_mask, gfla_stream_t stream);
int gfla_head_conv3x3_bwd_bf16(const uint16_t *x, const float *w, const uint16_t *y0, const uint16_t *y1, const uint16_t *grad_y0,
                               const uint16_t *grad_y1, uint16_t *grad_x, float *grad_w, float *grad_b, void *workspace, int64_t B,
                               int64_t Cin, int64_t Cout, int64_t C0, int64_t H, int64_t W, int pad_mode, int pre_act,
                               double pre_slope, int tanh_mask, int sigmoid_mask, gfla_stream_t stream);

/* ---- generator inference convolutions (csrc/gen_conv.hip): gfla_gen_conv_*, declared and documented in gfla_gen_conv.h ---- */
#include "gfla_gen_conv.h"

/* ---- launch geometry of the planes-in-LDS kernels (csrc/lds_plane.h), for tests: gfla_lds_plane_geometry, declared and
 * documented in gfla_lds_plane.h ---- */
#include "gfla_lds_plane.h"

/* ---- spectral normalisation of a batch of weight matrices (csrc/spectral_norm.hip): gfla_spectral_norm_*, declared and
 * documented in gfla_spectral_norm.h ---- */
#include "gfla_spectral_norm.h"

/* ---- frames-major 3-D convolutions and their pool (csrc/conv3d.hip, csrc/avg_pool_frames.hip): gfla_conv3d_*,
 * gfla_avg_pool_frames_*, declared and documented in gfla_conv3d.h ---- */
#include "gfla_conv3d.h"

/* ---- one Adam / AdamW step over all parameters of a group (csrc/adam.hip): gfla_adam_*, declared and documented in
 * gfla_adam.h ---- */
#include "gfla_adam.h"

/* ---- pose inputs: key points -> heat maps and back, uint8 images -> network input (csrc/pose_inputs.hip): gfla_pose_*,
 * gfla_normalize_images_*, declared and documented in gfla_pose.h ---- */
#include "gfla_pose.h"

/* ---- image inputs: Pillow's nearest-neighbour affine transform fused with ToTensor + Normalize, Pillow's 8-bit resize
 * (csrc/image_inputs.hip): gfla_affine_images_*, gfla_resize_pass_u8, declared and documented in gfla_image.h ---- */
#include "gfla_image.h"

/* ---- reconstruction metrics: generator output -> bytes, SSIM (uniform and Gaussian window), PSNR, L1, MAE of byte images
 * (csrc/recon_metrics.hip): gfla_images_to_uint8_*, gfla_recon_metrics*, declared and documented in gfla_metrics.h ---- */
#include "gfla_metrics.h"

#ifdef __cplusplus
}
#endif
#endif /* GFLA_HIP_H_ */
