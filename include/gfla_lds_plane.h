/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- launch geometry of the planes-in-LDS kernels (csrc/lds_plane.h: PlaneGeo), for tests -- host only, no GPU needed ----
 * gfla_lds_plane_geometry answers with the geometry a launch of the family would use right now.  The launchers and this query
 * call the same functions for the GATE (does the family take the call at all: csrc/gs_route.h, one route function per
 * entry-point family) as well as for the geometry; the tuning keys 4 = cap on G, 5 = split, 10 = LDS budget in KB are honoured
 * as a launch honours them:
 *   op 0 block_extractor backward, gradient of a (B,C,kH,kW) tensor     1 the attention-factored form (aggregation backward)
 *      2 the unfold form (gradient in unfold layout)                    3 unfold + attention in one pass
 *      4 block_extractor unfold forward
 *      5 resample2d forward      6 resample2d d/d input1 (scatter planes)      7 resample2d d/d input2 (gather planes)
 *   (Hs, Ws) the source plane, (H, W) the flow / output grid, k = kernel_size, dilation (resample2d; 1 otherwise),
 *   elem_size = sizeof the storage type (2 / 4 / 8); needs (ops 0-3): bit 0 = grad_source wanted, bit 1 = grad_flow wanted.
 *   out[6] = G (channel planes per workgroup), channel groups (the last one holds C - (groups - 1) G planes), split (workgroups
 *   sharing one (b, group)), work items per workgroup, margin (< 0: whole planes resident; >= 0: a row window, taps beyond it
 *   read global memory), dynamic LDS bytes.  G = 0 (and the rest 0) when the family does not take the call: planes beyond the
 *   budget where the kernel needs whole ones, the big-plane regime of csrc/tile_map.h, or the family switched off (keys 2, 6).
 *   Ops 5-7 describe rs_lds_kernel; a float32 d/d input2 with kernel_size 4, dilation 1 is served by the streaming kernel of
 *   csrc/rs_taps.h first (tuning key 22 = 1 turns that off).
 * Kernels that cannot flush a shared plane (16-bit storage: ops 0-3 and 6) report split = 1 whatever key 5 says.
 * NULL out -> -1; non-positive sizes, op outside 0-7, elem_size not 2 / 4 / 8, ops 0-3 without a wanted gradient, ops 5-7 with
 * k < 2 -> -2.  Additive: GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_LDS_PLANE_H_
#define GFLA_LDS_PLANE_H_

int gfla_lds_plane_geometry(int op, int64_t B, int64_t C, int64_t Hs, int64_t Ws, int64_t H, int64_t W, int k, int dilation,
                            int elem_size, int needs, int64_t *out);

#endif /* GFLA_LDS_PLANE_H_ */
