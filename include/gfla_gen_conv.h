/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- generator inference convolutions (base_function.py:334-391 EncoderBlock / ResBlock, 508-531 ResBlockDecoder, 672-691
 * Jump; csrc/gen_conv.hip) -------------------------------------------------------------------------------------------------
 * Forward (frozen or trainable weights) and, further down, the gradients.  x (B,Cin,H,W) contiguous in its storage type T (float32 / float16 / bfloat16), read as
 * stored; sums are float32 on the matrix cores, a 16-bit result is rounded to nearest even once.  groups 1, dilation 1.
 *   a = pre_act ? leaky_relu(x, pre_slope) rounded to T : x
 *   y = bias + conv(a, w) (+ add)
 * geometry 0  S1K3  Conv2d(k 3, s 1) with one pixel of padding, pad_mode 0 zeros / 1 reflect (-1 -> 1, H -> H-2; needs H, W
 *                   >= 2); y (B,Cout,H,W).
 * geometry 1  S2K4  Conv2d(k 4, s 2, p 1), zero padding, H, W >= 2 (odd sizes are valid); y (B,Cout,(H-2)/2+1,(W-2)/2+1).
 * geometry 2  T2K3  ConvTranspose2d(k 3, s 2, p 1, output_padding 1), w (Cin,Cout,3,3); y (B,Cout,2H,2W), computed as four
 *                   output phases of 1 / 2 / 2 / 4 taps per input pixel; y and add are accessed in pairs of elements, on any
 *                   element boundary.
 * bias: Cout float32 values, or NULL.  add: NULL, or a tensor of y's shape and type, added in float32 before the one
 * rounding; add == y (in place) is allowed.
 * `packed`: gfla_gen_conv_packed_bytes(Cout, Cin, geometry, sizeof(T)) bytes, 16-byte aligned, written by
 *           gfla_gen_conv_pack_weights_<T> from torch's weight tensor as stored ((Cout,Cin,k,k), geometry 2: (Cin,Cout,3,3))
 *           in src_type 0 float32 / 1 float16 / 2 bfloat16, rounded once to T:
 *           [tap = ky k + kx][chunk of 32 / sizeof(T) input channels][Cout padded to 32][chunk], zero-padded; 9 / 16 / 9 taps.
 * gfla_gen_conv_out_size: the output size of a geometry.
 * gfla_gen_conv_geometry (host only): out[0..7] = tile width, tile height (in pixels of the tiled map: the output for
 * geometry 0 / 1, the input for geometry 2), waves along the output channels, tiles along x, tiles along y, channel blocks
 * (grid = tiles x channel blocks x B), halo records per LDS buffer, LDS bytes of a workgroup.
 * No atomics: bit-identical from call to call.  NULL x / packed / y (w, out, Hout, Wout) -> -1; non-positive sizes,
 * geometry, pad_mode, src_type or elem_size out of range, pad_mode 1 with another geometry than 0 or with H or W < 2,
 * geometry 1 with H or W < 2 -> -2; a plane of x or y beyond 2^31 - 1, B > 65535 or more than 65536 channels ->
 * GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive: GFLA_ABI_VERSION stays 8.
 *
 * ---- gradients (csrc/gen_conv_bwd.hip, csrc/gen_conv_wgrad.hip) -------------------------------------------------------
 * `geometry`, `pad_mode`, `pre_act`, `pre_slope`, B, Cin, Cout, H, W are the forward's everywhere; grad_y has y's shape
 * and type, x is the forward's input as stored (nothing else is saved: a is recomputed from it).
 *   grad_x = act'(x) adj(grad_y, w),  act'(x) = x > 0 ? 1 : pre_slope (1 without pre_act); x's shape and type, rounded once
 *   grad_w[co][ci][tap] = sum over (b, pixel) of grad_y a, float32 in torch's layout ((Cout,Cin,k,k); geometry 2:
 *                         (Cin,Cout,3,3));  grad_b[co] = sum of grad_y, float32
 * `packed_grad`: gfla_gen_conv_grad_packed_bytes(Cout, Cin, geometry, sizeof(T)) bytes, 16-byte aligned, written by
 *           gfla_gen_conv_pack_grad_weights_<T> from torch's weight as stored: the packing of the adjoint geometry
 *           [tap][chunk of 32 / sizeof(T) OUTPUT channels][Cin padded to 32][chunk]; geometry 0: taps mirrored (9),
 *           geometry 1: the 16 taps as stored (four phases of 2 x 2 over the half-resolution grid), geometry 2: the 9 taps
 *           as stored (a Conv2d(k 3, s 2, p 1) of grad_y).
 * `workspace`: gfla_gen_conv_bwd_workspace_bytes(B, Cin, Cout, H, W, geometry, pad_mode, sizeof(T)) bytes, uninitialised,
 *           16-byte aligned; enough for either call.  bwd_data reads it only with pad_mode 1 (the gradient on the padded
 *           domain, float32, folded onto x by a second launch; NULL is accepted otherwise); bwd_weight holds the float32
 *           partial sums of the split reduction in it, summed in a fixed order by a second launch.
 * gfla_gen_conv_bwd_weight: grad_w or grad_b may be NULL (not computed); both NULL -> -1; x and workspace may be NULL
 *           when grad_w is.
 * No atomics: bit-identical from call to call.  Status codes as above: NULL -> -1, the forward's bad shapes -> -2, the
 * forward's limits or B x (pixels of the reduction) beyond 2^31 - 1 -> GFLA_ERR_UNSUPPORTED, nothing is launched.
 *
 * ---- 1x1 convolutions (discriminator.py: ResBlockEncoder's pooled shortcut, the final Conv2d(C, 1, 1); base_function.py:
 * ResBlock's learnable shortcut; csrc/conv1x1.hip, csrc/gen_conv_wgrad.hip) ---------------------------------------------
 * Functions of their own; the entry points above are untouched and keep refusing any geometry but 0 .. 2.
 *   p = pool == 2 ? avg_pool2d(x, 2, 2) : pre_act ? leaky_relu(x, pre_slope) : x       rounded to T once
 *   y = bias + conv1x1(p, w), w (Cout,Cin,1,1); y (B,Cout,H/pool,W/pool), torch's floor: an odd trailing row or column is
 *       dropped.  The pooled value is the float32 sum ((x00 + x01) + x10) + x11 times 0.25.  No addend.
 *   grad_x: pool 1: act'(x) sum_co w g; pool 2: 0.25 sum_co w g at the four elements of the block, and ZERO in the trailing
 *           row / column of an odd H / W, written by the same launch: grad_x may be uninitialised, every element is written.
 *   grad_w[co][ci] = sum over (b, pixel) of grad_y p, grad_b[co] = sum of grad_y: float32, the split reduction and the
 *           bias kernel of the gradients above.
 * `packed`: gfla_conv1x1_packed_bytes bytes, [chunk of 32 / sizeof(T) input channels][Cout padded to 32][chunk];
 * `packed_grad`: gfla_conv1x1_grad_packed_bytes bytes, the transposed weight, [chunk of OUTPUT channels][Cin padded to
 * 32][chunk]; `workspace` (bwd_weight only): gfla_conv1x1_bwd_workspace_bytes bytes, uninitialised, 16-byte aligned.
 * bias may be NULL; bwd_data reads x only with pre_act (NULL is accepted otherwise); bwd_weight: as above.
 * No atomics: bit-identical from call to call.  NULL -> -1; non-positive sizes, pool other than 1 / 2, pool 2 with H or W
 * < 2 or with pre_act, src_type or elem_size out of range -> -2; a plane of x beyond 2^31 - 257, B > 65535, more than
 * 65536 channels or B x (output pixels) beyond 2^31 - 1 -> GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive:
 * GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_GEN_CONV_H_
#define GFLA_GEN_CONV_H_

int64_t gfla_gen_conv_packed_bytes(int64_t Cout, int64_t Cin, int geometry, int elem_size);
int gfla_gen_conv_out_size(int geometry, int64_t H, int64_t W, int64_t *Hout, int64_t *Wout);
int gfla_gen_conv_geometry(int geometry, int64_t Cout, int64_t H, int64_t W, int elem_size, int64_t *out);
#define GFLA_DECL_GEN_CONV(SFX, T)                                                                                       \
  int gfla_gen_conv_pack_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,             \
                                       int geometry, gfla_stream_t stream);                                              \
  int gfla_gen_conv_fwd_##SFX(const T *x, const void *packed, const float *bias, const T *add, T *y, int64_t B,          \
                              int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry, int pad_mode, int pre_act,  \
                              double pre_slope, gfla_stream_t stream);
int64_t gfla_gen_conv_grad_packed_bytes(int64_t Cout, int64_t Cin, int geometry, int elem_size);
int64_t gfla_gen_conv_bwd_workspace_bytes(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry,
                                          int pad_mode, int elem_size);
#define GFLA_DECL_GEN_CONV_BWD(SFX, T)                                                                                   \
  int gfla_gen_conv_pack_grad_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,        \
                                            int geometry, gfla_stream_t stream);                                         \
  int gfla_gen_conv_bwd_data_##SFX(const T *grad_y, const T *x, const void *packed_grad, T *grad_x, void *workspace,     \
                                   int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry,             \
                                   int pad_mode, int pre_act, double pre_slope, gfla_stream_t stream);                   \
  int gfla_gen_conv_bwd_weight_##SFX(const T *grad_y, const T *x, float *grad_w, float *grad_b, void *workspace,         \
                                     int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int geometry,           \
                                     int pad_mode, int pre_act, double pre_slope, gfla_stream_t stream);
GFLA_DECL_GEN_CONV(f32, float)
GFLA_DECL_GEN_CONV(f16, uint16_t)
GFLA_DECL_GEN_CONV(bf16, uint16_t)
#undef GFLA_DECL_GEN_CONV
GFLA_DECL_GEN_CONV_BWD(f32, float)
GFLA_DECL_GEN_CONV_BWD(f16, uint16_t)
GFLA_DECL_GEN_CONV_BWD(bf16, uint16_t)
#undef GFLA_DECL_GEN_CONV_BWD

int64_t gfla_conv1x1_packed_bytes(int64_t Cout, int64_t Cin, int elem_size);
int64_t gfla_conv1x1_grad_packed_bytes(int64_t Cout, int64_t Cin, int elem_size);
int64_t gfla_conv1x1_bwd_workspace_bytes(int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool,
                                         int elem_size);
#define GFLA_DECL_CONV1X1(SFX, T)                                                                                        \
  int gfla_conv1x1_pack_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,              \
                                      gfla_stream_t stream);                                                             \
  int gfla_conv1x1_pack_grad_weights_##SFX(const void *w, int src_type, void *packed, int64_t Cout, int64_t Cin,         \
                                           gfla_stream_t stream);                                                        \
  int gfla_conv1x1_fwd_##SFX(const T *x, const void *packed, const float *bias, T *y, int64_t B, int64_t Cin,            \
                             int64_t Cout, int64_t H, int64_t W, int pool, int pre_act, double pre_slope,                \
                             gfla_stream_t stream);                                                                      \
  int gfla_conv1x1_bwd_data_##SFX(const T *grad_y, const T *x, const void *packed_grad, T *grad_x, int64_t B,            \
                                  int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool, int pre_act,                \
                                  double pre_slope, gfla_stream_t stream);                                               \
  int gfla_conv1x1_bwd_weight_##SFX(const T *grad_y, const T *x, float *grad_w, float *grad_b, void *workspace,          \
                                    int64_t B, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int pool, int pre_act,   \
                                    double pre_slope, gfla_stream_t stream);
GFLA_DECL_CONV1X1(f32, float)
GFLA_DECL_CONV1X1(f16, uint16_t)
GFLA_DECL_CONV1X1(bf16, uint16_t)
#undef GFLA_DECL_CONV1X1

#endif /* GFLA_GEN_CONV_H_ */
