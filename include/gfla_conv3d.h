/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- frames-major 3-D convolutions (base_function.py:43-67 ResBlock3DEncoder, the two 3-D blocks of discriminator.py's
 * TemporalDiscriminator; csrc/conv3d.hip, csrc/gen_conv_wgrad.hip, csrc/avg_pool_frames.hip) ---------------------------------
 * Layout: activations are FRAMES-MAJOR, x (B,L,C,H,W) contiguous in its storage type T (float32 / float16 / bfloat16) --
 * torch's Conv3d takes (B,C,L,H,W) --, so every frame is an NCHW sample and the 3 frames that start at frame f are one
 * contiguous (3 C,H,W) map.  Sums are float32 on the matrix cores, a 16-bit result is rounded to nearest even once; the
 * three temporal taps belong to one sum.  groups 1, dilation 1, temporal kernel 3, temporal stride 1.
 *   a = pre_act ? leaky_relu(x, pre_slope) rounded to T : x
 *   y = bias + conv3d(a, w) (+ add)                           y (B,Lout,Cout,Hout,Wout), frames-major again
 * geometry 0  k333  Conv3d(k (3,3,3), s 1, p (1,1,1)); Lout = L, Hout = H, Wout = W.
 * geometry 1  k344  Conv3d(k (3,4,4), s (1,2,2), p (0,1,1)); Lout = L - 2, Hout = (H-2)/2+1, Wout = (W-2)/2+1; needs
 *                   L >= 3 and H, W >= 2 (odd sizes are valid).
 * The window rule: output sample (b, lo) is the 2-D convolution (gfla_gen_conv.h's geometry 0 / 1) over the 3 C channels
 * of frames lo - pt .. lo - pt + 2 of sample b (pt the temporal padding: 1 / 0); channels of frames outside [0, L) read as
 * zero and are never addressed.  Reduced channel kt C + c is w[co][c][kt]:
 * `packed`: gfla_gen_conv_packed_bytes(Cout, 3 C, geometry, sizeof(T)) bytes, written by gfla_gen_conv_pack_weights_<T>
 *           with Cin = 3 C from w.permute(0,2,1,3,4), contiguous, read as (Cout, 3 C, k, k).
 * bias: Cout float32 values, or NULL.  add: NULL, or a tensor of y's shape and type, added in float32 before the one
 * rounding; add == y (in place) is allowed.
 *
 * Gradients.  `geometry`, `pre_act`, `pre_slope`, B, L, C, Cout, H, W are the forward's everywhere; grad_y has y's shape and
 * type, x is the forward's input as stored (nothing else is saved: a is recomputed from it).
 *   grad_x = act'(x) adj(grad_y, w): sample (b, l) is the adjoint 2-D convolution over the 3 Cout channels of frames
 *           l - (2 - pt) .. l + pt of grad_y, clipped to [0, Lout); x's shape and type, rounded once.  bwd_data reads x only
 *           with pre_act (NULL is accepted otherwise).
 * `packed_grad`: gfla_gen_conv_grad_packed_bytes(3 Cout, C, geometry, sizeof(T)) bytes, written by
 *           gfla_gen_conv_pack_grad_weights_<T> with Cout' = 3 Cout from the weight with its temporal taps reversed,
 *           w.flip(2).permute(2,0,1,3,4), contiguous, read as (3 Cout, C, k, k): row j Cout + co is w[co][.][2 - j].
 *   grad_w[co][kt C + c][tap] = sum over (b, lo, pixel) of grad_y a, float32, (Cout, 3 C, k, k): the caller permutes it
 *           back to (Cout, C, 3, k, k).  grad_b[co] = sum of grad_y, float32.  Either may be NULL (not computed), both NULL
 *           -> -1; x and workspace may be NULL when grad_w is.
 * `workspace`: gfla_conv3d_bwd_workspace_bytes(B, L, C, Cout, H, W, geometry, sizeof(T)) bytes, uninitialised, 16-byte
 *           aligned: the float32 partial sums of the split reduction, summed in a fixed order by a second launch.
 *
 * gfla_avg_pool_frames_*: AvgPool3d(kernel (3,2,2), stride (1,2,2)) on the same layout, x (B,L,C,H,W) -> y (B,L-2,C,H/2,
 *   W/2), torch's floor: an odd trailing row or column is dropped.  The value is one float32 sum over frames lo .. lo + 2
 *   ascending, within a frame ((x00 + x01) + x10) + x11, times 1/12, rounded to T once.  bwd: grad_x[b,l,c,y,x] = (1/12)
 *   sum over lo in [max(0, l-2), min(l, L-3)] of grad_y[b,lo,c,y/2,x/2], lo ascending, rounded once, and ZERO in the
 *   trailing row / column of an odd H / W: grad_x may be uninitialised, every element is written by exactly one lane.
 *   16-byte accesses where the row length and the pointers allow, element accesses otherwise, the same bits either way.
 *   The 1x1x1 convolution behind the pool is gfla_conv1x1_* (pool 1) on the pooled (B (L-2), C, H/2, W/2) batch.
 *
 * No atomics anywhere: bit-identical from call to call.  NULL -> -1; non-positive sizes, a geometry other than 0 / 1,
 * elem_size other than 2 / 4, geometry 1 (and the pool) with L < 3 or H or W < 2 -> -2; a plane of x or y beyond 2^31 - 1,
 * B L or B Lout beyond 65535, more than 65536 windowed channels (3 C or 3 Cout; the pool: C), a reduction of the weight
 * gradient (B Lout Hout Wout) beyond 2^31 - 1, or a pointer not aligned to its element -> GFLA_ERR_UNSUPPORTED; nothing is
 * launched on a refusal.  Additive: GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_CONV3D_H_
#define GFLA_CONV3D_H_

int gfla_conv3d_out_size(int geometry, int64_t L, int64_t H, int64_t W, int64_t *Lout, int64_t *Hout, int64_t *Wout);
int64_t gfla_conv3d_bwd_workspace_bytes(int64_t B, int64_t L, int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry,
                                        int elem_size);
#define GFLA_DECL_CONV3D(SFX, T)                                                                                         \
  int gfla_conv3d_fwd_##SFX(const T *x, const void *packed, const float *bias, const T *add, T *y, int64_t B, int64_t L, \
                            int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act, double pre_slope,  \
                            gfla_stream_t stream);                                                                       \
  int gfla_conv3d_bwd_data_##SFX(const T *grad_y, const T *x, const void *packed_grad, T *grad_x, int64_t B, int64_t L,  \
                                 int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry, int pre_act,               \
                                 double pre_slope, gfla_stream_t stream);                                                \
  int gfla_conv3d_bwd_weight_##SFX(const T *grad_y, const T *x, float *grad_w, float *grad_b, void *workspace,           \
                                   int64_t B, int64_t L, int64_t C, int64_t Cout, int64_t H, int64_t W, int geometry,    \
                                   int pre_act, double pre_slope, gfla_stream_t stream);                                 \
  int gfla_avg_pool_frames_fwd_##SFX(const T *x, T *y, int64_t B, int64_t L, int64_t C, int64_t H, int64_t W,            \
                                     gfla_stream_t stream);                                                              \
  int gfla_avg_pool_frames_bwd_##SFX(const T *grad_y, T *grad_x, int64_t B, int64_t L, int64_t C, int64_t H, int64_t W,  \
                                     gfla_stream_t stream);
GFLA_DECL_CONV3D(f32, float)
GFLA_DECL_CONV3D(f16, uint16_t)
GFLA_DECL_CONV3D(bf16, uint16_t)
#undef GFLA_DECL_CONV3D

#endif /* GFLA_CONV3D_H_ */
