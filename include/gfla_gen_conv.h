/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- generator inference convolutions (base_function.py:334-391 EncoderBlock / ResBlock, 508-531 ResBlockDecoder, 672-691
 * Jump; csrc/gen_conv.hip) -------------------------------------------------------------------------------------------------
 * Forward only, frozen weights.  x (B,Cin,H,W) contiguous in its storage type T (float32 / float16 / bfloat16), read as
 * stored; sums are float32 on the matrix cores, a 16-bit result is rounded to nearest even once.  groups 1, dilation 1.
 *   a = pre_act ? leaky_relu(x, pre_slope) rounded to T : x
 *   y = bias + conv(a, w) (+ add)
 * geometry 0  S1K3  Conv2d(k 3, s 1) with one pixel of padding, pad_mode 0 zeros / 1 reflect (-1 -> 1, H -> H-2; needs H, W
 *                   >= 2); y (B,Cout,H,W).
 * geometry 1  S2K4  Conv2d(k 4, s 2, p 1), zero padding, H, W >= 2 (odd sizes are valid); y (B,Cout,(H-2)/2+1,(W-2)/2+1).
 * geometry 2  T2K3  ConvTranspose2d(k 3, s 2, p 1, output_padding 1), w (Cin,Cout,3,3); y (B,Cout,2H,2W), computed as four
 *                   output phases of 1 / 2 / 2 / 4 taps per input pixel; y and add must be aligned to two elements.
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
 * GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive: GFLA_ABI_VERSION stays 8. */
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
GFLA_DECL_GEN_CONV(f32, float)
GFLA_DECL_GEN_CONV(f16, uint16_t)
GFLA_DECL_GEN_CONV(bf16, uint16_t)
#undef GFLA_DECL_GEN_CONV

#endif /* GFLA_GEN_CONV_H_ */
