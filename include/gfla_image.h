/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- image inputs on the device: Pillow's nearest-neighbour affine transform fused with ToTensor + Normalize, and
 * Pillow's 8-bit bilinear / bicubic resize (csrc/image_inputs.hip) ----------------------------------------------------
 * gfla_affine_images_*: `images` (B, H, W, C) uint8, C in 1..4; `inverse` (B, 2, 3) double on the device, m = inverse[b]
 *   maps an output pixel to a source pixel; `out` (B, C, H, W) in the suffix's storage type, every element written.
 *   out[b, c, y, x] = ((v / 255) - mean[c]) / std[c] in float32 -- a division, a subtraction, a division, rounded once
 *   more for 16-bit storage: gfla_normalize_images_*' value -- of the byte v = images[b, yin, xin, c] where 0 <= xin < W
 *   and 0 <= yin < H, and of v = fill[c] elsewhere.  All double arithmetic without contraction; per sample:
 *     poisoned      an entry of m is not finite, or |x*m[0] + y*m[1] + m[2]| or |x*m[3] + y*m[4] + m[5]| (summed left to
 *                   right) is not below 32767 at a corner x in {0, W}, y in {0, H}: the sample's whole image is NaN
 *     scale branch  m[1] == 0 and m[3] == 0 (also for -0), Pillow's ImagingScaleAffine: xo = m[2] + m[0]*0.5; for x = 0,
 *                   1, ... W-1 in turn xin = xo < 0 ? -1 : (int)xo, then xo += m[0] -- the repeated addition is part of
 *                   the result; rows likewise from m[5] and m[4]
 *     otherwise     Pillow's affine_fixed, FIX(v) = (int)floor(v*65536.0 + 0.5): a0, a1, a3, a4 = FIX(m[0]), FIX(m[1]),
 *                   FIX(m[3]), FIX(m[4]); a2 = FIX(m[2] + m[0]*0.5 + m[1]*0.5), a5 = FIX(m[5] + m[3]*0.5 + m[4]*0.5),
 *                   summed left to right; xin = (a2 + a0*x + a1*y) >> 16, yin = (a5 + a3*x + a4*y) >> 16, arithmetic
 *                   shifts of sums that fit an int32 (that is what the bound of 32767 is for)
 *   `workspace`: gfla_affine_images_workspace_bytes(B, H, W) bytes, 4-byte aligned, uninitialised: a first kernel writes
 *   each sample's branch, fixed-point coefficients and the scale branch's xin[W], yin[H] there, the second one gathers.
 *   Nothing is read back.  `fill`, `mean`, `std`: C doubles each in HOST memory; fill whole numbers 0..255, mean and std
 *   rounded to float32 first.
 * gfla_resize_pass_u8: one axis of Pillow's Image.resize for 8-bit channels.  `src` (outer, in_len, inner) uint8 ->
 *   `dst` (outer, out_len, inner) uint8; `coeffs` (out_len, ksize) int32 in units of 2^-22 and `bounds` (out_len, 2) int32,
 *   rows (first, count), on the device:
 *     dst[o, j, i] = clamp((2^21 + sum over k < count[j] of src[o, first[j] + k, i] * coeffs[j, k]) >> 22, 0, 255)
 *   in 32-bit integers.  first and count are clamped to the source, so no table makes the kernel read outside `src`.  The
 *   horizontal pass of (B, h, w, C) images is outer = B h, inner = C; the vertical one outer = B, inner = W C.
 * Every pointer may sit at any multiple of its element size; the affine kernel stores 16 bytes per access with
 * element-wise heads and tails.
 * NULL images / inverse / out / workspace / fill / mean / std / src / dst / coeffs / bounds -> -1; B, H, W, outer, in_len,
 * out_len, inner, ksize <= 0, C outside 1..4, a fill that is no whole number 0..255, a std of 0, a non-finite mean or std
 * -> -2; H or W > 32768, H * W > 2^31 - 1, a source or destination of a pass of more than 2^31 - 1 bytes, ksize > 4096 or
 * more than 2^31 - 1 workgroups -> GFLA_ERR_UNSUPPORTED.  All decided before anything is launched;
 * gfla_affine_images_workspace_bytes returns the same codes.
 * Additive: GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_IMAGE_H_
#define GFLA_IMAGE_H_

int64_t gfla_affine_images_workspace_bytes(int64_t B, int64_t H, int64_t W);
int gfla_affine_images_f32(const uint8_t *images, const double *inverse, float *out, void *workspace, int64_t B, int64_t H,
                           int64_t W, int64_t C, const double *fill, const double *mean, const double *std,
                           gfla_stream_t stream);
int gfla_affine_images_f16(const uint8_t *images, const double *inverse, uint16_t *out, void *workspace, int64_t B, int64_t H,
                           int64_t W, int64_t C, const double *fill, const double *mean, const double *std,
                           gfla_stream_t stream);
int gfla_affine_images_bf16(const uint8_t *images, const double *inverse, uint16_t *out, void *workspace, int64_t B, int64_t H,
                            int64_t W, int64_t C, const double *fill, const double *mean, const double *std,
                            gfla_stream_t stream);
int gfla_resize_pass_u8(const uint8_t *src, uint8_t *dst, const int32_t *coeffs, const int32_t *bounds, int64_t outer,
                        int64_t in_len, int64_t out_len, int64_t inner, int64_t ksize, gfla_stream_t stream);

#endif /* GFLA_IMAGE_H_ */
