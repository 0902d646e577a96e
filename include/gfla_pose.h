/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- pose inputs on the device: key points -> heat maps, heat maps -> key points, uint8 images -> network input
 * (csrc/pose_inputs.hip) --------------------------------------------------------------------------------------------
 * gfla_pose_maps_*: `cords` (B, J, 2) double on the device, a row = (y, x); `affine` NULL or B matrices of
 *   `affine_stride` doubles each (6: (B, 2, 3), 9: (B, 3, 3); rows 0 and 1 are applied); `out` (B, J, H, W) in the
 *   suffix's storage type, every element written by the kernel (no memset pass).  Per joint, in double, without
 *   contraction:
 *     missing   y == -1 or x == -1, tested first: the channel is +0
 *     p0 = (y / H0) * H, p1 = (x / W0) * W                 a division, then a multiplication, also for H0 == H
 *     r0 = a00*p1 + a01*p0 + a02, r1 = a10*p1 + a11*p0 + a12      summed left to right; c0 = trunc(r1), c1 = trunc(r0)
 *     without an affine c0 = trunc(p0), c1 = trunc(p1); trunc is toward zero; the centre is clamped to +-2^30
 *     out[b, j, y, x] = float32(ex[x] * ey[y]),  ex[x] = exp(-((x - c1)^2) / two_sigma_sq), ey likewise with c0:
 *       the product is taken in double and rounded to float32 once (float32 denormals are kept), 16-bit storage is
 *       that float32 rounded to nearest even once
 *   A joint that is not missing and has a non-finite coordinate, a non-finite entry among the `affine_stride` of its
 *   sample's matrix, or a NaN r0 / r1, has its channel filled with NaN.
 *   two_sigma_sq = 2 * sigma^2, formed by the caller in double.
 * gfla_pose_cords_*: `maps` (planes, H, W) in the suffix's storage type -> `out` (planes, 2) int64.  Per plane the
 *   maximum, compared as float32 (16-bit storage widened; -0 == +0); if it is > (float)threshold the result is (y, x) of
 *   its first occurrence in row-major order, else (-1, -1); a plane that holds a NaN gives (-1, -1).  One workgroup per
 *   plane, no atomics: bit-identical from call to call.
 * gfla_normalize_images_*: `images` (B, H, W, C) uint8, C in 1..4 -> `out` (B, C, H, W); per element
 *   ((v / 255) - mean[c]) / std[c] in float32: a division, a subtraction, a division, rounded once more for 16-bit
 *   storage.  `mean`, `std`: C doubles in HOST memory, rounded to float32 first.
 * Every pointer may sit at any multiple of its element size; the kernels move 16 bytes per access with element-wise
 * heads and tails.
 * NULL cords / out / maps / images / mean / std -> -1; B, J, H, W, planes <= 0, H0 or W0 <= 0, two_sigma_sq or
 * threshold NaN, two_sigma_sq <= 0 or infinite, affine_stride not 6 or 9 with an affine, C outside 1..4, a std of 0, a
 * non-finite mean or std -> -2; W > 4096 (maps), H * W > 2^31 - 1 or more than 2^31 - 1 workgroups ->
 * GFLA_ERR_UNSUPPORTED.  All decided before anything is launched.
 * Additive: GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_POSE_H_
#define GFLA_POSE_H_

int64_t gfla_pose_maps_band_rows(void);
int gfla_pose_maps_f32(const double *cords, const double *affine, int64_t affine_stride, float *out, int64_t B, int64_t J,
                       int64_t H, int64_t W, int64_t H0, int64_t W0, double two_sigma_sq, gfla_stream_t stream);
int gfla_pose_maps_f16(const double *cords, const double *affine, int64_t affine_stride, uint16_t *out, int64_t B, int64_t J,
                       int64_t H, int64_t W, int64_t H0, int64_t W0, double two_sigma_sq, gfla_stream_t stream);
int gfla_pose_maps_bf16(const double *cords, const double *affine, int64_t affine_stride, uint16_t *out, int64_t B, int64_t J,
                        int64_t H, int64_t W, int64_t H0, int64_t W0, double two_sigma_sq, gfla_stream_t stream);
int gfla_pose_cords_f32(const float *maps, int64_t *out, int64_t planes, int64_t H, int64_t W, double threshold,
                        gfla_stream_t stream);
int gfla_pose_cords_f16(const uint16_t *maps, int64_t *out, int64_t planes, int64_t H, int64_t W, double threshold,
                        gfla_stream_t stream);
int gfla_pose_cords_bf16(const uint16_t *maps, int64_t *out, int64_t planes, int64_t H, int64_t W, double threshold,
                         gfla_stream_t stream);
int gfla_normalize_images_f32(const uint8_t *images, float *out, int64_t B, int64_t H, int64_t W, int64_t C,
                              const double *mean, const double *std, gfla_stream_t stream);
int gfla_normalize_images_f16(const uint8_t *images, uint16_t *out, int64_t B, int64_t H, int64_t W, int64_t C,
                              const double *mean, const double *std, gfla_stream_t stream);
int gfla_normalize_images_bf16(const uint8_t *images, uint16_t *out, int64_t B, int64_t H, int64_t W, int64_t C,
                               const double *mean, const double *std, gfla_stream_t stream);

#endif /* GFLA_POSE_H_ */
