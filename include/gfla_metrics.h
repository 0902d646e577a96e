/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- reconstruction metrics on the device: generator output -> bytes, and SSIM / PSNR / L1 / MAE of byte images
 * (csrc/recon_metrics.hip) ---------------------------------------------------------------------------------------------
 * gfla_images_to_uint8_*: `x` (B, C, H, W) in the suffix's storage type -> `out` (B, H, W, C) uint8, every byte written.
 *   16-bit storage is widened exactly first.  In float32 without contraction, each operation rounded:
 *     t = ((x + 1) / 2) * bytes            (`bytes` rounded to float32 first)
 *     byte = (uint8)t, truncated toward zero, for 0 <= t < 256; 0 for t < 0 and for NaN; 255 for t >= 256.
 * gfla_recon_metrics: `pred`, `gt` (B, H, W, C) uint8, C in 1..4 -> `out` (5, B) double, rows ssim, ssim_256, psnr, l1,
 *   mae; bit 0 of `flags` asks for ssim, bit 1 for ssim_256, bit 2 for psnr, l1 and mae together.  Rows that were not
 *   asked for are not written.  Per image pair, with x a byte of gt and y the byte of pred at the same place:
 *     a = (double)((float)x / 255.f), b likewise of y; d = a - b, which is exact in double.  Over all n = H W C values
 *     psnr = 10 log10(1 / (sum d d / n)), l1 = (sum |d|) / n, mae = (sum |d|) / (sum (a + b)): +inf for equal images,
 *     NaN (0 / 0) for two black ones.  The sums are double sums in an order that depends on H W C alone.
 *   ssim: per channel and per position whose win_size x win_size window lies inside the image, from the window's exact
 *     integer sums Sx, Sy, Sxx, Syy, Sxy (N = win_size^2 values each; 32 bits hold them for win_size <= 255):
 *       nxx = N Sxx - Sx Sx, nyy = N Syy - Sy Sy, nxy = N Sxy - Sx Sy  (64-bit integers, exact as doubles)
 *       c1 = C1 N N, c2 = C2 N (N - 1), C1 = (0.01 * 255) (0.01 * 255), C2 = (0.03 * 255) (0.03 * 255)
 *       S = ((2 Sx Sy + c1) (2 nxy + c2)) / ((Sx Sx + Sy Sy + c1) (nxx + nyy + c2))
 *     which is ((2 ux uy + C1) (2 vxy + C2)) / ((ux ux + uy uy + C1) (vx + vy + C2)) of the means ux = Sx / N and the sample
 *     covariances vx = nxx / (N (N - 1)), with numerator and denominator multiplied through: one division, one rounding
 *     each in c1, c2, the four sums and the two products.
 *     the mean of S over the positions of a channel, then the mean over channels: the structural similarity with a uniform
 *     window, sample covariance and data range 1 of the images / 255, evaluated on the 0..255 scale.
 *   ssim_256: the same with Gaussian weights, `taps` (GFLA_METRICS_TAPS doubles in HOST memory, one axis; the window is
 *     their outer product), population covariance and R = max(pred) - min(pred) over the whole image, all channels:
 *       column sums first, taps in order: m = t[0] v[0]; m = m + t[i] v[i] for i = 1 .. 10, for v the values x, y, x x, y y,
 *       x y of the 11 rows (exact integers as doubles); then the same over the 11 columns' m: ux, uy, uxx, uyy, uxy
 *       vx = uxx - ux ux, vy = uyy - uy uy, vxy = uxy - ux uy; C1 = (0.01 R) (0.01 R), C2 = (0.03 R) (0.03 R);
 *       S = ((2 ux uy + C1) (2 vxy + C2)) / ((ux ux + uy uy + C1) (vx + vy + C2)), sums and products left to right.
 *     No contraction anywhere, and no special case: a constant prediction gives R = 0 and whatever IEEE makes of S.
 *   Sums of S: each workgroup adds its positions in a fixed order into one double of `workspace`; a last launch adds those
 *   per image in a fixed order.  No atomics: an image's numbers are the same bits in every call, at every position of
 *   every batch.  `workspace`: gfla_recon_metrics_workspace_bytes(B, H, W, C, win_size, flags) bytes, 8-byte aligned,
 *   uninitialised.  Nothing is read back.
 * gfla_recon_metrics_geometry: out[0], out[1] = output columns and output rows per workgroup of the uniform-window kernel
 *   at `win_size`, out[2], out[3] = those of the Gaussian kernel, out[4] = bytes per workgroup of the pixel-sum kernel.
 * pred, gt, out of images_to_uint8: any byte address; x: any multiple of its element size; out of recon_metrics: 8-byte
 * aligned.  Images are not padded.
 * NULL x / out / pred / gt / workspace, NULL taps with bit 1 set -> -1; B, C, H, W <= 0, C > 4 for the metrics, a bytes
 * that is not finite in float32, flags outside 1..7, an even win_size or one outside 3..255 with bit 0 set, an image
 * smaller than a window that was asked for (win_size, or GFLA_METRICS_TAPS with bit 1 set) -> -2; C > 4 for
 * images_to_uint8, H or W > 32768, more than 2^31 - 1 values per image or workgroups per launch, B > 65535 for the
 * metrics -> GFLA_ERR_UNSUPPORTED.  All decided before anything is launched; gfla_recon_metrics_workspace_bytes returns
 * the same codes.
 * Additive: GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_METRICS_H_
#define GFLA_METRICS_H_

#define GFLA_METRICS_TAPS 11

int gfla_images_to_uint8_f32(const float *x, uint8_t *out, int64_t B, int64_t C, int64_t H, int64_t W, double bytes,
                             gfla_stream_t stream);
int gfla_images_to_uint8_f16(const uint16_t *x, uint8_t *out, int64_t B, int64_t C, int64_t H, int64_t W, double bytes,
                             gfla_stream_t stream);
int gfla_images_to_uint8_bf16(const uint16_t *x, uint8_t *out, int64_t B, int64_t C, int64_t H, int64_t W, double bytes,
                              gfla_stream_t stream);
int64_t gfla_recon_metrics_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int64_t win_size, int flags);
int gfla_recon_metrics(const uint8_t *pred, const uint8_t *gt, double *out, void *workspace, int64_t B, int64_t H, int64_t W,
                       int64_t C, int64_t win_size, int flags, const double *taps, gfla_stream_t stream);
int gfla_recon_metrics_geometry(int64_t win_size, int64_t *out);

#endif /* GFLA_METRICS_H_ */
