/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- spectral normalisation of a batch of weight matrices (torch.nn.utils.spectral_norm's compute_weight;
 * csrc/spectral_norm.hip) ---------------------------------------------------------------------------------------------
 * Float32 only.  Matrix i of the batch is a convolution weight (Cout,Cin,kh,kw) read as stored: R_i x K_i row-major with
 * R = Cout, K = Cin kh kw, with its vectors u_i (R) and v_i (K).  For every matrix, in one call:
 *   repeat power_iterations times:   t = W^T u;  v = t / max(||t||_2, eps)
 *                                    s = W v;    u = s / max(||s||_2, eps)
 *   sigma = u . (W v)                W_sn = W / sigma        (a true division)
 * u and v are updated in place; power_iterations = 0 (eval mode) leaves them untouched and still gives sigma and W_sn.
 *
 * `table`: n records of 8 int64 on the device, built by the caller once per set of matrices:
 *   [0] address of W_i   [1] address of u_i   [2] address of v_i   (float32, contiguous; all three distinct buffers)
 *   [3] R_i   [4] K_i
 *   [5] element offset of matrix i in the flat arrays w_sn / grad_sn / grad_w: sum of R_j K_j over j < i
 *   [6] offset of the K_i-vector of matrix i in the vector arrays:             sum of (R_j + K_j) over j < i
 *   [7] offset of the R_i-vector of matrix i in the vector arrays:             [6] + K_i
 * gfla_spectral_norm_layout (host only) writes [5], [6], [7] for every matrix into offsets (n x 3) and the lengths of the
 * flat arrays and of the vector arrays into totals[0], totals[1].
 * `dims`: n x 2 int64 in HOST memory, (R_i, K_i): the same numbers as the table's, for the argument checks and the launch
 * geometry; the device table is never read by the host.
 * gfla_spectral_norm_fwd_f32: w_sn (totals[0] floats) receives every W_sn,i at its element offset, sigma (n floats) every
 *   sigma_i.  saved (totals[1] floats, or NULL): the v_i and u_i the result was computed with, at offsets [6] and [7] --
 *   what the backward needs after a later forward has moved the buffers on.  scratch: totals[1] floats, uninitialised.
 *   Launches: 2 power_iterations + 1 (2 with power_iterations = 0), whatever n is: per iteration column sums over
 *   (matrix, 64 columns) and row dots over (matrix, 4 rows) -- the last row dots are the W v of sigma --, then a
 *   finalise-and-scale pass over (matrix, 4096 elements).  A workgroup recomputes the norm it needs from the t / s vector
 *   of its matrix; u and v are written by one workgroup per matrix in launches in which no workgroup reads them.
 * gfla_spectral_norm_bwd_f32: with u, v (from `saved`) and sigma constants, as in torch (the iteration runs under no_grad),
 *   and G_i = grad_sn at the element offset:
 *     c_i = <G_i, W_i> / sigma_i        grad_w_i = (G_i - c_i u_i v_i^T) / sigma_i
 *   scratch: gfla_spectral_norm_bwd_scratch_floats(dims, n) floats, uninitialised.  Two launches.
 * No atomics: every sum has an order fixed by (R_i, K_i) alone, so results are bit-identical from call to call and a
 * matrix gives the same bits alone as in a batch.
 * NULL table, dims or outputs (offsets / totals; w_sn / sigma / scratch; grad_sn / saved / grad_w) -> -1; n <= 0, a
 * non-positive R or K, power_iterations < 0, eps <= 0 -> -2; n > 65535, R or K > 2^24, R K > 2^31 - 1 ->
 * GFLA_ERR_UNSUPPORTED, nothing is launched.  Additive: GFLA_ABI_VERSION stays 8.
 *
 * ---- matrices that are not their storage: the gfla_spectral_norm_mixed_* entry points ------------------------------------
 * torch normalises an nn.ConvTranspose2d along dim 1: the matrix of a weight stored (Cin, Cout, kh, kw) is
 * weight.permute(1,0,2,3).reshape(Cout, Cin kh kw).  With inner = kh kw it has R = Cout rows and K = Cin inner columns, and
 * element (r, c) is at ((c / inner) R + r) inner + c % inner of the storage.  The mixed entry points take such matrices
 * ("dim 1") and matrices read as stored ("dim 0") in one batch, with the arithmetic above on every one of them:
 *   `dims`:  n x 3 int64 in HOST memory, (R_i, K_i, inner_i); inner_i = 0: dim 0, as stored; inner_i >= 1: dim 1.
 *   `table`: n records of 9 int64: [0] .. [7] as above, [8] = inner_i.  u_i keeps R_i entries and v_i K_i entries, in the
 *            matrix's own order (v: column c = ci inner + tap), so they are the buffers of torch's hook.
 *   w_sn, grad_sn and grad_w hold matrix i at its element offset IN THE WEIGHT'S STORAGE LAYOUT: W_sn,i is the tensor a
 *   transposed convolution takes as it is, and its weight gradient enters as it is.  No permuted copy exists anywhere.
 * Layout, `saved`, the backward's scratch, status codes and limits as above; in addition a negative inner or a K that is
 * no multiple of inner -> -2, inner > 25 -> GFLA_ERR_UNSUPPORTED.  scratch of gfla_spectral_norm_mixed_fwd_f32:
 * 3 totals[1] + 2 floats, uninitialised (the float32 vector arrays, and behind them, at the next multiple of 8 bytes, the
 * same vectors in float64 for the dim-1 matrices).
 * Launches: the same as above whatever the batch holds -- 2 power_iterations + 1 forward (2 with power_iterations = 0),
 * 2 backward; a workgroup takes the branch of its matrix.  Every pass of a dim-1 matrix reads the weight in storage
 * order, consecutive lanes at consecutive addresses: the column sums take one slab W[ci] (R inner contiguous floats) per
 * workgroup, each thread adding into its own LDS bin per tap, a wave then adding a tap's 256 bins in a fixed order; the
 * row dots take max(1, 64 / inner) rows per workgroup, whose floats are one contiguous run in every slab, one lane per
 * float, the four waves a quarter of the slabs each; the scale pass and <G, W> are element-wise; grad_w maps a storage
 * offset back to (r, c).  The sums of a dim-1 matrix's forward are float64 on the float32 weight -- bins and per-row sums
 * are serial where the dim-0 passes have a butterfly, and sigma = u . (W v) cancels on fresh buffers --: t, s and both
 * norms stay float64 between the launches, u, v and sigma are each rounded to float32 once.  The order of every sum is fixed by (R, K, inner) alone: bit-identical from call to call and for
 * a matrix alone or in any batch, and a dim-0 matrix gives the bits the dim-0 entry points give (which run the same
 * kernels on 8-word records).  u and v are written by one workgroup per matrix in launches in which nobody reads them. */
#ifndef GFLA_SPECTRAL_NORM_H_
#define GFLA_SPECTRAL_NORM_H_

int gfla_spectral_norm_layout(const int64_t *dims, int64_t n, int64_t *offsets, int64_t *totals);
int64_t gfla_spectral_norm_bwd_scratch_floats(const int64_t *dims, int64_t n);
int gfla_spectral_norm_fwd_f32(const void *table, const int64_t *dims, int64_t n, float *w_sn, float *sigma, float *saved,
                               float *scratch, int power_iterations, double eps, gfla_stream_t stream);
int gfla_spectral_norm_bwd_f32(const void *table, const int64_t *dims, int64_t n, const float *grad_sn, const float *saved,
                               const float *sigma, float *grad_w, float *scratch, gfla_stream_t stream);
int gfla_spectral_norm_mixed_layout(const int64_t *dims, int64_t n, int64_t *offsets, int64_t *totals);
int64_t gfla_spectral_norm_mixed_bwd_scratch_floats(const int64_t *dims, int64_t n);
int gfla_spectral_norm_mixed_fwd_f32(const void *table, const int64_t *dims, int64_t n, float *w_sn, float *sigma,
                                     float *saved, float *scratch, int power_iterations, double eps, gfla_stream_t stream);
int gfla_spectral_norm_mixed_bwd_f32(const void *table, const int64_t *dims, int64_t n, const float *grad_sn,
                                     const float *saved, const float *sigma, float *grad_w, float *scratch,
                                     gfla_stream_t stream);

#endif /* GFLA_SPECTRAL_NORM_H_ */
