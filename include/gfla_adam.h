/* Part of gfla_hip.h (which includes this file inside its extern "C" block: include that one), in the same dialect; the
 * ctypes binding reads both.
 *
 * ---- one Adam / AdamW step over all parameters of a group (torch.optim.Adam's _single_tensor_adam; csrc/adam.hip) -------
 * The suffix is the storage type of parameter and gradient; moments and master copies are float32.  All arithmetic is
 * float32 per element, without contraction, in torch's order; with t = *step + 1:
 *   bc1 = 1 - beta1^t, bc2 = 1 - beta2^t               in double, once per workgroup
 *   g' = g * (1 / *grad_scale)                         when grad_scale is given; the reciprocal rounded to float32 once
 *   g' += wd * p                                       L2 decay (flags bit 0 clear, wd != 0)
 *   p  *= 1 - lr * wd                                  decoupled decay (flags bit 0 set: AdamW)
 *   m  += (g' - m) * (1 - beta1)                       beta1 == 0: m is not read, m = g' is stored
 *   v   = beta2 * v + ((1 - beta2) * g') * g'
 *   p  += (-(lr / bc1) * m) / (sqrt(v) / sqrt(bc2) + eps)
 * A record with a master copy reads p from the master, writes the master, and stores the master rounded to nearest even
 * as the parameter.  Gradients are left as stored: not unscaled in memory, not zeroed.  A non-finite gradient element
 * poisons its own p, m, v and master element and no other.
 *
 * `table`: n records of 8 int64 on the device:
 *   [0] address of the parameter   [1] address of its gradient; 0: no gradient this step, nothing of the tensor is touched
 *   [2] address of exp_avg   [3] address of exp_avg_sq   (float32)
 *   [4] address of the float32 master copy, 0 for none (float32 parameters)
 *   [5] numel   [6] index of the tensor's first work chunk: sum of ceil(numel_j / chunk) over j < i   [7] 0
 * gfla_adam_chunk_elems: the elements one workgroup processes, a constant of the build.
 * gfla_adam_layout (host only): writes [6] for every tensor into first_chunk (n) and the chunk count into totals[0].
 * gfla_adam_vector_path (host only): 1 if a tensor with these addresses takes the 16-byte path -- every address a
 *   multiple of 16 (a master of 0 counts as one), elem_size 2 or 4 --, 0 if it takes the element path, which handles any
 *   2-byte (16-bit storage) or 4-byte phase of p and g.  The kernel decides per tensor with the same inline function.
 * `numels`: n int64 in HOST memory, the same numbers as [5], for the argument checks and the grid; the device table is
 *   never read by the host.
 * `step`: one device float, the steps taken so far.  `grad_scale`, `found_inf`: device floats or NULL.  With found_inf
 *   given and nonzero no workgroup stores anything and *step stays; otherwise *step becomes t, in a one-wave launch after
 *   the main one, so that no workgroup reads what another of its launch writes.  Two launches per call, whatever n is.
 * No atomics, element-wise: results are bit-identical from call to call, and a tensor gives the same bits alone as in a
 * batch.
 * NULL table, numels or step (layout: numels, first_chunk or totals) -> -1; n <= 0, a numel <= 0, lr < 0, eps <= 0, a beta
 * outside [0, 1), weight_decay < 0 (or any of these NaN), flag bits other than bit 0 -> -2; n > 65535, a numel > 2^31 - 1
 * or more than 2^24 - 1 chunks in all -> GFLA_ERR_UNSUPPORTED.  All decided before anything touches the device.
 * Additive: GFLA_ABI_VERSION stays 8. */
#ifndef GFLA_ADAM_H_
#define GFLA_ADAM_H_

int64_t gfla_adam_chunk_elems(void);
int gfla_adam_layout(const int64_t *numels, int64_t n, int64_t *first_chunk, int64_t *totals);
int gfla_adam_vector_path(int64_t p, int64_t g, int64_t m, int64_t v, int64_t master, int elem_size);
int gfla_adam_step_f32(const void *table, const int64_t *numels, int64_t n, float *step, const float *grad_scale,
                       const float *found_inf, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int flags, gfla_stream_t stream);
int gfla_adam_step_f16(const void *table, const int64_t *numels, int64_t n, float *step, const float *grad_scale,
                       const float *found_inf, double lr, double beta1, double beta2, double eps, double weight_decay,
                       int flags, gfla_stream_t stream);
int gfla_adam_step_bf16(const void *table, const int64_t *numels, int64_t n, float *step, const float *grad_scale,
                        const float *found_inf, double lr, double beta1, double beta2, double eps, double weight_decay,
                        int flags, gfla_stream_t stream);

#endif /* GFLA_ADAM_H_ */
