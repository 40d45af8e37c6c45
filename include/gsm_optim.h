/*
 * gsm_optim.h — C ABI of libgsm.so, the optimizer step: the global-norm
 * gradient clip and one Adam update of a list of tensors in one launch pair.
 * A header of its own beside gsm.h (whose rules, status codes and
 * gsm_last_error it shares; GSM_ABI_VERSION does not count these entry
 * points); the in-tree binding is _lib.OPTIM_SIGNATURES.
 */
#ifndef GSM_OPTIM_H_
#define GSM_OPTIM_H_

#include "gsm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The step after loss.backward(): what torch.nn.utils.clip_grad_norm_(params,
 * max_norm) followed by torch.optim.Adam(lr, betas, eps).step() computes, with
 * two deliberate differences (below). p, g, m, v: HOST arrays of n_tensors
 * device pointers (parameter, gradient, first and second moment, each f32 [n[i]],
 * contiguous); n: host int64 [n_tensors], each in [0, 2^31); a tensor of 0
 * elements is skipped (its pointers may be NULL). The arrays are read before
 * the call returns; any n_tensors >= 0. lr: device f32 [1] and step: device
 * int32 [1] (the number of updates so far), both read when the kernels run (a
 * captured graph sees a schedule that rewrites lr in place). With t = step[0]:
 *   norm = sqrt(sum of g^2 over every element of every tensor)
 *          the squares and their sum in fp64 (a float's square is exact there
 *          and cannot overflow), the root in fp64, rounded to fp32 once
 *   coef = min(1, max_norm / (norm + 1e-6f))       in fp32; max_norm = INFINITY:
 *          no clip. norm + 1e-6f <= max_norm gives exactly 1.0f, g * coef == g
 *   norm not finite (a NaN or an Inf in a gradient): the update is SKIPPED: no
 *          bit of any p, m, v or of the step word changes, GSM_OPT_NONFINITE is
 *          OR-ed into status and stats[3] = 1 (torch's clip, with its default
 *          error_if_nonfinite=False, goes on and overwrites every parameter with
 *          NaN: the first deliberate difference)
 *   otherwise t <- t + 1, g' = g * coef and, every line one correctly rounded
 *   fp32 operation at a time:
 *     m <- beta1 * m + (1 - beta1) * g'
 *     v <- beta2 * v + (1 - beta2) * (g' * g')
 *     p <- p - step_size * (m / (sqrtf(v) / bc2_sqrt + eps))
 *   beta1, beta2, 1 - beta1, 1 - beta2 and eps: the doubles rounded once to
 *   fp32; step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) formed
 *   in fp64 (the powers by squaring) and rounded once. No weight decay, no
 *   amsgrad. The gradients are inputs: g is never written, the clip is applied
 *   on the fly (torch rescales .grad in place: the second deliberate difference).
 * stats f32 [4]: norm, coef (0 when skipped), the step count after the call,
 * skipped (0 / 1). status: device int32 [1], OR-ed, zeroed by the caller; NULL:
 * not wanted. A call on no elements at all still counts as an update (norm 0).
 * work: device f32, gsm_adam_work_floats of them, 8-BYTE ALIGNED (it holds
 * doubles): a 16-byte header, then one fp64 partial per chunk of 1024 elements.
 * Pass 1: a workgroup adds a chunk's squares (a thread four consecutive
 * elements, the 64 lanes of a wave, the four waves, in a fixed order) and
 * writes its partial; workgroup 0 copies t + 1 into the header. Pass 2: every
 * workgroup adds all partials in one fixed order, forms norm, coef, the skip
 * decision and the bias corrections, and updates its chunks; workgroup 0 alone
 * writes stats, status and, when not skipped, the step word, which pass 2
 * never reads. No float atomics: two calls on the same state give the same bits
 * (also whatever the tensors' alignment: 16-byte accesses when p, g, m and v of
 * a tensor are all 16-byte aligned, scalar accesses to the same elements in the
 * same order otherwise). The tensors' pointers go by value in the kernel
 * arguments, 32 tensors a launch: up to 32 tensors are two launches, n_tensors
 * of them 2 * ceil(n_tensors / 32), all on `stream` in order. No device table,
 * no copy, no allocation, no synchronisation: the call can be captured, as long
 * as the pointers it was captured with stay valid.
 * Limits (GSM_EINVAL, checked first, nothing is launched): n_tensors >= 0, every
 * n[i] in [0, 2^31), a NULL pointer of a tensor with n[i] > 0, beta1 and beta2
 * in [0, 1), eps >= 0, max_norm >= 0 (not NaN), lr, step, work or stats NULL,
 * work not 8-byte aligned. Stateless; asynchronous on `stream`. */
#define GSM_OPT_NONFINITE 1   /* status: a non-finite gradient norm, the update skipped */
int gsm_adam_work_floats(int64_t n_tensors, int64_t total_elements, int64_t *n_floats);
int gsm_adam_step(float *const *p, const float *const *g, float *const *m, float *const *v, const int64_t *n,
                  int64_t n_tensors, const float *lr, int32_t *step, double beta1, double beta2, double eps,
                  float max_norm, float *work, float *stats, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSM_OPTIM_H_ */
