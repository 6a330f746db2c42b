/*
 * libffn_hip.so, the parameter update of a training step -- what the google/ffn
 * checkout's model.set_up_optimizer adds to the gradients: the clip of every
 * gradient entry (model.py:127, +-0.7), one of the five update rules that
 * ffn/training/optimizer.py names, and the statistics a step needs to refuse
 * a gradient that is not finite.  The unit knows nothing about tensors, models
 * or the gradients unit: it works on flat arrays of `count` floats.  A driver
 * (ffn_amd/training/trainer.py) lays the model's variables out in one such
 * array and owns the learning-rate schedule and the step counter.
 *
 * Conventions as in ffn_gradients.h: plain C types, 0 / negative FFN_ERR_*
 * return codes, the library's last-error call for the message.  A handle owns
 * one HIP stream and its workspace; calls on one handle must be serialised.
 * Every pointer named *_dev is f32 device memory of the handle's device,
 * dense, 16-byte aligned, and whatever wrote it has completed before the
 * call.  1 <= count < 2^31.  Every call validates on the host first
 * (FFN_ERR_ARG, nothing launched, nothing written) and otherwise returns with
 * its kernels complete.
 *
 * Exact definition of apply.  Per element, in f32, every operation below
 * IEEE-rounded (to nearest even) on its own and in the order written; there is
 * no fused multiply-add anywhere, sqrt and / are the correctly rounded ones,
 * and denormals are kept.  First the clip,
 *   g = grads[i];  if clip > 0:  g < -clip -> -clip,  g > clip -> clip
 * (a NaN stays a NaN, -0 stays -0), then the rule, with p = params[i] and the
 * slots a = slot0[i], b = slot1[i]:
 *   0 sgd       (no slot)          p = p - lr * g
 *   1 momentum  (a, starts at 0)   a = a * c0 + g
 *                                  p = p - a * lr
 *   2 adagrad   (a, starts at 0.1) a = a + g * g
 *                                  p = p - (lr * g) / sqrt(a)
 *   3 adam      (a = m, b = v,     a = a + (g - a) * c0
 *                both start at 0)  b = b + (g * g - b) * c1
 *                                  p = p - (a * lr) / (sqrt(b) + eps)
 *   4 rmsprop   (a = ms, starts    a = a + (g * g - a) * c0
 *                at 1; b = mom,    b = b * c1 + (g * lr) / sqrt(a + eps)
 *                starts at 0)      p = p - b
 * c0, c1: momentum's c0 is the momentum; adam's are 1 - beta1 and 1 - beta2,
 * and its lr is the caller's bias-corrected lr sqrt(1 - beta2^t) / (1 -
 * beta1^t); rmsprop's c0 is 1 - decay and its c1 the momentum.  Arguments a
 * rule does not name are ignored, except the slots: one the rule does not use
 * must be NULL, one it uses must not be.  params and the slots are updated in
 * place, grads is only read.
 *
 * These forms restate the documented Apply* kernels of the TF1 optimizers
 * that optimizer.py constructs.  The claim of this unit is equality, bit for
 * bit, with the table above (tests/optimizer_ref.py restates it in numpy);
 * equality with TensorFlow's own bits is not claimed and has not been tested.
 *
 * grad_stats.  max_abs = the largest |g| over the finite entries (0 if there
 * is none), clipped = the number of finite entries with |g| > clip (0 when
 * clip <= 0), nonfinite = the number of NaN or +-inf entries.  A maximum and
 * integer sums do not depend on the order they are taken in: per-workgroup
 * partials, combined by a second launch.  No float atomics.
 *
 * Exact definition of aggregate: the gradients of n replicas, each clipped,
 * folded in replica order and averaged.  src holds n arrays of `count` floats,
 * `stride` floats apart (array r starts at src + r * stride).  Per element i,
 * in f32, every operation IEEE-rounded (to nearest even) on its own and in the
 * order written; no fused multiply-add, / is the correctly rounded one, and
 * denormals are kept:
 *   c_r = src[r * stride + i];  if clip > 0:  c_r < -clip -> -clip,
 *                                              c_r > clip -> clip
 *   (a NaN stays a NaN, -0 stays -0)
 *   t = c_0
 *   t = t + c_r            for r = 1 .. n - 1, in this order
 *   dst[i] = t / (float)n
 * n = 1 gives dst = clip(src) / 1.0f, which keeps the bits of the clipped
 * value, a -0 included.  The order of the fold is part of the contract: f32
 * addition is not associative, and a caller that gathers replica gradients
 * from several processes gets the same bits whatever dealt the replicas to
 * the processes, as long as it lays them out in replica order
 * (tests/replicas_ref.py restates the fold in numpy).  One launch, no atomics.
 */
#ifndef FFN_OPTIMIZER_H_
#define FFN_OPTIMIZER_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFN_OPTIMIZER_SGD 0
#define FFN_OPTIMIZER_MOMENTUM 1
#define FFN_OPTIMIZER_ADAGRAD 2
#define FFN_OPTIMIZER_ADAM 3
#define FFN_OPTIMIZER_RMSPROP 4

typedef struct ffn_optimizer ffn_optimizer;

int ffn_optimizer_create(int device_id, ffn_optimizer** out);
void ffn_optimizer_destroy(ffn_optimizer* h);

/* max_abs, clipped and nonfinite are HOST values, written on success only. */
int ffn_optimizer_grad_stats(ffn_optimizer* h, int64_t count,
                             const float* grads_dev, float clip,
                             float* max_abs, uint64_t* clipped,
                             uint64_t* nonfinite);

/* The arrays must not overlap one another.  lr must be finite and clip must
 * not be a NaN. */
int ffn_optimizer_apply(ffn_optimizer* h, int rule, int64_t count,
                        float* params_dev, const float* grads_dev,
                        float* slot0_dev, float* slot1_dev, float lr,
                        float clip, float c0, float c1, float eps);

/* 1 <= n <= 256; stride >= count and a multiple of 4 (every array is 16-byte
 * aligned); dst_dev (count floats) must not overlap the (n - 1) * stride +
 * count floats of src_dev; clip must not be a NaN.  src is only read. */
int ffn_optimizer_aggregate(ffn_optimizer* h, int64_t count, int n,
                            const float* src_dev, int64_t stride, float clip,
                            float* dst_dev);

/* HIP-event kernel time of the last grad_stats (index 0) and the last apply
 * (1) on this handle. */
int ffn_optimizer_last_timing(ffn_optimizer* h, double kernel_ms[2]);

/* The third entry of the unit's timing, of the last aggregate.  (A call of
 * its own: last_timing's array of two is what existing callers allocate.) */
int ffn_optimizer_last_timing_aggregate(ffn_optimizer* h, double* kernel_ms);

#ifdef __cplusplus
}
#endif
#endif /* FFN_OPTIMIZER_H_ */
