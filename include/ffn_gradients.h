/*
 * libffn_hip.so, the linear bricks of the conv stack's backward pass -- what a
 * training step of the google/ffn checkout's ConvStack3DFFNModel needs beyond
 * the forward engine: a 3x3x3 SAME conv that keeps its pre-activations, its
 * two gradients, the 1x1x1 logit head with its gradient, and the weighted
 * pixelwise loss with its logit gradient.  A driver (ffn_amd/training/
 * gradients.py) composes them into the whole stack; this unit knows nothing
 * about the engine, the optimizer or train.py.
 *
 * Conventions as in ffn_evaluation.h: plain C types, 0 / negative FFN_ERR_*
 * return codes, the library's last-error call for the message, (z, y, x)
 * order.  A handle owns one HIP stream and its workspace; calls on one handle
 * must be serialised.  Every pointer named *_dev is f32 device memory of the
 * handle's device, dense, and whatever wrote it has completed before the
 * call.  Every call validates its sizes and pointers on the host first
 * (FFN_ERR_ARG, nothing launched, nothing written) and otherwise returns with
 * its kernels complete.
 *
 * Layouts.  Activations and their gradients are channels-last
 * [n][z][y][x][32].  Image, seed, labels, loss weights and logits are
 * [n][z][y][x].  Conv weights are the checkpoint's own [kz][ky][kx][cin][32]
 * with bias [32]; the head's are [32] and [1].  cin is 32, or 2 for conv0_a,
 * whose input is two planes (image, then seed: convstack_3d.py:86).  1 <= n
 * <= FFN_GRADIENTS_MAX_BATCH, every side >= 1, n z y x < 2^26.  Borders are
 * SAME: a tap outside the FoV contributes zero and is never read.
 *
 * Exact definition.  With t = (kz, ky, kx) in 0..2 and p + t the voxel at
 * offset t - 1 from p:
 *   forward            y(p)[co] = b[co] + sum_t sum_ci in(p + t)[ci] W[t][ci][co]
 *                      (+ skip(p)[co]), in = x or max(x, 0); no ReLU follows
 *   backward to input  dx(p)[ci] = sum_t sum_co dy(p - t)[co] W[t][ci][co],
 *                      then * (pre(p)[ci] > 0) if pre is given, then + the
 *                      old dx(p)[ci] if accumulate
 *   backward to weights dW[t][ci][co] = sum_n,p in(p + t)[ci] dy(p)[co],
 *                      db[co] = sum_n,p dy(p)[co]
 *   head               logits(p) = seed(p) + b + sum_c max(net(p)[c], 0) w[c]
 *   head backward      dnet(p)[c] = (net(p)[c] > 0) ? dlogits(p) w[c] : 0,
 *                      dw[c] = sum_p dlogits(p) max(net(p)[c], 0),
 *                      db = sum_p dlogits(p)
 *   loss               mean over the N = n z y x voxels of
 *                      w (max(x, 0) - x z + log1p(exp(-|x|))), x the logit and
 *                      z the label; dlogits = w (sigmoid(x) - z) / N
 * All arithmetic is f32: v_mfma_f32_16x16x4_f32 (an f32 fmaf chain) for the
 * three 32-channel contractions, plain fmaf elsewhere.  No float atomics: the
 * sums over positions are taken per workgroup over a slice of one batch item's
 * positions that depends on (z, y, x) only, written as partials, and added in
 * index order by a second launch.  Equal inputs give equal bits on every run,
 * and an item's terms are summed in the same order whatever else the batch
 * holds.
 */
#ifndef FFN_GRADIENTS_H_
#define FFN_GRADIENTS_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFN_GRADIENTS_MAX_BATCH 32
#define FFN_GRADIENTS_FEATURES 32

typedef struct ffn_gradients ffn_gradients;

int ffn_gradients_create(int device_id, ffn_gradients** out);
void ffn_gradients_destroy(ffn_gradients* h);

/* cin 32: x_dev is [n][z][y][x][32] and x2_dev is ignored.  cin 2: x_dev is the
 * image plane and x2_dev the seed plane, both [n][z][y][x].  skip_dev may be
 * NULL; y_dev must not overlap x_dev. */
int ffn_gradients_conv_forward(ffn_gradients* h, int n,
                               const int32_t shape_zyx[3], int cin,
                               const float* x_dev, const float* x2_dev,
                               int relu_in, const float* w_dev,
                               const float* b_dev, const float* skip_dev,
                               float* y_dev);

/* cin = 32 only.  pre_dev may be NULL (no mask).  With accumulate != 0 the
 * result is added to what dx_dev holds.  dx_dev must not overlap dy_dev. */
int ffn_gradients_conv_backward_input(ffn_gradients* h, int n,
                                      const int32_t shape_zyx[3],
                                      const float* dy_dev, const float* w_dev,
                                      const float* pre_dev, int accumulate,
                                      float* dx_dev);

/* x_dev / x2_dev / relu_in as in the forward call.  dw_dev: [27][cin][32],
 * db_dev: [32]; both are overwritten. */
int ffn_gradients_conv_backward_weights(ffn_gradients* h, int n,
                                        const int32_t shape_zyx[3], int cin,
                                        const float* x_dev, const float* x2_dev,
                                        int relu_in, const float* dy_dev,
                                        float* dw_dev, float* db_dev);

int ffn_gradients_head_forward(ffn_gradients* h, int n,
                               const int32_t shape_zyx[3], const float* net_dev,
                               const float* seed_dev, const float* w_dev,
                               const float* b_dev, float* logits_dev);

/* dnet_dev: [n][z][y][x][32], dw_dev: [32], db_dev: [1]; all overwritten. */
int ffn_gradients_head_backward(ffn_gradients* h, int n,
                                const int32_t shape_zyx[3],
                                const float* net_dev, const float* dlogits_dev,
                                const float* w_dev, float* dnet_dev,
                                float* dw_dev, float* db_dev);

/* *loss is a HOST float.  dlogits_dev may be NULL (loss only). */
int ffn_gradients_loss(ffn_gradients* h, int n, const int32_t shape_zyx[3],
                       const float* logits_dev, const float* labels_dev,
                       const float* weights_dev, float* loss,
                       float* dlogits_dev);

/* HIP-event kernel time of the last conv_forward (index 0), conv_backward_input
 * (1), conv_backward_weights (2), head_forward (3), head_backward (4) and loss
 * (5) on this handle. */
int ffn_gradients_last_timing(ffn_gradients* h, double kernel_ms[6]);

#ifdef __cplusplus
}
#endif
#endif /* FFN_GRADIENTS_H_ */
