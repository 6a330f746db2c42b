"""The gradient oracle itself (tests/gradients_ref.py), without a GPU: autograd
against central finite differences, the single-conv helper against the whole
stack's definition, and the rule that the product path has no CPU fallback."""
import numpy as np
import pytest
import torch

from tests import gradients_ref as ref


@pytest.fixture(scope='module')
def small_case():
  depth, n, zyx = 2, 2, (3, 4, 5)
  variables = ref.random_variables(depth, seed=3, stddev=0.2)
  seed, image, labels, weights = ref.training_inputs(n, zyx, seed=5)
  weights = np.random.RandomState(6).uniform(0, 2, weights.shape).astype(
      np.float32)
  base = ref.run(variables, depth, seed, image, labels, weights)
  return depth, variables, (seed, image, labels, weights), base


def test_autograd_agrees_with_central_differences(small_case):
  """40 randomly chosen weights of a depth-2, 3x4x5, batch-2 model in f64, to
  a relative 1e-6 of the tensor's largest gradient entry.  The masks of the
  base run are held fixed, so the loss is smooth in the weights.  Step 1e-4:
  truncation ~ step^2 * f''' / 6 = 2e-9 * f''', round-off ~ 1e-16 / step =
  1e-12, both far below 1e-6 of gradients of order 1e-2."""
  depth, variables, inputs, base = small_case
  masks = [p > 0 for p in base['pre']]
  fixed = ref.run(variables, depth, *inputs, masks=masks)
  assert fixed['loss'] == base['loss']
  rng = np.random.RandomState(11)
  names = sorted(variables)
  step = 1e-4
  worst = 0.0
  for _ in range(40):
    name = names[rng.randint(len(names))]
    index = tuple(rng.randint(s) for s in variables[name].shape)
    losses = []
    for sign in (+1, -1):
      moved = {k: np.asarray(a, dtype=np.float64).copy()
               for k, a in variables.items()}
      moved[name][index] += sign * step
      losses.append(ref.run(moved, depth, *inputs, masks=masks,
                            want_grads=False)['loss'])
    numeric = (losses[0] - losses[1]) / (2 * step)
    g = fixed['grads'][name]
    err = abs(numeric - g[index]) / np.max(np.abs(g))
    worst = max(worst, err)
    assert err <= 1e-6, (name, index, numeric, g[index])
  print('largest relative difference: %.3g' % worst)


def test_masks_default_to_the_sign_of_the_pre_activation(small_case):
  depth, variables, inputs, base = small_case
  assert len(base['pre']) == 2 * depth
  assert all(p.shape == inputs[0].shape + (32,) for p in base['pre'])
  flipped = [np.zeros_like(p, dtype=bool) for p in base['pre']]
  dead = ref.run(variables, depth, *inputs, masks=flipped)
  # every ReLU closed: only the biases of the last conv see the loss
  assert np.all(dead['grads']['seed_update/conv0_a/weights'] == 0)
  assert np.any(dead['grads']['seed_update/conv_lom/biases'] != 0)


def test_conv_case_is_the_definition():
  """dW[t][ci][co] = sum_p in(p + t)[ci] dy(p)[co] and the flipped, transposed
  kernel for dx, restated with explicit loops on a tiny case."""
  rng = np.random.RandomState(2)
  n, z, y, x, cin, cout = 1, 2, 3, 4, 2, 32
  xs = rng.normal(size=(n, z, y, x, cin))
  w = rng.normal(size=(3, 3, 3, cin, cout))
  b = rng.normal(size=(cout,))
  dy = rng.normal(size=(n, z, y, x, cout))
  yv, dx, dw, db = ref.conv_case(xs, w, b, dy)
  pad = np.pad(xs, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))
  want_y = np.zeros_like(dy) + b
  want_dw = np.zeros_like(w)
  for kz in range(3):
    for ky in range(3):
      for kx in range(3):
        win = pad[:, kz:kz + z, ky:ky + y, kx:kx + x]
        want_y += win @ w[kz, ky, kx]
        want_dw[kz, ky, kx] = np.einsum('nzyxi,nzyxo->io', win, dy)
  np.testing.assert_allclose(yv, want_y, rtol=0, atol=1e-12)
  np.testing.assert_allclose(dw, want_dw, rtol=0, atol=1e-12)
  np.testing.assert_allclose(db, dy.sum(axis=(0, 1, 2, 3)), rtol=0, atol=1e-12)
  dpad = np.pad(dy, ((0, 0), (1, 1), (1, 1), (1, 1), (0, 0)))
  want_dx = np.zeros_like(xs)
  for kz in range(3):
    for ky in range(3):
      for kx in range(3):
        win = dpad[:, 2 - kz:2 - kz + z, 2 - ky:2 - ky + y, 2 - kx:2 - kx + x]
        want_dx += win @ w[kz, ky, kx].T
  np.testing.assert_allclose(dx, want_dx, rtol=0, atol=1e-12)


def test_no_cpu_fallback_without_gpu():
  """Without a GPU the constructors raise; nothing routes to torch."""
  if torch.cuda.is_available():
    pytest.skip('GPU present')
  from ffn_amd import _lib
  from ffn_amd.training import gradients
  from ffn_amd.training.models import convstack_3d
  with pytest.raises(_lib.FFNHipError):
    gradients.GradientOps(0)
  model = convstack_3d.ConvStack3DFFNModel(fov_size=[5, 5, 5], deltas=[1, 1, 1],
                                           depth=2)
  model.init_random()
  with pytest.raises(_lib.FFNHipError):
    gradients.ConvStackGradients(model, 1, 0)
