"""The gradients unit on the GPU (include/ffn_gradients.h,
ffn_amd/training/gradients.py) against the torch f64 oracle
(tests/gradients_ref.py).

Yardstick.  E(g) = max |g - g_f64| / max |g_f64|; E_ref is E of the oracle's
own f32 run on the same inputs (and the same ReLU masks); a GPU result passes
when E_gpu <= 4 E_ref, the factor covering the different summation order and
shape.  Every test prints both figures; the largest are in DESIGN.md 10.5.

The whole-stack tests hand the GPU's own ReLU masks to both oracle runs and
check the masks separately (pre-activations within 1e-4 of the f64 run's, sign
flips only where |pre_f64| is below the measured distance and on at most
0.01 % of the inputs): a comparison of two independent forward passes would
trip over the ReLU kink.

Exact cases.  The per-conv ops are plain f32, so on integer operands (x, dy, skip
in [-3, 3], w, b in [-2, 2]) every partial sum in any order is an integer far
below 2^24 -- y and dx sum 864 terms of at most 6 (+ bias and skip), dW at most
2 * 9 * 11 * 13 = 2574 positions of at most 9, below 2^15 -- and the result must
be the f64 oracle's bit for bit: no yardstick, np.array_equal.  The loss and the
whole stack stay on the yardstick (sigmoid and log are not exact).
"""
import ctypes

import numpy as np
import pytest

from tests import gradients_ref as ref

pytestmark = pytest.mark.gpu

FACTOR = 4.0
SHAPES = [(2, 9, 11, 13), (1, 5, 7, 70), (3, 1, 1, 1)]
ERR_ARG = -1


@pytest.fixture(scope='module')
def torch():
  import torch as torch_module
  return torch_module


@pytest.fixture(scope='module')
def gr():
  from ffn_amd.training import gradients
  return gradients


@pytest.fixture(scope='module')
def ops(gr):
  return gr.default_ops(0)


@pytest.fixture(scope='module')
def dev(torch):
  def to_device(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to('cuda:0')
    torch.cuda.synchronize()
    return t
  return to_device


def host(t):
  return t.cpu().numpy()


def yardstick(label, got, want64, want32):
  e_gpu, e_ref = ref.spread(got, want64), ref.spread(want32, want64)
  print('%-44s E_gpu %.3g  E_ref %.3g' % (label, e_gpu, e_ref))
  assert np.all(np.isfinite(got)), label
  assert e_gpu <= FACTOR * e_ref, (label, e_gpu, e_ref)
  return e_gpu, e_ref


def conv_inputs(shape, cin, seed):
  """x (or the two planes), w, b, dy, skip of one conv; the weights have the
  scale of a trained checkpoint's (std 0.05)."""
  rng = np.random.RandomState(seed)
  act = shape + (32,)
  if cin == 2:
    x = (rng.normal(0, 1, shape).astype(np.float32),
         rng.normal(-2, 1, shape).astype(np.float32))
  else:
    x = rng.normal(0, 1, act).astype(np.float32)
  w = rng.normal(0, 0.05, (3, 3, 3, cin, 32)).astype(np.float32)
  b = rng.normal(0, 0.05, (32,)).astype(np.float32)
  dy = rng.normal(0, 1, act).astype(np.float32)
  skip = rng.normal(0, 1, act).astype(np.float32)
  return x, w, b, dy, skip


def exact_conv_inputs(shape, cin, seed):
  """conv_inputs with integers: x, dy, skip in [-3, 3], w, b in [-2, 2]"""
  rng = np.random.RandomState(seed)
  act = shape + (32,)
  ints = lambda lo, hi, size: rng.randint(lo, hi + 1, size).astype(np.float32)
  x = (ints(-3, 3, shape), ints(-3, 3, shape)) if cin == 2 else ints(-3, 3, act)
  return (x, ints(-2, 2, (3, 3, 3, cin, 32)), ints(-2, 2, (32,)), ints(-3, 3, act),
          ints(-3, 3, act))


def exactly(label, got, want64):
  """got (f32, from the GPU) is the f64 oracle's value, which is an f32 value"""
  want64 = np.asarray(want64, np.float64)
  want = want64.astype(np.float32)
  assert np.array_equal(want.astype(np.float64), want64), label
  assert np.abs(want64).max() > 0, label
  differ = int((got != want).sum())
  print('%-44s exact case: %d of %d differ from f64, max |value| %g' %
        (label, differ, want.size, np.abs(want64).max()))
  assert got.shape == want.shape and differ == 0, label


def oracle_pair(*args, **kwargs):
  import torch
  return (ref.conv_case(*args, dtype=torch.float64, **kwargs),
          ref.conv_case(*args, dtype=torch.float32, **kwargs))


# -- 1. conv forward ----------------------------------------------------------
@pytest.mark.parametrize('use_skip', [False, True])
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('cin', [2, 32])
@pytest.mark.parametrize('shape', SHAPES)
def test_conv_forward(ops, dev, torch, shape, cin, relu_in, use_skip):
  x, w, b, dy, skip = conv_inputs(shape, cin, seed=1)
  r64, r32 = oracle_pair(x, w, b, dy, relu_in=relu_in,
                         skip=skip if use_skip else None)
  runs = [run_forward(ops, dev, torch, shape, cin, x, relu_in, w, b,
                      skip if use_skip else None) for _ in range(2)]
  assert np.array_equal(runs[0], runs[1])
  yardstick('conv_forward %s cin %d' % (shape, cin), runs[0], r64[0], r32[0])
  check_forward_exact(ops, dev, torch, shape, cin, relu_in, use_skip)


def run_forward(ops, dev, torch, shape, cin, x, relu_in, w, b, skip):
  xd = [dev(p) for p in x] if cin == 2 else [dev(x), None]
  wd, bd, sd = dev(w), dev(b), None if skip is None else dev(skip)
  y = torch.full(shape + (32,), np.nan, dtype=torch.float32, device='cuda:0')
  torch.cuda.synchronize()
  ops.conv_forward(shape[0], shape[1:], cin, xd[0], xd[1], relu_in, wd, bd, sd,
                   y)
  return host(y)


def check_forward_exact(ops, dev, torch, shape, cin, relu_in, use_skip):
  x, w, b, dy, skip = exact_conv_inputs(shape, cin, seed=11)
  skip = skip if use_skip else None
  r64 = ref.conv_case(x, w, b, dy, relu_in=relu_in, skip=skip,
                      dtype=torch.float64)
  got = run_forward(ops, dev, torch, shape, cin, x, relu_in, w, b, skip)
  exactly('conv_forward %s cin %d' % (shape, cin), got, r64[0])


# (1, 2, 3, 4): fewer positions than one tile of any of the three ops
@pytest.mark.parametrize('use_skip', [False, True])
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('cin', [2, 32])
def test_conv_forward_exact_single_slice(ops, dev, torch, cin, relu_in,
                                         use_skip):
  check_forward_exact(ops, dev, torch, (1, 2, 3, 4), cin, relu_in, use_skip)


# -- 2. conv backward to the input -------------------------------------------
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('use_mask', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_conv_backward_input(ops, dev, torch, shape, use_mask, accumulate):
  x, w, b, dy, old = conv_inputs(shape, 32, seed=2)
  pre = x  # any array serves as the pre-activation whose sign masks dx
  r64, r32 = oracle_pair(x, w, b, dy)

  def finish(dx):
    if use_mask:
      dx = dx * (pre > 0).astype(dx.dtype)
    if accumulate:
      dx = dx + old.astype(dx.dtype)
    return dx

  got = run_backward_input(ops, dev, torch, shape, dy, w, pre, old, use_mask,
                           accumulate)
  yardstick('conv_backward_input %s' % (shape,), got, finish(r64[1]),
            finish(r32[1]))
  check_backward_input_exact(ops, dev, torch, shape, use_mask, accumulate)


def run_backward_input(ops, dev, torch, shape, dy, w, pre, old, use_mask,
                       accumulate):
  dxd = dev(old) if accumulate else torch.full(
      shape + (32,), np.nan, dtype=torch.float32, device='cuda:0')
  torch.cuda.synchronize()
  ops.conv_backward_input(shape[0], shape[1:], dev(dy), dev(w),
                          dev(pre) if use_mask else None, accumulate, dxd)
  return host(dxd)


def check_backward_input_exact(ops, dev, torch, shape, use_mask, accumulate):
  x, w, b, dy, old = exact_conv_inputs(shape, 32, seed=12)
  dx = ref.conv_case(x, w, b, dy, dtype=torch.float64)[1]
  if use_mask:
    dx = dx * (x > 0).astype(dx.dtype)
  if accumulate:
    dx = dx + old.astype(dx.dtype)
  got = run_backward_input(ops, dev, torch, shape, dy, w, x, old, use_mask,
                           accumulate)
  exactly('conv_backward_input %s' % (shape,), got, dx)


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('use_mask', [False, True])
def test_conv_backward_input_exact_single_slice(ops, dev, torch, use_mask,
                                                accumulate):
  check_backward_input_exact(ops, dev, torch, (1, 2, 3, 4), use_mask,
                             accumulate)


# -- 3. conv backward to the weights -----------------------------------------
def run_backward_weights(ops, dev, torch, shape, cin, x, relu_in, dy):
  xd = [dev(p) for p in x] if cin == 2 else [dev(x), None]
  dw = torch.full((27 * cin * 32,), np.nan, dtype=torch.float32,
                  device='cuda:0')
  db = torch.full((32,), np.nan, dtype=torch.float32, device='cuda:0')
  torch.cuda.synchronize()
  ops.conv_backward_weights(shape[0], shape[1:], cin, xd[0], xd[1], relu_in,
                            dev(dy), dw, db)
  return host(dw).reshape(3, 3, 3, cin, 32), host(db)


# (2, 9, 11, 13): per item 27 tiles of 32 positions in slices of 4 (cin 32)
# and 1287 positions in slices of 128 (cin 2): the last slice of an item is
# partial in both.  (1, 2, 3, 4) fits in a single slice.
@pytest.mark.parametrize('relu_in', [False, True])
@pytest.mark.parametrize('cin', [2, 32])
@pytest.mark.parametrize('shape', SHAPES + [(1, 2, 3, 4)])
def test_conv_backward_weights(ops, dev, torch, shape, cin, relu_in):
  x, w, b, dy, _ = conv_inputs(shape, cin, seed=3)
  r64, r32 = oracle_pair(x, w, b, dy, relu_in=relu_in)
  first = run_backward_weights(ops, dev, torch, shape, cin, x, relu_in, dy)
  again = run_backward_weights(ops, dev, torch, shape, cin, x, relu_in, dy)
  assert np.array_equal(first[0], again[0])
  assert np.array_equal(first[1], again[1])
  yardstick('dW %s cin %d' % (shape, cin), first[0], r64[2], r32[2])
  yardstick('db %s cin %d' % (shape, cin), first[1], r64[3], r32[3])
  x, w, b, dy, _ = exact_conv_inputs(shape, cin, seed=13)
  r64 = ref.conv_case(x, w, b, dy, relu_in=relu_in, dtype=torch.float64)
  dw, db = run_backward_weights(ops, dev, torch, shape, cin, x, relu_in, dy)
  assert np.abs(r64[2]).max() < 2 ** 15
  exactly('dW %s cin %d' % (shape, cin), dw, r64[2])
  exactly('db %s cin %d' % (shape, cin), db, r64[3])


@pytest.mark.parametrize('corner', ['first', 'last'])
@pytest.mark.parametrize('cin', [2, 32])
def test_conv_backward_weights_corner_voxel(ops, dev, torch, cin, corner):
  """dy is 1 at one corner voxel and 0 elsewhere: dW[t][ci][co] is the input
  at the corner shifted by t - 1, exactly, and zero where that leaves the FoV
  (borders and tap order)."""
  shape = (2, 9, 11, 13)
  x, _, _, _, _ = conv_inputs(shape, cin, seed=4)
  xs = np.stack(x, axis=-1) if cin == 2 else x
  at = (0, 0, 0, 0) if corner == 'first' else (1, 8, 10, 12)
  dy = np.zeros(shape + (32,), np.float32)
  dy[at] = 1.0
  dw, db = run_backward_weights(ops, dev, torch, shape, cin, x, False, dy)
  want = np.zeros((3, 3, 3, cin, 32), np.float32)
  for kz in range(3):
    for ky in range(3):
      for kx in range(3):
        p = (at[1] + kz - 1, at[2] + ky - 1, at[3] + kx - 1)
        if all(0 <= v < s for v, s in zip(p, shape[1:])):
          want[kz, ky, kx] = xs[(at[0],) + p][:, None]
  assert np.array_equal(dw, want)
  assert np.array_equal(db, np.ones(32, np.float32))


# -- 4. loss ------------------------------------------------------------------
def test_loss(ops, dev, torch):
  import torch as t
  shape = (2, 5, 7, 9)
  rng = np.random.RandomState(7)
  logits = rng.uniform(-80, 80, shape).astype(np.float32)
  logits.reshape(-1)[:5] = [0.0, 80.0, -80.0, 1e-3, -1e-3]
  labels = np.where(rng.uniform(size=shape) < 0.5, 0.95, 0.05).astype(
      np.float32)
  weights = rng.uniform(0, 2, shape).astype(np.float32)
  weights[rng.uniform(size=shape) < 0.2] = 0.0
  weights.reshape(-1)[:5] = 1.0
  loss64, d64 = ref.loss_case(logits, labels, weights, t.float64)
  _, d32 = ref.loss_case(logits, labels, weights, t.float32)
  xd, zd, wd = dev(logits), dev(labels), dev(weights)
  runs = []
  for _ in range(2):
    d = torch.full(shape, np.nan, dtype=torch.float32, device='cuda:0')
    torch.cuda.synchronize()
    loss = ops.loss(shape[0], shape[1:], xd, zd, wd, d)
    runs.append((loss, host(d)))
  assert runs[0][0] == runs[1][0]
  assert np.array_equal(runs[0][1], runs[1][1])
  rel = abs(runs[0][0] - loss64) / abs(loss64)
  print('loss %.9g  f64 %.9g  relative difference %.3g' %
        (runs[0][0], loss64, rel))
  assert np.isfinite(runs[0][0])
  assert rel <= 1e-6
  yardstick('dlogits', runs[0][1], d64, d32)
  # loss only
  assert ops.loss(shape[0], shape[1:], xd, zd, wd, None) == runs[0][0]


# -- 5 / 6. the whole stack ---------------------------------------------------
def make_model(variables, depth, zyx):
  from ffn_amd.training.models import convstack_3d
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(zyx[::-1]),
                                       deltas=[1, 1, 1], depth=depth)
  m.set_variables(variables)
  return m


def random_model_variables(depth):
  return ref.random_variables(depth, seed=21, stddev=0.05)


STACK_CASES = {
    'fib25_9x11x13': (12, 2, (9, 11, 13), 31),
    'fib25_5x7x9': (12, 3, (5, 7, 9), 32),
    'depth3_5x7x70': (3, 3, (5, 7, 70), 33),
}
_stack_results = {}


@pytest.fixture(scope='module')
def stack_result(gr, fib25_variables):
  """name -> everything the whole-stack protocol needs, computed once."""
  import torch as t

  def get(name):
    if name in _stack_results:
      return _stack_results[name]
    depth, n, zyx, seed = STACK_CASES[name]
    variables = (fib25_variables if name.startswith('fib25') else
                 random_model_variables(depth))
    inputs = ref.training_inputs(n, zyx, seed=seed)
    csg = gr.ConvStackGradients(make_model(variables, depth, zyx), n, 0)
    loss, logits, grads, pre = csg.loss_and_gradients(
        *inputs, return_pre_activations=True)
    csg.close()
    masks = [p > 0 for p in pre]
    out = dict(
        depth=depth, variables=variables, gpu=(loss, logits, grads, pre),
        free64=ref.run(variables, depth, *inputs, dtype=t.float64,
                       want_grads=False),
        free32=ref.run(variables, depth, *inputs, dtype=t.float32,
                       want_grads=False),
        masked64=ref.run(variables, depth, *inputs, dtype=t.float64,
                         masks=masks),
        masked32=ref.run(variables, depth, *inputs, dtype=t.float32,
                         masks=masks))
    out['e_ref'] = {k: ref.spread(out['masked32']['grads'][k], g)
                    for k, g in out['masked64']['grads'].items()}
    _stack_results[name] = out
    return out
  return get


@pytest.mark.parametrize('name', sorted(STACK_CASES))
def test_whole_stack(stack_result, name):
  r = stack_result(name)
  loss, logits, grads, pre = r['gpu']
  depth = r['depth']
  assert len(pre) == 2 * depth
  assert len(grads) == 4 * depth + 2
  # pre-activation agreement and sign flips
  total = flips = ref_flips = 0
  for k, (p, p64, p32) in enumerate(zip(pre, r['free64']['pre'],
                                        r['free32']['pre'])):
    dist = float(np.max(np.abs(p - p64)))
    assert dist <= 1e-4, (k, dist)
    differ = (p > 0) != (p64 > 0)
    if differ.any():
      assert np.max(np.abs(p64[differ])) <= dist, (k, dist)
    total += p.size
    flips += int(differ.sum())
    ref_flips += int(((p32 > 0) != (p64 > 0)).sum())
  print('%s: %d ReLU inputs, sign flips against f64: GPU %d, f32 oracle %d' %
        (name, total, flips, ref_flips))
  assert flips <= 1e-4 * total
  assert ref_flips <= 1e-4 * total
  # gradients, both oracle runs on the GPU's masks
  worst = (0.0, 0.0, None)
  for key in sorted(grads):
    assert grads[key].shape == r['variables'][key].shape
    e_gpu, e_ref = yardstick(key, grads[key], r['masked64']['grads'][key],
                             r['masked32']['grads'][key])
    worst = max(worst, (e_gpu, e_ref, key))
  print('%s: largest E_gpu %.3g (E_ref %.3g) at %s' % ((name,) + worst))
  # loss and logits
  loss64 = r['free64']['loss']
  rel = abs(loss - loss64) / abs(loss64)
  dist = float(np.max(np.abs(logits - r['free64']['logits'])))
  print('%s: loss %.9g  f64 %.9g  relative %.3g; logits within %.3g' %
        (name, loss, loss64, rel, dist))
  assert rel <= 1e-6
  assert dist <= 1e-4


# -- 7. 33^3 ------------------------------------------------------------------
def test_fov_33_batches_and_repeats(gr, stack_result, fib25_variables,
                                    fib25_blob):
  from oracle import ffn_oracle
  zyx = (33, 33, 33)
  seed, image, labels, weights = ref.training_inputs(2, zyx, seed=41)
  csg = gr.ConvStackGradients(make_model(fib25_variables, 12, zyx), 2, 0)
  one = [a[:1] for a in (seed, image, labels, weights)]
  loss1, logits1, grads1 = csg.loss_and_gradients(*one)
  loss1b, logits1b, grads1b = csg.loss_and_gradients(*one)
  assert loss1 == loss1b and np.array_equal(logits1, logits1b)
  for key in grads1:
    assert np.array_equal(grads1[key], grads1b[key]), key
  want = ffn_oracle.forward(image[0], seed[0], fib25_blob, 12)
  dist = float(np.max(np.abs(logits1[0] - want)))
  print('33^3 logits within %.3g of the C oracle' % dist)
  assert dist <= 1e-4
  # the same FoV as item 0 of a batch of 2 whose item 1 has zero loss weight:
  # every term of item 1 is exactly zero and the mean runs over twice as many
  # voxels, so twice the batch's gradient is the FoV's own.  (The unit sums an
  # item's terms in an order that does not depend on the batch, so the spread
  # is expected to be 0.)  E_ref: the f32 oracle's spread on the 9x11x13 case.
  w2 = weights.copy()
  w2[1] = 0.0
  loss2, logits2, grads2 = csg.loss_and_gradients(seed, image, labels, w2)
  csg.close()
  assert np.array_equal(logits2[0], logits1[0])
  # two f32 tree sums of positive terms, each within (log2(2 N) + 1) 2^-24 =
  # 1.1e-6 of its exact value
  assert abs(2 * loss2 - loss1) <= 2.2e-6 * abs(loss1)
  e_ref = stack_result('fib25_9x11x13')['e_ref']
  worst = (0.0, 0.0, None)
  for key in sorted(grads1):
    e = ref.spread(2.0 * grads2[key], grads1[key])
    print('%-44s E_batch %.3g  E_ref %.3g' % (key, e, e_ref[key]))
    worst = max(worst, (e, e_ref[key], key))
    assert e <= FACTOR * e_ref[key], (key, e, e_ref[key])
  print('33^3: largest batch-2 / batch-1 spread %.3g (E_ref %.3g) at %s' % worst)


# -- 8. errors ----------------------------------------------------------------
def test_bad_arguments_launch_nothing(ops, dev, torch):
  from ffn_amd import _lib
  shape = (2, 3, 4, 5)
  x, w, b, dy, _ = conv_inputs(shape, 32, seed=9)
  canary = np.float32(-12345.0)
  xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
  plane = dev(x[..., 0])
  outs = {k: torch.full(s, float(canary), dtype=torch.float32, device='cuda:0')
          for k, s in (('act', shape + (32,)), ('dw', (27 * 32 * 32,)),
                       ('db', (32,)), ('vox', shape))}
  torch.cuda.synchronize()
  lib, h = ops._lib, ops._h
  P = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
  zyx = _lib.i3(shape[1:])
  loss = ctypes.c_float(float(canary))

  def forward(n=2, cin=32, x=xd, y=outs['act'], zyx=zyx):
    return lib.ffn_gradients_conv_forward(h, n, zyx, cin, P(x), P(None), 0,
                                          P(wd), P(bd), P(None), P(y))

  def backward_input(n=2, dy=dyd):
    return lib.ffn_gradients_conv_backward_input(h, n, zyx, P(dy), P(wd),
                                                 P(None), 0, P(outs['act']))

  def backward_weights(n=2, cin=32, dy=dyd):
    return lib.ffn_gradients_conv_backward_weights(
        h, n, zyx, cin, P(xd), P(None), 0, P(dy), P(outs['dw']), P(outs['db']))

  def head_forward(n=2, seed=plane):
    return lib.ffn_gradients_head_forward(h, n, zyx, P(xd), P(seed), P(bd),
                                          P(bd), P(outs['vox']))

  def head_backward(n=2, dl=plane):
    return lib.ffn_gradients_head_backward(h, n, zyx, P(xd), P(dl), P(bd),
                                           P(outs['act']), P(outs['db']),
                                           P(outs['db']))

  def loss_call(n=2, labels=plane):
    return lib.ffn_gradients_loss(h, n, zyx, P(plane), P(labels), P(plane),
                                  ctypes.byref(loss), P(outs['vox']))

  for call in (forward, backward_input, backward_weights, head_forward,
               head_backward, loss_call):
    assert call(n=0) == ERR_ARG, call.__name__
    assert call(n=33) == ERR_ARG, call.__name__
  assert forward(cin=5) == ERR_ARG
  assert backward_weights(cin=5) == ERR_ARG
  assert forward(x=None) == ERR_ARG
  assert forward(y=None) == ERR_ARG
  assert forward(cin=2) == ERR_ARG  # the seed plane is missing
  assert forward(zyx=_lib.i3((3, 0, 5))) == ERR_ARG
  assert forward(y=xd) == ERR_ARG   # in place
  assert backward_input(dy=None) == ERR_ARG
  assert backward_weights(dy=None) == ERR_ARG
  assert head_forward(seed=None) == ERR_ARG
  assert head_backward(dl=None) == ERR_ARG
  assert loss_call(labels=None) == ERR_ARG
  assert lib.ffn_last_error()
  torch.cuda.synchronize()
  for k, t in outs.items():
    assert np.all(host(t) == canary), k
  assert loss.value == canary
  assert np.array_equal(host(xd), x)
  # and the same handle still works
  assert forward() == 0
