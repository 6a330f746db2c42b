"""The fp16 inference mode (engine option mfma_products = 1) on the CPU: its torch
restatement tests/half_ref.py against the f64 oracle where the two must coincide, and
what plan_stack does with the product count (tests/half_plan_shim.cpp, g++ alone)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import half_ref

HERE = os.path.dirname(os.path.abspath(__file__))
FAMILIES = ['Conv32', 'Conv32c', 'D160', 'D96', 'M', 'MT', 'H']


def exact_depth1_variables(seed=7, representable=True):
  """Depth-1 variables (conv0_a -> conv0_b -> head) whose conv0_b sees only
  fp16-representable operands for images that are multiples of 2^-6 in [-4, 4): conv0_a
  is the centre tap of the image channel times a power of two per output channel, no
  bias; conv0_b's weights are rounded to fp16 (none in (0, 2^-14))."""
  from oracle import ffn_oracle
  v = ffn_oracle.random_weights(1, seed=seed, stddev=0.05)
  rng = np.random.RandomState(seed)
  w0 = np.zeros((3, 3, 3, 2, 32), np.float32)
  w0[1, 1, 1, 0, :] = 2.0 ** rng.randint(-3, 2, size=32)
  v['seed_update/conv0_a/weights'] = w0
  v['seed_update/conv0_a/biases'] = np.zeros(32, np.float32)
  if representable:
    w = half_ref.hi_np(v['seed_update/conv0_b/weights'])
    assert not ((np.abs(w) > 0) & (np.abs(w) < half_ref.TINY)).any()
    v['seed_update/conv0_b/weights'] = w
  return v


def exact_image(shape, seed=11):
  rng = np.random.RandomState(seed)
  return (rng.randint(-256, 256, size=shape) / 64.0).astype(np.float32)


def test_hi_is_the_stored_hi_half():
  """RNE to fp16, |v| < 2^-14 to zero, representable values untouched."""
  v = np.array([1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -14, 2.0 ** -15,
                -2.0 ** -15, 0.9999 * 2.0 ** -14, 0.1, -4.0, 65504.0], np.float32)
  got = half_ref.hi_np(v)
  want = np.array([1.0, 1.0, 1.0 + 2.0 ** -9, 2.0 ** -14, 0.0, 0.0, 0.0,
                   float(np.float16(0.1)), -4.0, 65504.0], np.float32)
  assert np.array_equal(got, want)
  assert np.array_equal(half_ref.hi_np(got), got)


def test_h64_is_the_f64_oracle_on_representable_operands():
  """With activations and weights that are exactly fp16-representable hi() changes
  nothing: h64 equals forward_torch(f64=True) to the last bit of the f32 result."""
  from oracle import ffn_oracle
  variables = exact_depth1_variables()
  image = exact_image((2, 9, 11, 13))
  seed = np.random.RandomState(3).normal(0, 1, image.shape).astype(np.float32)
  want = ffn_oracle.forward_torch(image, seed, dict(variables), 1, f64=True)
  got = half_ref.forward_half(image, seed, variables, 1, acc='h64')
  assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
  # ... and with weights that are NOT representable it is the oracle on hi(w), and no
  # longer the oracle on w
  raw = exact_depth1_variables(representable=False)
  got = half_ref.forward_half(image, seed, raw, 1, acc='h64')
  on_hi = ffn_oracle.forward_torch(image, seed, half_ref.hi_variables(raw, 1), 1, f64=True)
  on_w = ffn_oracle.forward_torch(image, seed, dict(raw), 1, f64=True)
  assert np.array_equal(got.view(np.uint32), on_hi.view(np.uint32))
  assert not np.array_equal(got, on_w)


def test_h32_stands_close_to_h64(fib25_variables):
  """The f32 restatement on ordinary data (FIB-25 weights, depth 12, a small FoV): it
  differs from h64 -- by rounding-boundary flips of the activations, so by far more than
  an f32 sum's error -- and stays well inside the mode's own distance to f64."""
  from ffn_amd import synthetic
  from oracle import ffn_oracle
  vol = synthetic.normalize(synthetic.cells_volume((48, 48, 48), seed=3))
  image = vol[4:13, 5:16, 6:19]
  seed = np.full(image.shape, ffn_oracle.f32_logit(0.05), np.float32)
  seed[4, 5, 6] = ffn_oracle.f32_logit(0.95)
  h64 = half_ref.forward_half(image, seed, fib25_variables, 12, acc='h64')
  h32 = half_ref.forward_half(image, seed, fib25_variables, 12, acc='h32')
  f64 = ffn_oracle.forward_torch(image, seed, dict(fib25_variables), 12, f64=True)
  d_impl = float(np.abs(h32 - h64).max())
  d_mode = float(np.abs(h64 - f64).max())
  print('max|h32 - h64| %.3g   max|h64 - f64| %.3g' % (d_impl, d_mode))
  assert 0 < d_impl <= d_mode
  assert 1e-4 < d_mode < 2e-2  # (2.7e-3 on this input: a thousand times the split kernels')


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
  """plan_stack with EIGHT arguments (the build fails without the parameter)."""
  out = os.path.join(str(tmp_path_factory.mktemp('half_plan')), 'half_plan_shim.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC',
                         '-o', out, os.path.join(HERE, 'half_plan_shim.cpp')])
  lib = ctypes.CDLL(out)
  lib.half_plan_stack.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 8 + [
      ctypes.c_void_p]

  def call(variant, flow, n, products, flow_skip=0, tail_batched=0, batch_chunks=1,
           fov=(33, 33, 33), deltas=(8, 8, 8), depth=12):
    f, d = np.asarray(fov, np.int32), np.asarray(deltas, np.int32)
    res = np.zeros(5, np.int32)
    lib.half_plan_stack(f.ctypes.data, d.ctypes.data, depth, variant, flow, flow_skip,
                        tail_batched, batch_chunks, n, products, res.ctypes.data)
    return dict(family=FAMILIES[res[0]], resident=bool(res[1]), tail_tiles=int(res[2]),
                chunks=int(res[3]), products=int(res[4]))
  return call


def test_one_product_plan_is_never_resident(plan):
  three = plan(9, 2, 1, 3)
  one = plan(9, 2, 1, 1)
  assert three == dict(family='MT', resident=True, tail_tiles=1, chunks=356, products=3)
  assert one['resident'] is False
  assert one['family'] == 'MT' and one['products'] == 1
  assert one['chunks'] == three['chunks'] and one['tail_tiles'] == three['tail_tiles']
  # the same plan as flow = 0 gives the three-product stack, but for the product count
  assert {**plan(9, 0, 1, 3), 'products': 1} == one


def test_only_m_and_mt_take_the_product_count(plan):
  """Every other family ignores the option (products 3 in its plan) and keeps its plan
  otherwise; M and MT keep family, chunks and tail tiles."""
  seen = set()
  for variant in (0, 2, 6, 7, 8, 9, 10):
    for n in (1, 2, 16):
      for flow in (0, 2):
        for tail_batched in (0, 1):
          for batch_chunks in (1, 2):
            kw = dict(tail_batched=tail_batched, batch_chunks=batch_chunks)
            three = plan(variant, flow, n, 3, **kw)
            one = plan(variant, flow, n, 1, **kw)
            seen.add(three['family'])
            assert three['products'] == 3
            if three['family'] in ('M', 'MT'):
              assert one == {**three, 'products': 1, 'resident': False}
            else:
              assert one == three, (variant, n, flow)
  assert seen == set(FAMILIES)
