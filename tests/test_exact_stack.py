"""The exact conv-stack cases of tests/exact_stack.py, on the CPU alone: every case meets its
preconditions; the sequential-f32 oracle and the f64 oracle give the same bits on it; the
fp16 split loses nothing of any operand; the three-product sum, restated in f32 in two
association orders, is the f64 value -- and is not where both sides of a conv carry a
residual; and a single changed weight always changes the f64 logits.  What the GPU is then
asked for in tests/test_gpu_exact_stack.py is np.array_equal against the same f64 oracle.
"""

import numpy as np
import pytest

from tests import exact_stack as es


@pytest.fixture(scope='module')
def oracle():
  from oracle import ffn_oracle
  return ffn_oracle


@pytest.mark.parametrize('case', [pytest.param(c, id=c.name) for c in es.CASES])
def test_case_is_exact_on_the_cpu(oracle, case):
  variables, image, seed = es.build(case)
  traced = es.trace(variables, case.depth, image, seed)
  rows = es.preconditions(variables, case.depth, image, seed, one_product=case.one_product,
                          traced=traced)
  print('exact_stack %s fov %s depth %d n %d: %s' % (
      case.name, 'x'.join(str(f) for f in case.fov), case.depth, case.n, es.maxima(rows)))
  assert all(r.abs_sum_units < es.SUM_CAP for r in rows[:-1])
  assert rows[-1].abs_sum_units < es.HEAD_CAP
  if case.one_product:
    assert all(max(r.operand_bits, r.weight_bits) <= es.FP16_BITS for r in rows[1:-1])
  # the f64 logits are f32 values, and all three forward passes agree on them
  logits64 = traced[-1]['logits']
  want = logits64.astype(np.float32)
  assert np.array_equal(logits64, want.astype(np.float64))
  blob = oracle.weights_blob(variables, case.depth)
  assert np.array_equal(oracle.forward_f64c(image, seed, blob, case.depth), want)
  assert np.array_equal(oracle.forward(image, seed, blob, case.depth), want)
  # the split: hi + res / 2048 is the value, for every operand and weight of every conv
  for c, row in zip(traced[1:-1], rows[1:-1]):
    assert c['name'] == row.name
    # (what preconditions calls a residual is what the split leaves)
    assert (row.x_residual, row.w_residual) == (es.has_residual(c['x']),
                                                 es.has_residual(c['w'])), row.name
    for what in ('x', 'w'):
      v = c[what]
      assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), (c['name'], what)
      hi, res = es.split_np(v)
      assert np.all(np.isfinite(res)), (c['name'], what)
      assert np.array_equal(hi.astype(np.float64) + res.astype(np.float64) / 2048, v), (
          c['name'], what)


SMALL = (5, 7, 11)


def _small_trace(builder, args, depth, input_seed):
  variables = es.BUILDERS[builder](*args)
  image, seed = es.exact_inputs(1, SMALL, input_seed)
  return variables, image, seed, {c['name']: c for c in
                                  es.trace(variables, depth, image, seed)}


@pytest.mark.parametrize('builder,args,conv', [
    ('weight_residual', ('conv1_a', 7), 'conv1_a'),   # residual on the weights
    ('weight_residual', ('conv0_b', 7), 'conv1_b'),   # residual on the activations, + skip
])
def test_three_products_in_two_orders_are_the_f64_value(builder, args, conv):
  variables, image, seed, convs = _small_trace(builder, args, 2, 31)
  es.preconditions(variables, 2, image, seed)
  c = convs[conv]
  side = 'w' if conv == 'conv1_a' else 'x'
  assert es.has_residual(c[side]) and not es.has_residual(c['x' if side == 'w' else 'w'])
  skip = None if c['skip'] is None else es.channel_last(c['skip'][0])
  want = es.channel_last(c['pre'][0])
  assert np.abs(want).max() > 0
  for order in ('tap', 'channel'):
    got = es.three_products(es.channel_last(c['x'][0]), c['w'], c['b'], skip, order)
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.float64), want), (conv, order)


def test_control_residuals_on_both_sides_are_refused_and_inexact():
  """Why the precondition is there: with residual weights on a conv whose inputs carry
  residuals too, the three products miss the f64 value by the res x res terms, and
  preconditions says so."""
  variables, image, seed, convs = _small_trace('both_residuals', (7,), 2, 31)
  with pytest.raises(ValueError, match='conv1_a: activations and weights both carry'):
    es.preconditions(variables, 2, image, seed)
  c = convs['conv1_a']
  assert es.has_residual(c['x']) and es.has_residual(c['w'])
  want = es.channel_last(c['pre'][0])
  for order in ('tap', 'channel'):
    got = es.three_products(es.channel_last(c['x'][0]), c['w'], c['b'], None, order)
    missed = np.abs(got.astype(np.float64) - want)
    # (the f64 value lies on the grid 2^-22 here and need not be an f32 value: the miss
    # is more than its rounding to f32)
    assert not np.array_equal(got, want.astype(np.float32))
    assert missed.max() >= 2.0 ** -22
    # what is missing is res_w res_x 2^-22: far below the 1e-4 gate of the float tests
    assert missed.max() < 1e-4
  # the other caps are checked too
  big, _ = es.exact_inputs(1, SMALL, 31, amp=2000)
  with pytest.raises(ValueError, match='> 32768'):
    es.preconditions(es.deep_sparse(12, 4, 3), 12, big, big)
  with pytest.raises(ValueError, match='one product'):
    c4 = es.BY_NAME['deep4_last_one']
    v, im, sd = es.build(c4)
    es.preconditions(v, c4.depth, im[:1], sd[:1], one_product=True)


MUTATION_FAMILIES = [
    ('deep_sparse', (12, 4, 3), 12, SMALL),
    ('deep_sparse', (12, 2, 9), 12, (9, 9, 9)),
    ('dense_shallow', (5,), 2, SMALL),
    ('weight_residual', ('conv1_a', 7), 2, (9, 9, 9)),
]


@pytest.mark.parametrize('builder,args,depth,fov', MUTATION_FAMILIES)
def test_every_single_weight_mutation_changes_the_f64_logits(oracle, builder, args, depth,
                                                            fov):
  """40 of 40: a nonzero weight zeroed, or 1 added to a random entry, of a random conv."""
  variables = es.BUILDERS[builder](*args)
  grid = es.DENSE_GRID if builder == 'dense_shallow' else 1.0
  amp = es.DENSE_AMP if builder == 'dense_shallow' else 4
  image, seed = es.exact_inputs(2, fov, 77, amp, grid)
  want = oracle.forward_f64c(image, seed, oracle.weights_blob(variables, depth), depth)
  rng = np.random.RandomState(2024)
  seen, least = 0, np.inf
  for _ in range(40):
    mutant, what = es.mutate(variables, depth, rng)
    got = oracle.forward_f64c(image, seed, oracle.weights_blob(mutant, depth), depth)
    moved = float(np.abs(got.astype(np.float64) - want).max())
    assert moved > 0, what
    seen += 1
    least = min(least, moved)
  print('exact_stack mutations %s%s fov %s: %d of 40 seen, the smallest change %g' % (
      builder, args, 'x'.join(str(f) for f in fov), seen, least))
  assert seen == 40
