"""Zero-tolerance parity of the conv stack: on the cases of tests/exact_stack.py -- every
operand on one power-of-two grid, every sum of |terms| below 2^23 grid units, no conv with
a split residual on both sides -- every conv kernel of the engine must return the f64
oracle's logits bit for bit (the argument is in tests/exact_stack.py, the CPU half in
tests/test_exact_stack.py).  Every comparison here is np.array_equal against
ffn_oracle.forward_f64c; there is no float gate.  A dropped, doubled, misplaced or
misweighted term moves a logit by at least one grid unit.

After every predict the engine's conv_variant must still be what the test set: a value
past the fp16 range would void the step and repeat it on exact_variant, and the test would
pass on the wrong kernel.

Every test prints `exact_stack <case> <variant / flow / n>: equal` lines and the case's
measured maxima (profiles/exact_stack.txt is made of them)."""

import numpy as np
import pytest

from tests import exact_stack as es
from tests import fov_edges
from tests.test_gpu_fov_edges import VARIANTS, _admitted
from tests.test_stack_plan import _expected

pytestmark = pytest.mark.gpu

_PREPARED = {}


@pytest.fixture(scope='module')
def prepared():
  """name -> the case with its variables, inputs, measured rows and the f64 oracle's
  logits, each computed once for the module and never written to again."""
  from oracle import ffn_oracle

  def get(name):
    if name not in _PREPARED:
      case = es.BY_NAME[name]
      variables, image, seed = es.build(case)
      rows = es.preconditions(variables, case.depth, image, seed,
                              one_product=case.one_product)
      blob = ffn_oracle.weights_blob(variables, case.depth)
      want = ffn_oracle.forward_f64c(image, seed, blob, case.depth)
      for a in (image, seed, want):
        a.setflags(write=False)
      print('exact_stack %s fov %s depth %d: %s' % (
          name, 'x'.join(str(f) for f in case.fov), case.depth, es.maxima(rows)))
      _PREPARED[name] = dict(case=case, variables=variables, image=image, seed=seed,
                             want=want, rows=rows)
    return _PREPARED[name]
  return get


def _engine(p, max_batch):
  from ffn_amd import engine as hip_engine
  from ffn_amd.training.models import convstack_3d
  case = p['case']
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(case.fov[::-1]),
                                       deltas=list(case.deltas[::-1]), depth=case.depth)
  m.set_variables(p['variables'])
  return hip_engine.HipEngine.from_model(m, max_batch=max_batch)


def _equal(p, what, got, n, first=0):
  want = p['want'][first:first + n]
  same = np.array_equal(got, want)
  name = p['case'].name
  if not same:
    d = np.abs(got.astype(np.float64) - want)
    print('exact_stack %s %s: DIFFERENT at %d of %d logits, max |difference| %g '
          '(grid %g)' % (name, what, int((d != 0).sum()), d.size, d.max(),
                         min(r.grid for r in p['rows'])))
  else:
    print('exact_stack %s %s: equal' % (name, what))
  assert same, (name, what)


def _predict(eng, p, n, variant, what, first=0):
  got = eng.predict(p['seed'][first:first + n], p['image'][first:first + n])
  assert eng.get_option('conv_variant') == variant, (
      'the step was voided and repeated on another kernel', what)
  _equal(p, what, got, n, first)
  return got


def _set_admitted(eng, exp, variant):
  """sets conv_variant if the geometry's rules admit it; True if it is set"""
  from ffn_amd import _lib
  admitted = _admitted(exp)[variant]
  try:
    eng.set_option('conv_variant', variant)
    accepted = True
  except _lib.FFNHipError:
    accepted = False
  if variant == 10 and admitted and not accepted:
    print('exact_stack: variant 10 refused where h_geom_ok holds (its residency half)')
    return False
  assert accepted == admitted, (variant, accepted, admitted)
  return accepted


def _every_variant(eng, p, exp, ns, variants=VARIANTS):
  ran = []
  for variant in variants:
    if not _set_admitted(eng, exp, variant):
      continue
    ran.append(variant)
    for n in ns:
      _predict(eng, p, n, variant, 'variant %d n %d' % (variant, n))
  assert ran, 'no variant ran'
  return ran


def _resident_forms(eng, p, what=''):
  """conv_variant 9, one FoV: flow 0, 1 and 2, then the production and the LAB form of the
  resident launch and the per-layer launches.  False if this device cannot hold the
  resident launch (flow 0 after creation): flow 0 alone is checked then."""
  from tests.test_gpu_lean_stack import _three_ways
  eng.set_option('conv_variant', 9)
  resident = eng.get_option('flow') == 2
  for flow in (0, 1, 2) if resident else (0,):
    eng.set_option('flow', flow)
    _predict(eng, p, 1, 9, '%svariant 9 flow %d n 1' % (what, flow))
    assert eng.get_option('stat_flow_timeouts') == 0, flow
  if resident:
    out = _three_ways(eng, p['seed'][:1], p['image'][:1])
    _equal(p, '%sresident, production form' % what, out[0], 1)
    _equal(p, '%sresident, LAB form' % what, out[1], 1)
    _equal(p, '%sper-layer launches' % what, out['layers'], 1)
    assert eng.get_option('conv_variant') == 9
  assert eng.get_option('stat_flow_timeouts') == 0
  return resident


NOT_RESIDENT = ('flow 0 after creation (this device cannot hold the resident launch): the '
                'per-layer launches alone were checked, every comparison equal')


# -- a. 33^3 at depth 12 -----------------------------------------------------------------
def test_deep_33_every_variant_and_the_resident_forms(prepared):
  p = prepared('deep4_33')
  exp = _expected(p['case'].fov, p['case'].depth)
  eng = _engine(p, 1)
  try:
    assert eng.get_option('conv_variant') == exp['default_variant'] == 9
    ran = _every_variant(eng, p, exp, (1,))
    assert set(ran) >= {0, 2, 6, 7, 8, 9}
    resident = _resident_forms(eng, p)
  finally:
    eng.close()
  if not resident:
    pytest.skip(NOT_RESIDENT)


# -- b. the same model in batches --------------------------------------------------------
def test_deep_33_batches(prepared):
  p = prepared('deep4_33')
  eng = _engine(p, 4)
  try:
    for variant in (6, 8, 9):
      eng.set_option('conv_variant', variant)
      for n in (3, 4):
        _predict(eng, p, n, variant, 'max_batch 4 variant %d n %d' % (variant, n))
    eng.set_option('tail_batched', 1)
    for n in (3, 4):
      _predict(eng, p, n, 9, 'max_batch 4 variant 9 tail_batched n %d' % n)
    # one FoV that is not item 0 of the inputs
    _predict(eng, p, 1, 9, 'max_batch 4 variant 9 tail_batched item 3 alone', first=3)
    eng.set_option('tail_batched', 0)
    assert eng.get_option('stat_flow_timeouts') == 0
  finally:
    eng.close()


# -- c. a batch of 17 in max_batch 32 ----------------------------------------------------
@pytest.mark.parametrize('name', ['deep4_last_one', 'deep4_perm021_small'])
def test_batch_of_17(prepared, name):
  p = prepared(name)
  exp = _expected(p['case'].fov, p['case'].depth)
  eng = _engine(p, 32)
  try:
    default = eng.get_option('conv_variant')
    assert default == exp['default_variant']
    _predict(eng, p, 17, default, 'max_batch 32 default variant %d n 17' % default)
    ran = _every_variant(eng, p, exp, (17,), [v for v in VARIANTS if v != default])
    assert ran
    # a single FoV from the middle of the inputs, after the batches ran in these buffers
    eng.set_option('conv_variant', default)
    _predict(eng, p, 1, default, 'max_batch 32 default variant %d item 9 alone' % default,
             first=9)
  finally:
    eng.close()


# -- d. dense: every entry of the weight fragments ---------------------------------------
def test_dense_33_every_variant(prepared):
  p = prepared('dense_33')
  exp = _expected(p['case'].fov, p['case'].depth)
  eng = _engine(p, 1)
  try:
    ran = _every_variant(eng, p, exp, (1,))
    assert set(ran) >= {0, 2, 6, 7, 8, 9}
    resident = _resident_forms(eng, p)
  finally:
    eng.close()
  if not resident:
    pytest.skip(NOT_RESIDENT)


@pytest.mark.parametrize('edge', [e[0] for e in fov_edges.EDGES])
def test_dense_at_the_edge_geometries(prepared, edge):
  """the permuted layouts, the one-voxel last chunk, 256 tail workgroups, the 7-voxel tail,
  the widest row ...: every variant the rules admit, one FoV and two"""
  p = prepared('dense_' + edge)  # (re-passes the preconditions at its own FoV)
  case = p['case']
  assert (case.fov, case.deltas) == fov_edges.BY_NAME[edge][1:3]
  exp = _expected(case.fov, case.depth)
  eng = _engine(p, 2)
  try:
    assert eng.get_option('conv_variant') == exp['default_variant']
    ran = _every_variant(eng, p, exp, (1, 2))
    assert exp['default_variant'] in ran
    # the second FoV alone
    eng.set_option('conv_variant', exp['default_variant'])
    _predict(eng, p, 1, exp['default_variant'],
             'variant %d item 1 alone' % exp['default_variant'], first=1)
    assert eng.get_option('stat_flow_timeouts') == 0
  finally:
    eng.close()


# -- e. one conv with a residual weight plane --------------------------------------------
@pytest.mark.parametrize('geometry', ['33', 'perm021_resident'])
@pytest.mark.parametrize('which', es.WHICH)
def test_weight_residual_plane(prepared, which, geometry):
  p = prepared('wres_%s_%s' % (which, geometry))
  case = p['case']
  exp = _expected(case.fov, case.depth)
  assert exp['default_variant'] == 9
  conv = [r for r in p['rows'] if r.name == which][0]
  assert conv.w_residual and not conv.x_residual
  assert min(r.grid for r in p['rows']) == 2.0 ** -11
  eng = _engine(p, 1)
  try:
    ran = _every_variant(eng, p, exp, (1,), (2, 6, 7, 8, 9))
    assert set(ran) >= {6, 8, 9}
    resident = _resident_forms(eng, p)
  finally:
    eng.close()
  if not resident:
    pytest.skip(NOT_RESIDENT)


# -- f. 41 x 41 x 21 at depth 18 ---------------------------------------------------------
def test_configs4_geometry_depth_18(prepared):
  p = prepared('deep2_configs4')
  case = p['case']
  assert case.depth == 18
  exp = _expected(case.fov, case.depth)
  eng = _engine(p, 1)
  try:
    default = eng.get_option('conv_variant')
    assert default == exp['default_variant'] == 9
    _predict(eng, p, 1, default, 'default variant %d n 1' % default)
    resident = _resident_forms(eng, p)
  finally:
    eng.close()
  if not resident:
    pytest.skip(NOT_RESIDENT)


# -- g. one product ----------------------------------------------------------------------
def test_one_product_on_fp16_operands(prepared):
  """mfma_products = 1 keeps hi x hi alone: on operands and weights of at most 11
  significant bits that is still every term."""
  p = prepared('deep2_33')
  assert all(max(r.operand_bits, r.weight_bits) <= es.FP16_BITS for r in p['rows'][1:-1])
  eng = _engine(p, 3)
  try:
    eng.set_option('mfma_products', 1)
    for variant in (8, 9):
      eng.set_option('conv_variant', variant)
      for n in (1, 3):
        _predict(eng, p, n, variant, 'one product, variant %d n %d' % (variant, n))
    assert eng.get_option('mfma_products') == 1
  finally:
    eng.close()


def test_one_product_control_reaches_the_kernel(prepared):
  """The 4-nonzero model reads activations of 14 bits: with one product their residuals
  are gone and the logits are NOT the oracle's; back on three products they are."""
  p = prepared('deep4_33')
  assert max(r.operand_bits for r in p['rows'][1:-1]) > es.FP16_BITS
  eng = _engine(p, 3)
  try:
    for variant in (8, 9):
      eng.set_option('conv_variant', variant)
      for n in (1, 3):
        eng.set_option('mfma_products', 1)
        got = eng.predict(p['seed'][:n], p['image'][:n])
        assert eng.get_option('conv_variant') == variant
        differ = int((got != p['want'][:n]).sum())
        print('exact_stack deep4_33 one product, variant %d n %d: %d of %d logits differ '
              '(the control)' % (variant, n, differ, got.size))
        assert differ > 0, (variant, n)
        eng.set_option('mfma_products', 3)
        _predict(eng, p, n, variant, 'three products again, variant %d n %d' % (variant, n))
  finally:
    eng.close()


# -- the comparison has teeth ------------------------------------------------------------
@pytest.mark.parametrize('name', ['deep4_last_one', 'wres_conv1_a_33'])
def test_a_single_changed_weight_on_the_engine_is_seen(prepared, name):
  """tests/test_exact_stack.py shows on the oracle that every single-weight mutation moves
  the f64 logits; here the ENGINE gets the mutated weights and the oracle keeps the
  original ones: the comparison that every test above makes must fail, for each mutation
  and under the default and the exact kernel."""
  from oracle import ffn_oracle
  p = prepared(name)
  case = p['case']
  eng = _engine(p, 1)
  try:
    default = eng.get_option('conv_variant')
    rng = np.random.RandomState(5)
    for k in range(6):
      mutant, what = es.mutate(p['variables'], case.depth, rng)
      eng.set_weights(ffn_oracle.weights_blob(mutant, case.depth))
      for variant in (default, eng.get_option('exact_variant')):
        eng.set_option('conv_variant', variant)
        got = eng.predict(p['seed'][:1], p['image'][:1])
        differ = int((got != p['want'][:1]).sum())
        print('exact_stack %s mutation %d (%s) variant %d: %d logits differ' % (
            name, k, what, variant, differ))
        assert differ > 0, (what, variant)
    eng.set_weights(ffn_oracle.weights_blob(p['variables'], case.depth))
    eng.set_option('conv_variant', default)
    _predict(eng, p, 1, default, 'the original weights again, variant %d n 1' % default)
  finally:
    eng.close()
