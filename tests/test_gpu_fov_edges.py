"""The conv stack and the canvas step on a GPU at the FoV geometries where a rule of
conv_caps (ffn_amd/csrc/ffn_stack_plan.h) is at its limit: tests/fov_edges.py, found by
tools/fov_edges.py.  What the rules must say about each geometry comes from the CPU
restatement in tests/test_stack_plan.py (_expected), never from what the engine did; the
reference is the double-precision forward (ffn_oracle.forward_f64c), the tolerance the
project's 1e-4.  Every test prints its measured maximum errors (`fov_edges ...` lines:
profiles/fov_edges_errors.txt is made of them).
"""

import ctypes

import numpy as np
import pytest

from tests import fov_edges
from tests.test_gpu_parity import TOL
from tests.test_stack_plan import _expected

pytestmark = pytest.mark.gpu

VARIANTS = (0, 2, 6, 7, 8, 9, 10)
BIG = 40000  # voxels: the four FoVs above it run batches of 2 instead of 3


def _model(fov_zyx, deltas_zyx, depth, seed, stddev=0.07):
  from ffn_amd.training.models import convstack_3d
  from oracle import ffn_oracle
  variables = ffn_oracle.random_weights(depth, seed=seed, stddev=stddev)
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(fov_zyx[::-1]),
                                       deltas=list(deltas_zyx[::-1]), depth=depth)
  m.set_variables(variables)
  return m, variables, ffn_oracle.weights_blob(variables, depth)


def _admitted(exp):
  """conv_variant -> do the rules admit it (set_conv_variant's geometric conditions)"""
  return {0: True, 2: exp['exact_variant'] == 2, 6: exp['d_ok'], 7: exp['e_ok'],
          8: exp['m_ok'], 9: exp['t_ok'], 10: exp['h_geom_ok']}


def _report(name, fov, depth, what, err):
  print('fov_edges %-16s fov %-12s depth %d %-28s max |err| %.3g' % (
      name, 'x'.join(str(f) for f in fov), depth, what, err))


@pytest.mark.parametrize('name,fov,deltas', [
    pytest.param(e[0], e[1], e[2], id=e[0]) for e in fov_edges.EDGES + [fov_edges.TOO_WIDE]])
def test_edge_geometry_predict(name, fov, deltas):
  """Every conv_variant the rules admit computes the f64 reference's logits within TOL,
  for one FoV and for a batch, on two input draws one after the other; every variant the
  rules refuse is refused; and the identities between the variants that the suite asserts
  at 33^3 hold here too."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  depth = 2
  if name == 'too_wide':
    m, _, _ = _model(fov, deltas, depth, seed=21)
    with pytest.raises(_lib.FFNHipError, match='too wide'):
      hip_engine.HipEngine.from_model(m, max_batch=1)
    # the refusal left nothing behind: the next engine of the process works
    _, wfov, wdeltas, _ = fov_edges.BY_NAME['widest']
    m, _, blob = _model(wfov, wdeltas, depth, seed=21)
    eng = hip_engine.HipEngine.from_model(m, max_batch=1)
    try:
      rng = np.random.RandomState(5)
      img = rng.normal(0, 1, (1,) + wfov).astype(np.float32)
      seed = rng.normal(0, 2, (1,) + wfov).astype(np.float32)
      err = np.abs(eng.predict(seed, img) - ffn_oracle.forward_f64c(img, seed, blob, depth)).max()
      _report(name, wfov, depth, 'widest, after the refusal', err)
      assert err <= TOL
    finally:
      eng.close()
    return

  exp = _expected(fov, depth)
  admitted = _admitted(exp)
  nb = 2 if fov[0] * fov[1] * fov[2] > BIG else 3
  m, _, blob = _model(fov, deltas, depth, seed=21)
  eng = hip_engine.HipEngine.from_model(m, max_batch=nb + 1)
  notes = []
  try:
    default = eng.get_option('conv_variant')
    assert default == exp['default_variant']
    assert eng.get_option('exact_variant') == exp['exact_variant']
    flow = eng.get_option('flow')
    assert flow in (0, 2) and (flow == 0 or exp['t_ok'])
    if exp['t_ok'] and flow == 0:
      notes.append('flow 0: this device cannot hold the resident launch')
    rng = np.random.RandomState(9)
    draws = []
    for _ in range(2):
      img = rng.normal(0, 1, (nb + 1,) + fov).astype(np.float32)
      seed = rng.normal(0, 2, (nb + 1,) + fov).astype(np.float32)
      draws.append((img, seed, ffn_oracle.forward_f64c(img, seed, blob, depth)))
    out, current = {}, default
    for variant in VARIANTS:
      try:
        eng.set_option('conv_variant', variant)
        accepted = True
      except _lib.FFNHipError:
        accepted = False
      if variant == 10 and admitted[10] and not accepted:
        notes.append('variant 10 refused where h_geom_ok holds: its residency half')
        continue
      assert accepted == admitted[variant], (
          'conv_variant %d: the rules %s it, the engine %s it' % (
              variant, 'admit' if admitted[variant] else 'refuse',
              'accepted' if accepted else 'refused'))
      if not accepted:
        assert eng.get_option('conv_variant') == current  # a refusal changes nothing
        continue
      current = variant
      for d, (img, seed, want) in enumerate(draws):
        for n in (1, nb):
          got = eng.predict(seed[:n], img[:n])
          err = np.abs(got - want[:n]).max()
          _report(name, fov, depth, 'variant %2d n %d draw %d' % (variant, n, d), err)
          assert err <= TOL, (variant, n, d, err)
          out[variant, d, n] = got
    assert default in [v for v, _, _ in out]
    for d, (img, seed, want) in enumerate(draws):
      # conv32d's arithmetic does not depend on the chunk size
      if (6, d, 1) in out and (7, d, 1) in out:
        assert np.array_equal(out[6, d, 1], out[7, d, 1])
        if not exp['m_ok']:  # (with conv32m a batch of variant 6 runs that)
          assert np.array_equal(out[6, d, nb], out[7, d, nb])
      # variants 9 and 10 run several FoVs as conv32m
      for v in (9, 10):
        if (v, d, nb) in out:
          assert np.array_equal(out[v, d, nb], out[8, d, nb]), v
      if (9, d, 1) in out:
        # tail_batched: conv32mt for every step, the single FoV's bits
        eng.set_option('conv_variant', 9)
        eng.set_option('tail_batched', 1)
        both = eng.predict(seed[:nb], img[:nb])
        last = eng.predict(seed[nb - 1:nb], img[nb - 1:nb])
        eng.set_option('tail_batched', 0)
        assert np.array_equal(both[0], out[9, d, 1][0])
        assert np.array_equal(both[nb - 1], last[0])
        assert np.abs(both - want[:nb]).max() <= TOL
      # a ragged batch gives the full batch's rows, bit for bit
      eng.set_option('conv_variant', default)
      full = eng.predict(seed, img)
      assert np.abs(full - want).max() <= TOL
      assert np.array_equal(full[:nb], out[default, d, nb])
    # and after everything else has run in these buffers, the first run's bits again
    img, seed, _ = draws[0]
    assert np.array_equal(eng.predict(seed[:1], img[:1]), out[default, 0, 1])
    assert eng.get_option('stat_flow_timeouts') == 0
  finally:
    eng.close()
  if notes:
    pytest.skip('%s: everything else held; %s' % (name, '; '.join(notes)))


@pytest.mark.parametrize('name', ['perm021_resident', 'perm021_tail7', 'tail_256'])
def test_resident_stack_at_tail_extremes(name):
  """One tail workgroup (seven of the eight XCDs without one), one of 7 voxels, and the
  256 that fill every slot of the chip: flow 0, 1 and 2, the production and the LAB form
  of the resident launch -- the same bits, within TOL of f64, no poll ever giving up."""
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  from tests.test_gpu_lean_stack import _three_ways
  _, fov, deltas, _ = fov_edges.BY_NAME[name]
  depth = 3
  exp = _expected(fov, depth)
  assert exp['t_ok'] and exp['default_variant'] == 9
  m, _, blob = _model(fov, deltas, depth, seed=40 + depth, stddev=0.05)
  eng = hip_engine.HipEngine.from_model(m, max_batch=1)
  try:
    assert eng.get_option('conv_variant') == 9
    resident = eng.get_option('flow') == 2
    rng = np.random.RandomState(17)
    for trial in range(3):
      img = rng.normal(0, 1, (1,) + fov).astype(np.float32)
      seed = rng.normal(0, 1.5, (1,) + fov).astype(np.float32)
      want = ffn_oracle.forward_f64c(img, seed, blob, depth)
      got = {}
      for flow in (0, 1, 2) if resident else (0,):
        eng.set_option('flow', flow)
        got[flow] = eng.predict(seed, img)
        assert eng.get_option('stat_flow_timeouts') == 0, (trial, flow)
      err = np.abs(got[0] - want).max()
      _report(name, fov, depth, 'variant  9 flow 0 draw %d' % trial, err)
      assert err <= TOL
      if resident:
        assert np.array_equal(got[0], got[1]), trial
        assert np.array_equal(got[0], got[2]), trial
        out = _three_ways(eng, seed, img)
        assert np.array_equal(out[0], got[0]) and np.array_equal(out[1], got[0]), trial
        assert np.array_equal(out['layers'], got[0]), trial
    assert eng.get_option('stat_flow_timeouts') == 0
  finally:
    eng.close()
  if not resident:
    pytest.skip('%s: flow 0 after creation (this device cannot hold the resident launch): '
                'the per-layer launches alone were checked' % name)


# moves of a canvas test in units of the deltas, from the start: between them they go
# along each of the three axes in both directions
MOVES5 = [(0, 0, 0), (1, 0, 0), (-1, 1, 0), (0, -1, 1), (0, 0, -1)]
MOVES3 = [(0, 0, 0), (1, -1, 1), (-1, 1, -1)]


@pytest.mark.parametrize('name,moves', [
    ('perm021_small', MOVES5), ('perm120_small', MOVES5), ('perm102_small', MOVES5),
    ('last_one', MOVES5),
    ('one_chunk_5', MOVES5), ('m_rows_miss', MOVES3)])
def test_edge_geometry_canvas_step(name, moves):
  """gather, conv stack, disco, paste, faces and point reads on the layouts (0,2,1) and
  (1,0,2), with (1,2,0) on the same voxels as the control, and under the defaults 8, 2
  and 6, step by step against the oracle's canvas with the f64 forward behind it."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  from ffn_amd import synthetic
  from oracle import ffn_oracle
  _, fov, deltas, _ = fov_edges.BY_NAME[name]
  depth = 2
  exp = _expected(fov, depth)
  m, _, blob = _model(fov, deltas, depth, seed=8, stddev=0.06)
  eng = hip_engine.HipEngine.from_model(m, max_batch=1)
  try:
    assert eng.get_option('conv_variant') == exp['default_variant']
    shape = tuple(2 * f + 3 for f in fov)  # just over two FoVs per axis
    vol = synthetic.normalize(synthetic.cells_volume(shape, seed=3))
    canvas = eng.create_canvas(vol)
    oc = ffn_oracle.OracleCanvas(vol, blob, depth, fov, deltas, ffn_oracle.Options())
    oc.forward_fn = lambda img, seed: ffn_oracle.forward_f64c(img, seed, blob, depth)
    start = tuple(s // 2 for s in shape)
    canvas.init_seed(start, oc.init_activation)
    oc.seed[start] = oc.init_activation
    params = _lib.StepParams(oc.pad_value, oc.move_threshold, oc.disco_seed_threshold,
                             float(np.float32(ffn_oracle.logit(0.8))))
    # two candidates the steps paste over, one they never reach, one in the far corner
    cands = [tuple(s + d for s, d in zip(start, deltas)),
             tuple(s - d for s, d in zip(start, deltas)), (0, 0, 0),
             tuple(s - 1 for s in shape)]
    worst = 0.0
    for move in moves:
      pos = tuple(s + k * d for s, k, d in zip(start, move, deltas))
      req = _lib.StepRequest()
      req.pos[:] = pos
      req.start_pos[:] = start
      req.num_candidates = len(cands)
      for k, c in enumerate(cands):
        req.candidates[k][:] = c
      res = eng.step1(canvas, req, params)
      logits = oc.update_at(pos)
      scores, idx = ffn_oracle.face_maxima(deltas, logits)
      assert np.allclose(list(res.face_score), scores, atol=TOL), pos
      assert list(res.face_index) == [int(i) for i in idx], pos
      assert abs(res.start_logit - oc.seed[start]) <= TOL
      assert abs(int(res.num_deleted) - oc.last_deleted) <= oc.last_deleted_ties
      for k, c in enumerate(cands):
        a, b = res.cand_seed[k], oc.seed[c]
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= TOL, (pos, c)
        assert res.cand_seg[k] == 0
      got = canvas.read_seed()
      assert np.array_equal(np.isnan(got), np.isnan(oc.seed)), pos
      worst = max(worst, float(np.nanmax(np.abs(got - oc.seed))))
      assert worst <= TOL, pos
    _report(name, fov, depth, 'canvas, variant %d, %d steps' % (
        exp['default_variant'], len(moves)), worst)
    canvas.close()
  finally:
    eng.close()


def test_speculated_conv0a_on_layout_021():
  """test_speculative_conv0a_permuted_layout's check on the layout (0,2,1): a flood through
  a canvas of just over two FoVs per axis, the next step's conv0_a launched ahead or
  not -- the same steps, the same canvas."""
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd import synthetic
  from tests.test_gpu_round2 import _request
  _, fov, deltas, _ = fov_edges.BY_NAME['perm021_small']
  assert _expected(fov, 2)['oa'] == (0, 2, 1)
  m, _, _ = _model(fov, deltas, 2, seed=8, stddev=0.06)
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), m, m.info, None,
                                  inference_utils.Counters(), 1, device_id=0)
  eng = exe.engine
  try:
    r = _request()
    r.inference_options.move_threshold = 0.01  # below the pad value: every face moves
    shape = tuple(2 * f + 3 for f in fov)
    vol = synthetic.normalize(synthetic.cells_volume(shape, seed=3))
    out = {}
    for spec in (1, 0):
      eng.set_option('speculate', spec)
      eng.set_option('stat_reset', 0)
      counters = inference_utils.Counters()
      canvas = inference.DeviceCanvas(
          m.info, exe.get_client(counters, direct=True), vol, r.inference_options,
          counters=counters, movement_policy_fn=movement.get_policy_fn(r, m.info),
          keep_history=True)
      assert canvas._native_loop_ok()
      n = canvas.segment_at(tuple(s // 2 for s in shape))
      out[spec] = (n, [tuple(int(v) for v in p) for p in canvas.history],
                   np.array(np.asarray(canvas.seed)), eng.get_option('stat_spec_launched'),
                   eng.get_option('stat_spec_hits'))
      canvas.close()
    print('fov_edges perm021_small flood: %d steps, %d launched ahead, %d used' % (
        out[1][0], out[1][3], out[1][4]))
    assert out[1][0] == out[0][0] > 10
    assert out[1][1] == out[0][1]
    assert np.array_equal(out[1][2], out[0][2], equal_nan=True)
    assert out[0][3:] == (0, 0)
    assert out[1][3] > 0 and out[1][4] > 0
  finally:
    eng.close()


def test_range_fallback_to_conv32():
  """test_fp16_range_fallback where the exact-f32 kernel of the FoV is conv32 (variant 0:
  conv32c does not take rows of 57): a value beyond the fp16 range voids the step, and
  the repeat runs on conv32."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  name = 'perm021_tail7'
  _, fov, deltas, _ = fov_edges.BY_NAME[name]
  depth = 2
  exp = _expected(fov, depth)
  assert exp['default_variant'] == 9 and exp['exact_variant'] == 0
  m, _, blob = _model(fov, deltas, depth, seed=21)
  eng = hip_engine.HipEngine.from_model(m, max_batch=1)
  try:
    assert eng.get_option('conv_variant') == 9 and eng.get_option('exact_variant') == 0
    rng = np.random.RandomState(12)
    img = rng.normal(0, 1, (1,) + fov).astype(np.float32)
    seed = rng.normal(0, 2, (1,) + fov).astype(np.float32)
    ok = eng.predict(seed, img)
    assert eng.get_option('conv_variant') == 9  # ordinary data stays on fp16 pairs
    assert np.abs(ok - ffn_oracle.forward_f64c(img, seed, blob, depth)).max() <= TOL
    big = (img * 3e5).astype(np.float32)  # conv0_a outputs far beyond 65504
    got = eng.predict(seed, big)
    assert eng.get_option('conv_variant') == 0 == eng.get_option('exact_variant')
    want = ffn_oracle.forward(big, seed, blob, depth)
    assert np.isfinite(got).all()
    err = np.abs(got - want).max()
    _report(name, fov, depth, 'conv32 after the void, / max', err / np.abs(want).max())
    assert err <= 1e-5 * np.abs(want).max()
    again = eng.predict(seed, img)
    assert np.array_equal(again, eng.predict(seed, img))
    _report(name, fov, depth, 'conv32 against variant 9', np.abs(again - ok).max())
    assert np.abs(again - ok).max() <= 2e-5
    # canvas step: the voided step must leave the canvas untouched, then repeat
    eng.set_option('conv_variant', 9)
    lo = (4, 4, 4)
    hi = tuple(l + f for l, f in zip(lo, fov))
    vol = np.zeros(tuple(f + 7 for f in fov), np.float32)
    vol[tuple(slice(l, h) for l, h in zip(lo, hi))] = big[0]
    canvas = eng.create_canvas(vol)
    start = tuple(l + f // 2 for l, f in zip(lo, fov))
    canvas.init_seed(start, 2.9444386959)
    params = _lib.StepParams(-2.9444389343, 2.1972243786, 0.0)
    req = _lib.StepRequest()
    req.pos[:] = start
    req.start_pos[:] = start
    req.num_candidates = 0
    arr = (ctypes.c_void_p * 1)()
    arr[0] = canvas._h
    res = (_lib.StepResult * 1)()
    rc = _lib.load().ffn_canvas_step(eng._h, 1, arr, ctypes.byref(req), ctypes.byref(params),
                                     res)
    assert rc == _lib.ERR_RANGE and res[0].range_error == 1
    seed_now = canvas.read_seed()
    assert np.isnan(seed_now).sum() == seed_now.size - 1  # nothing was pasted
    eng.set_option('conv_variant', 9)
    r = eng.step1(canvas, req, params)  # the Python handle repeats the step
    assert eng.range_fallbacks == 1 and eng.get_option('conv_variant') == 0
    assert r.range_error == 0 and np.isfinite(r.start_logit)
    assert np.isfinite(canvas.read_seed(lo, hi)).all()
    canvas.close()
  finally:
    eng.close()


@pytest.mark.parametrize('fov,deltas', [((33, 33, 33), (8, 8, 8)), ((5, 5, 5), (1, 1, 1))])
def test_depth_one(fov, deltas):
  """conv0_a, conv0_b and the head alone: the exact-f32 kernels compute it, no fp16
  variant ever answers with logits."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  from ffn_amd import synthetic
  from oracle import ffn_oracle
  depth = 1
  exp = _expected(fov, depth)
  assert exp['default_variant'] == exp['exact_variant'] == 2 and not exp['d_ok']
  m, variables, blob = _model(fov, deltas, depth, seed=11, stddev=0.08)
  eng = hip_engine.HipEngine.from_model(m, max_batch=2)
  try:
    assert eng.get_option('conv_variant') == eng.get_option('exact_variant') == 2
    assert eng.get_option('flow') == 0
    rng = np.random.RandomState(1)
    img = rng.normal(0, 1, (2,) + fov).astype(np.float32)
    seed = rng.normal(0, 1.5, (2,) + fov).astype(np.float32)
    want = ffn_oracle.forward_f64c(img, seed, blob, depth)
    # two double-precision forwards differ by the rounding of their last bit to f32 at
    # the most: one ulp below 16 is 9.6e-7
    torch64 = ffn_oracle.forward_torch(img, seed, dict(variables), depth, f64=True)
    assert np.abs(want).max() < 16 and np.abs(want - torch64).max() <= 1e-6
    for variant in (0, 2):
      eng.set_option('conv_variant', variant)
      for n in (1, 2):
        err = np.abs(eng.predict(seed[:n], img[:n]) - want[:n]).max()
        _report('depth_one', fov, depth, 'variant %2d n %d' % (variant, n), err)
        assert err <= TOL, (variant, n)
    for variant in (6, 7, 8, 9, 10):
      with pytest.raises(_lib.FFNHipError):
        eng.set_option('conv_variant', variant)
        eng.predict(seed[:1], img[:1])
      eng.set_option('conv_variant', 2)
    if fov == (5, 5, 5):
      vol = synthetic.normalize(synthetic.cells_volume((13, 13, 13), seed=3))
      canvas = eng.create_canvas(vol)
      oc = ffn_oracle.OracleCanvas(vol, blob, depth, fov, deltas, ffn_oracle.Options())
      oc.forward_fn = lambda a, b: ffn_oracle.forward_f64c(a, b, blob, depth)
      start = (6, 6, 6)
      canvas.init_seed(start, oc.init_activation)
      oc.seed[start] = oc.init_activation
      params = _lib.StepParams(oc.pad_value, oc.move_threshold, oc.disco_seed_threshold)
      req = _lib.StepRequest()
      req.pos[:] = start
      req.start_pos[:] = start
      req.num_candidates = 0
      res = eng.step1(canvas, req, params)
      scores, idx = ffn_oracle.face_maxima(deltas, oc.update_at(start))
      assert np.allclose(list(res.face_score), scores, atol=TOL)
      assert list(res.face_index) == [int(i) for i in idx]
      got = canvas.read_seed()
      assert np.array_equal(np.isnan(got), np.isnan(oc.seed))
      err = float(np.nanmax(np.abs(got - oc.seed)))
      _report('depth_one', fov, depth, 'canvas step', err)
      assert err <= TOL
      canvas.close()
  finally:
    eng.close()
