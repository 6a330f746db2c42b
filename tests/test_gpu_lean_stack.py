"""The resident stack (conv32ps_kernel) and the fused step launch exist in two forms: the
production form, which a step runs unless told otherwise, and the LAB form with the lab's
run-time plumbing (debug_clock, debug_layer, flow_debug, debug_fused_trace, the flow
trace).  Engine option flow_lab = 1 forces the LAB form; stat_lab_launches counts the
resident stacks queued in it.  Both forms run the same bodies: the same bits as each other
and as one launch per conv, on every geometry the resident launch takes.
"""

import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

# the smallest resident-launch geometries of test_resident_stack_same_bits_as_per_layer_launches
# (conv32mt: 256 main chunks + 32-voxel tail workgroups; the last one on the permuted layout)
GEOMS = [([33, 33, 33], [8, 8, 8]), ([35, 33, 31], [8, 8, 7]), ([41, 41, 21], [10, 10, 5])]
DEPTH = 3  # 5 convs: the first, an odd, an even and the last body of either role


def _three_ways(eng, seed, img):
  """logits of the production form, the LAB form and the per-layer launches"""
  assert eng.get_option('conv_variant') == 9 and eng.get_option('flow') == 2
  assert eng.get_option('flow_lab') == 0
  out = {}
  for lab in (0, 1, 0):
    eng.set_option('flow_lab', lab)
    eng.set_option('stat_reset', 0)
    got = eng.predict(seed, img)
    launches = eng.get_option('stat_lab_launches')
    assert (launches > 0) == bool(lab), (lab, launches)
    if lab in out:
      assert np.array_equal(got, out[lab])
    out[lab] = got
  eng.set_option('flow', 0)
  eng.set_option('stat_reset', 0)
  out['layers'] = eng.predict(seed, img)
  assert eng.get_option('stat_lab_launches') == 0  # (no resident launch at all)
  eng.set_option('flow', 2)
  assert eng.get_option('stat_flow_timeouts') == 0
  return out


@pytest.mark.parametrize('fov_xyz,deltas_xyz', GEOMS)
def test_production_and_lab_form_same_bits_as_per_layer_launches(fov_xyz, deltas_xyz):
  from ffn_amd import engine as hip_engine
  from ffn_amd.training.models import convstack_3d
  from oracle import ffn_oracle
  m = convstack_3d.ConvStack3DFFNModel(fov_size=fov_xyz, deltas=deltas_xyz, depth=DEPTH)
  m.set_variables(ffn_oracle.random_weights(DEPTH, seed=40 + DEPTH, stddev=0.05))
  eng = hip_engine.HipEngine.from_model(m, max_batch=1)
  try:
    zyx = fov_xyz[::-1]
    rng = np.random.RandomState(17)
    for trial in range(2):
      img = rng.normal(0, 1, [1] + zyx).astype(np.float32)
      seed = rng.normal(0, 1.5, [1] + zyx).astype(np.float32)
      out = _three_ways(eng, seed, img)
      assert np.isfinite(out[0]).all() and out[0].std() > 0
      assert np.array_equal(out[0], out[1]), trial
      assert np.array_equal(out[0], out['layers']), trial
  finally:
    eng.close()


def test_fib25_weights_same_bits(fib25_model):
  from ffn_amd import engine as hip_engine
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
  try:
    rng = np.random.RandomState(23)
    img = ((rng.randint(0, 256, (1, 33, 33, 33)).astype(np.float32)) - 128) / 33
    seed = rng.normal(0, 1.5, (1, 33, 33, 33)).astype(np.float32)
    out = _three_ways(eng, seed, img)
    assert np.array_equal(out[0], out[1])
    assert np.array_equal(out[0], out['layers'])
  finally:
    eng.close()


@pytest.mark.parametrize('option,value', [('debug_clock', 1), ('debug_clock', 2),
                                          ('flow_debug', 1), ('debug_layer', 1)])
def test_lab_options_run_the_lab_form(option, value):
  """What the production form has no code for must reach the kernel that has: the clock
  stamps, the flow_debug bits (the fault injection of tests/test_gpu_round5.py among
  them) and the traces stay meaningful only while setting them selects the LAB form."""
  from ffn_amd import engine as hip_engine
  from ffn_amd.training.models import convstack_3d
  from oracle import ffn_oracle
  m = convstack_3d.ConvStack3DFFNModel(fov_size=[33, 33, 33], deltas=[8, 8, 8], depth=DEPTH)
  m.set_variables(ffn_oracle.random_weights(DEPTH, seed=7, stddev=0.05))
  eng = hip_engine.HipEngine.from_model(m, max_batch=1)
  try:
    rng = np.random.RandomState(3)
    img = rng.normal(0, 1, (1, 33, 33, 33)).astype(np.float32)
    seed = rng.normal(0, 1.5, (1, 33, 33, 33)).astype(np.float32)
    eng.set_option('stat_reset', 0)
    plain = eng.predict(seed, img)
    assert eng.get_option('stat_lab_launches') == 0
    default = eng.get_option(option)
    eng.set_option(option, value)
    got = eng.predict(seed, img)
    assert eng.get_option('stat_lab_launches') > 0
    assert np.array_equal(got, plain)
    eng.set_option(option, default)
    eng.set_option('stat_reset', 0)
    assert np.array_equal(eng.predict(seed, img), plain)
    assert eng.get_option('stat_lab_launches') == 0
  finally:
    eng.close()


def test_segment_loop_same_steps_and_canvas_bytes(fib25_model):
  """One segment of the cells56 fixture through ffn_canvas_segment_at (speculative
  conv0_a, the stack queued ahead, the fused step launch: the shipped defaults) with the
  production forms and with the LAB forms: the same positions, the same canvas."""
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference_utils
  from tests.test_gpu_round2 import _assert_shipped_default, _device_canvas
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  image = synthetic.normalize(g['volume'])
  start = tuple(int(v) for v in g['seeds'][0])
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None, inference_utils.Counters(), 1,
                                  device_id=0)
  eng = exe.engine
  try:
    _assert_shipped_default(eng)
    runs = {}
    for lab in (0, 1):
      eng.set_option('flow_lab', lab)
      eng.set_option('stat_reset', 0)
      canvas = _device_canvas(exe, fib25_model, image, keep_history=True)
      assert canvas._native_loop_ok()
      n = canvas.segment_at(start)
      launches = eng.get_option('stat_lab_launches')
      assert (launches > 0) == bool(lab), (lab, launches)
      runs[lab] = (n, list(canvas.history), np.asarray(canvas.seed).tobytes(),
                   np.asarray(canvas.segmentation).tobytes())
      canvas.close()
    assert runs[0][0] == runs[1][0] > 1
    assert runs[0][1] == runs[1][1]
    assert runs[0][2] == runs[1][2] and runs[0][3] == runs[1][3]
    assert eng.get_option('stat_flow_timeouts') == 0
  finally:
    eng.set_option('flow_lab', 0)
    eng.close()
