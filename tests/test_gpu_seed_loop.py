"""ffn_canvas_segment_all on the device: `DeviceCanvas.segment_all` through the
library's seed loop against the reference-minted run and against the Python seed
loop (`_segment_all_gen`) on the same engine, with and without a restrictor."""
import functools
import json
import os

import numpy as np
import pytest

from ffn_amd import synthetic
from ffn_amd.inference import inference
from ffn_amd.inference import inference_utils
from ffn_amd.inference import movement
from ffn_amd.inference import request as req_lib
from ffn_amd.inference import seed as seed_lib
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _options():
  r = req_lib.InferenceRequest()
  o = r.inference_options
  o.init_activation, o.pad_value, o.move_threshold = 0.95, 0.05, 0.9
  o.segment_threshold, o.min_segment_size = 0.6, 1000
  o.min_boundary_dist.x = o.min_boundary_dist.y = o.min_boundary_dist.z = 1
  return r


@pytest.fixture(scope='module')
def hip_exe(fib25_model):
  from ffn_amd.inference import executor
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None,
                                  inference_utils.Counters(), 1, device_id=0)
  yield exe
  exe.engine.close()


class PythonSeedLoopCanvas(inference.DeviceCanvas):
  NATIVE_SEED_LOOP = False


def _canvas(exe, model, image, cls=inference.DeviceCanvas, **kw):
  r = _options()
  counters = inference_utils.Counters()
  return cls(model.info, exe.get_client(counters, direct=True), image,
             r.inference_options, counters=counters,
             movement_policy_fn=movement.get_policy_fn(r, model.info), **kw)


def _state(c):
  return {
      'segmentation': np.array(np.asarray(c.segmentation)),
      'seed': np.array(c._handle.read_seed()).view(np.uint32),
      'origins': {k: (tuple(int(x) for x in v.start_zyx), int(v.iters))
                  for k, v in c.origins.items()},
      'overlaps': {k: np.asarray(v).tolist() for k, v in c.overlaps.items()},
      'max_id': c._max_id, 'idx': c.seed_policy.idx, 'gate_rejects': c.gate_rejects,
      'counters': {k: t.value for k, t in c.counters if not k.endswith('-time-ms')},
  }


def _both(exe, model, image, policy, **kw):
  """One pass through the library's seed loop and one forced onto the Python seed
  loop, same engine -> the first canvas' state, both compared."""
  out = []
  mismatch = exe.engine.get_option('stat_spec_mismatch')
  for cls in (inference.DeviceCanvas, PythonSeedLoopCanvas):
    c = _canvas(exe, model, image, cls, **kw)
    assert c._native_loop_ok() and c._turn_ok()
    c.segment_all(seed_policy=policy)
    out.append((c.__dict__.get('seed_loop_calls', 0), c.turns, _state(c)))
    c.close()
  (ncalls, nturns, ns), (pcalls, pturns, ps) = out
  assert ncalls > 0 and pcalls == 0  # the new call was taken, and only where meant
  assert nturns > 0 and pturns > 0
  assert ns.keys() == ps.keys()
  for key in ns:
    if isinstance(ns[key], np.ndarray):
      assert np.array_equal(ns[key], ps[key]), key
    else:
      assert ns[key] == ps[key], key
  assert exe.engine.get_option('stat_spec_mismatch') == mismatch == 0
  return ns


def test_seed_loop_reproduces_reference_run(hip_exe, fib25_model):
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  c = _canvas(hip_exe, fib25_model, synthetic.normalize(g['volume']))
  c.segment_all(seed_policy=functools.partial(seed_lib.PolicyFixed,
                                              coords=g['seeds']))
  assert c.seed_loop_calls > 0
  assert np.array_equal(np.asarray(c.segmentation), g['segmentation'])
  ref = json.loads(str(g['counters']))
  for key in ('update_at-calls', 'voxels-segmented', 'voxels-overlapping',
              'skip_invalid_pos', 'skip_threshold', 'seed_got_too_weak',
              'segment_at-loop-calls', 'seed-policy-calls', 'segment_all-calls'):
    if key in ref:
      assert c.counters[key].value == ref[key], key
  c.close()


def test_seed_loop_equals_python_seed_loop(hip_exe, fib25_model):
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  st = _both(hip_exe, fib25_model, synthetic.normalize(g['volume']),
             functools.partial(seed_lib.PolicyFixed, coords=g['seeds']))
  assert st['counters']['update_at-calls'] > 0 and st['max_id'] > 0


class _Box:

  def __init__(self, start, size):
    self.start = np.array(start)
    self.end = self.start + np.array(size)


def _restrictor(shape):
  """tests/test_gpu_restrictor.py's synthetic restrictor: a slab plus a cylinder
  (mask), a seed-mask box, an f32 shift field at scale 2."""
  z, y, x = np.indices(shape)
  zc, yc, xc = shape[0] // 2, shape[1] // 3, (2 * shape[2]) // 3
  mask = ((z >= zc) & (z < zc + 4)) | (
      (y - yc) ** 2 + (x - xc) ** 2 <= (shape[1] // 16) ** 2)
  seed_mask = np.zeros(shape, bool)
  seed_mask[shape[0] // 10:shape[0] // 3, shape[1] // 10:shape[1] // 2,
            shape[2] // 10:shape[2] // 2] = True
  shift = np.zeros((2, shape[0], shape[1] // 2, shape[2] // 2), np.float32)
  shift[0, (3 * shape[0]) // 4:(3 * shape[0]) // 4 + 6, 10:16, 20:26] = 5.0
  shift[1, shape[0] // 5:shape[0] // 5 + 4, shape[1] // 3:shape[1] // 3 + 4,
        4:8] = -4.0
  return movement.MovementRestrictor(
      mask=mask, seed_mask=seed_mask, shift_mask=shift,
      shift_mask_fov=_Box((-6, -6, -4), (13, 13, 9)), shift_mask_threshold=4,
      shift_mask_scale=2)


def test_restricted_seed_loop_equals_python_seed_loop(hip_exe, fib25_model):
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  shape = g['volume'].shape
  # the fixture's seeds, then a grid: some vetoed, some segmented, some too close
  grid = np.array(list(g['seeds']) +
                  [(z, y, x) for z in range(16, 40, 6) for y in range(16, 40, 6)
                   for x in range(16, 40, 6)])
  st = _both(hip_exe, fib25_model, synthetic.normalize(g['volume']),
             functools.partial(seed_lib.PolicyFixed, coords=grid),
             restrictor=_restrictor(shape))
  assert st['idx'] == len(grid) and st['counters']['update_at-calls'] > 0
