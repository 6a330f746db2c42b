"""MovementRestrictor on the device (include/ffn_hip.h,
ffn_canvas_set_restrictor): the bit planes against tests/restriction_ref.py,
and restricted canvases through the library's segment loop, turn,
segment_many and the Runner against the Python loop and the reference run."""
import functools
import glob
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
from tests import restriction_ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIX = os.path.join(GOLDEN, 'ref_masks.npz')
WORK = ('update_at-calls', 'skip_restriced_pos', 'skip_threshold',
        'skip_invalid_pos', 'seed_got_too_weak', 'voxels-segmented')


class _Box:

  def __init__(self, start, size):
    self.start = np.array(start)
    self.end = self.start + np.array(size)


def _fixture_restrictor(g):
  return movement.MovementRestrictor(
      mask=g['run_mask'], seed_mask=g['run_seed_mask'], shift_mask=g['run_shift'],
      shift_mask_fov=_Box((-6, -6, -4), (13, 13, 9)), shift_mask_threshold=4,
      shift_mask_scale=2)


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


class PythonLoopCanvas(inference.DeviceCanvas):
  NATIVE_LOOP = False


def _canvas(exe, model, image, restrictor, cls=inference.DeviceCanvas, **kw):
  r = _options()
  counters = inference_utils.Counters()
  return cls(model.info, exe.get_client(counters, direct=True), image,
             r.inference_options, counters=counters, restrictor=restrictor,
             movement_policy_fn=movement.get_policy_fn(r, model.info), **kw)


def _record_segments(canvas):
  segs = []
  inner = canvas._segment_at_gen

  def gen(start_pos, partial_segment_iters=0):
    n = yield from inner(start_pos, partial_segment_iters)
    segs.append((tuple(int(v) for v in start_pos),
                 [tuple(int(v) for v in p) for p in canvas.history], n))
    return n

  canvas._segment_at_gen = gen
  return segs


# ---------------------------------------------------------------------------
# (a) the bit planes
# ---------------------------------------------------------------------------
def _shift_restrictor(shift, pre, post, scale, mask=None, seed_mask=None):
  """A stock restrictor whose reduced shift mask is `shift` != 0."""
  pre, post = np.array(pre), np.array(post)
  return movement.MovementRestrictor(
      mask=mask, seed_mask=seed_mask,
      shift_mask=None if shift is None else (np.asarray(shift) != 0)[None].astype(
          np.float32) * 5,
      shift_mask_fov=_Box(pre[::-1], (post - pre + 1)[::-1]),
      shift_mask_threshold=4, shift_mask_scale=scale)


def _cases():
  rng = np.random.RandomState(7)
  shape = (40, 36, 150)  # three words per row, the last one padded

  def sparse(s, p):
    return rng.rand(*s) < p

  return [
      ('scale1', shape, _shift_restrictor(sparse(shape, 0.002), (-4, -6, -6),
                                          (4, 6, 6), 1)),
      ('scale2_positive_zs_ne_z', shape, _shift_restrictor(
          sparse((30, 18, 75), 0.01), (2, 3, 1), (5, 7, 9), 2,
          mask=sparse(shape, 0.05), seed_mask=sparse(shape, 0.05))),
      ('scale3_negative', shape, _shift_restrictor(
          sparse((45, 12, 50), 0.01), (-10, -9, -7), (-1, -1, -1), 3)),
      ('past_high_edges', shape, _shift_restrictor(
          sparse((44, 20, 80), 0.003), (0, 20, 100), (50, 40, 200), 2)),
      ('mask_only', shape, movement.MovementRestrictor(mask=sparse(shape, 0.1))),
      ('seed_mask_only', shape,
       movement.MovementRestrictor(seed_mask=sparse(shape, 0.1))),
      ('nan_counts_as_set', shape, movement.MovementRestrictor(
          mask=np.where(sparse(shape, 0.1), np.nan, 0.0).astype(np.float32))),
  ]


def test_restriction_planes_match_the_definition(fib25_model):
  from ffn_amd import engine as hip_engine
  g = np.load(FIX)
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
  rng = np.random.RandomState(3)
  try:
    cases = _cases() + [('fixture', g['run_mask'].shape, _fixture_restrictor(g))]
    for name, shape, r in cases:
      args = inference._device_restriction(r, shape)
      assert args is not None, name
      want = restriction_ref.restriction(shape, **restriction_ref.restrictor_args(r))
      # the numpy restatement is the restrictor's own test
      for _ in range(400):
        p = tuple(int(rng.randint(0, s)) for s in shape)
        assert bool(want[p] & 1) == (not r.is_valid_pos(p)), (name, p)
        assert bool(want[p] & 2) == (not r.is_valid_seed(p)), (name, p)
      h = eng.create_canvas(np.zeros(shape, np.float32))
      h.set_restrictor(**args)
      got = h.read_restriction()
      assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5])
      lo, hi = (3, 5, 60), (17, 30, min(shape[2], 140))
      assert np.array_equal(h.read_restriction(lo, hi),
                            want[tuple(slice(l, u) for l, u in zip(lo, hi))]), name
      h.set_restrictor()  # cleared
      assert not h.read_restriction().any()
      h.close()
  finally:
    eng.close()


# ---------------------------------------------------------------------------
# (b) the reference's restricted run through the library's loop and turn
# ---------------------------------------------------------------------------
def test_restricted_reference_run_in_the_library(hip_exe, fib25_model):
  g = np.load(FIX)
  c = _canvas(hip_exe, fib25_model, synthetic.normalize(g['run_volume']),
              _fixture_restrictor(g), keep_history=True)
  assert c._native_loop_ok() and c._turn_ok()
  segs = _record_segments(c)
  c.segment_all(seed_policy=functools.partial(seed_lib.PolicyFixed,
                                              coords=g['run_seeds']))
  assert c.turns > 0
  steps = [p for s in segs for p in s[1]]
  assert steps == [tuple(int(v) for v in p) for p in g['run_steps']]
  assert np.array_equal(np.asarray(c.segmentation), g['run_segmentation'])
  ref = json.loads(str(g['run_counters']))
  for key in ('update_at-calls', 'skip_restriced_pos', 'skip_invalid_pos',
              'skip_threshold', 'voxels-segmented'):
    assert c.counters[key].value == ref[key], key
  c.close()


# ---------------------------------------------------------------------------
# (c) native vs Python loop on a synthetic volume with a three-part restrictor
# ---------------------------------------------------------------------------
def synthetic_restrictor(shape):
  """A slab plus a vertical cylinder (mask), a seed-mask box, an f32 shift
  field at scale 2 with patches >= 4 (FoV start (-6, -6, -4) xyz, size
  (13, 13, 9))."""
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


def test_native_and_python_loops_agree_under_a_restrictor(hip_exe, fib25_model):
  shape = (128, 128, 128)
  vol = synthetic.normalize(synthetic.cells_volume(shape, seed=11))
  runs = []
  for cls in (inference.DeviceCanvas, PythonLoopCanvas):
    c = _canvas(hip_exe, fib25_model, vol, synthetic_restrictor(shape), cls,
                keep_history=True)
    assert c._native_loop_ok() == (cls is inference.DeviceCanvas)
    assert c._turn_ok()
    segs = _record_segments(c)
    c.segment_all(seed_policy=seed_lib.PolicyPeaks)
    runs.append(dict(segs=segs, seg=np.array(np.asarray(c.segmentation)),
                     seed=np.array(c._handle.read_seed()), turns=c.turns,
                     counters={k: c.counters[k].value for k in WORK}))
    c.close()
  a, b = runs
  assert len(a['segs']) > 10 and a['turns'] > 10
  assert a['segs'] == b['segs']
  assert np.array_equal(a['seg'], b['seg'])
  assert np.array_equal(a['seed'], b['seed'], equal_nan=True)
  assert a['counters'] == b['counters']
  assert a['counters']['skip_restriced_pos'] > 0


# ---------------------------------------------------------------------------
# (d) MultiCanvasDriver: restricted canvases inside segment_many
# ---------------------------------------------------------------------------
def test_driver_runs_restricted_canvases_in_segment_many(fib25_model):
  from ffn_amd import engine as hip_engine
  from ffn_amd.inference import executor
  g = np.load(FIX)
  plain = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  jobs = [(g['run_volume'], g['run_seeds'], True),
          (plain['volume'], plain['seeds'], False),
          (g['run_volume'], g['run_seeds'], True),
          (plain['volume'], plain['seeds'], False)]
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None,
                                  inference_utils.Counters(), 4)
  try:
    hip_engine.pin_batched_arithmetic(exe.engine)

    def make(vol, restricted):
      return _canvas(exe, fib25_model, synthetic.normalize(vol),
                     _fixture_restrictor(g) if restricted else None)

    def result(c):
      return dict(seg=np.array(np.asarray(c.segmentation)),
                  seed=np.array(c._handle.read_seed()),
                  counters={k: c.counters[k].value for k in WORK})

    single = []
    for vol, seeds, restricted in jobs:
      c = make(vol, restricted)
      c.segment_all(seed_policy=functools.partial(seed_lib.PolicyFixed,
                                                  coords=seeds))
      single.append(result(c))
      c.close()
    canvases = [make(vol, restricted) for vol, _, restricted in jobs]
    through_many = set()
    inner = exe.engine.segment_many

    def segment_many(handles, *args, **kwargs):
      through_many.update(id(h) for h in handles)
      return inner(handles, *args, **kwargs)

    exe.engine.segment_many = segment_many
    drv = inference.MultiCanvasDriver(exe.engine, batch_size=4, native=True)
    drv.run((c, functools.partial(seed_lib.PolicyFixed, coords=seeds))
            for c, (_, seeds, _) in zip(canvases, jobs))
    for k, (c, want) in enumerate(zip(canvases, single)):
      got = result(c)
      assert id(c._handle) in through_many, k
      assert c.counters['segment_at-loop-calls'].value > 0, k
      assert np.array_equal(got['seg'], want['seg']), k
      assert np.array_equal(got['seed'], want['seed'], equal_nan=True), k
      assert got['counters'] == want['counters'], k
      if jobs[k][2]:
        assert np.array_equal(got['seg'], g['run_segmentation']), k
      c.close()
  finally:
    exe.engine.close()


# ---------------------------------------------------------------------------
# (e) reassignment, subclasses
# ---------------------------------------------------------------------------
def test_restrictor_reassignment_reuploads(hip_exe, fib25_model):
  g = np.load(FIX)
  c = _canvas(hip_exe, fib25_model, synthetic.normalize(g['run_volume']), None)
  assert c._native_loop_ok() and not c._handle.read_restriction().any()
  c.restrictor = _fixture_restrictor(g)
  assert c._native_loop_ok() and c._turn_ok()
  want = restriction_ref.restriction(
      c.shape, **restriction_ref.restrictor_args(c.restrictor))
  assert np.array_equal(c._handle.read_restriction(), want)

  class Custom(movement.MovementRestrictor):
    pass

  c.restrictor = Custom(mask=g['run_mask'])
  assert not c._native_loop_ok() and not c._turn_ok()
  assert not c._handle.read_restriction().any()
  c.restrictor = movement.MovementRestrictor(mask=g['run_mask'])
  assert c._native_loop_ok()
  c.restrictor.mask = np.zeros_like(g['run_mask'])
  assert c._handle.read_restriction().any()  # the device holds a snapshot
  c.refresh_restrictor()
  assert not c._handle.read_restriction().any()
  c.close()


# ---------------------------------------------------------------------------
# (f) Runner with npy masks / seed masks / shift mask
# ---------------------------------------------------------------------------
def _restricted_request(g, tmp_path, out_dir):
  vol_path = str(tmp_path / 'vol.npy')
  np.save(vol_path, g['run_volume'])
  np.save(tmp_path / 'mask.npy', g['run_mask'].astype(np.uint8))
  np.save(tmp_path / 'seed_mask.npy', g['run_seed_mask'].astype(np.uint8))
  np.save(tmp_path / 'shift.npy', g['run_shift'])
  weights = os.path.join(GOLDEN, 'fib25_weights.npz')
  seeds = json.dumps({'coords': g['run_seeds'].tolist()}).replace('"', '\\"')
  text = '''
    image { npy: "%s" }
    image_mean: 128
    image_stddev: 33
    seed_policy: "PolicyFixed"
    seed_policy_args: "%s"
    model_checkpoint_path: "%s"
    model_name: "convstack_3d.ConvStack3DFFNModel"
    model_args: "{\\"depth\\": 12, \\"fov_size\\": [33, 33, 33], \\"deltas\\": [8, 8, 8]}"
    segmentation_output_dir: "%s"
    masks { volume { mask { npy: "%s" } channels { channel: 0 values: 1 } } }
    seed_masks { volume { mask { npy: "%s" } channels { channel: 0 values: 1 } } }
    shift_mask { npy: "%s" }
    shift_mask_scale: 2
    shift_mask_fov { start { x: -6 y: -6 z: -4 } size { x: 13 y: 13 z: 9 } }
    inference_options {
      init_activation: 0.95
      pad_value: 0.05
      move_threshold: 0.9
      min_boundary_dist { x: 1 y: 1 z: 1}
      segment_threshold: 0.6
      min_segment_size: 1000
    }''' % (vol_path, seeds, weights, out_dir, tmp_path / 'mask.npy',
            tmp_path / 'seed_mask.npy', tmp_path / 'shift.npy')
  return req_lib.request_from_text(text)


def test_runner_with_masks_runs_in_the_library(fib25_model, tmp_path, monkeypatch):
  from ffn_amd.inference import runner as runner_lib
  g = np.load(FIX)
  out = []
  for native in (True, False):
    monkeypatch.setattr(inference.DeviceCanvas, 'NATIVE_LOOP', native)
    out_dir = str(tmp_path / ('out%d' % native))
    runner = runner_lib.Runner()
    runner.start(_restricted_request(g, tmp_path, out_dir))
    canvas = runner.run((0, 0, 0), tuple(g['run_volume'].shape))
    assert canvas._native_loop_ok() == native
    assert canvas.__dict__.get('_restrict_on')
    assert canvas.counters['segment_at-loop-calls'].value > 0
    assert canvas.counters['skip_restriced_pos'].value > 0
    runner.stop_executor()
    files = glob.glob(os.path.join(out_dir, '**', 'seg-*.npz'), recursive=True)
    assert len(files) == 1
    with np.load(files[0], allow_pickle=True) as d:
      out.append((np.array(d['segmentation']), d['origins'].item()))
  assert np.array_equal(out[0][0], out[1][0])
  assert out[0][0].max() > 0
  assert sorted(out[0][1]) == sorted(out[1][1])
  for k in out[0][1]:
    assert tuple(out[0][1][k].start_zyx) == tuple(out[1][1][k].start_zyx)
    assert out[0][1][k].iters == out[1][1][k].iters
