"""GPU tests added in round 2: parity at the BASELINE size, uint8 canvases,
checkpoint resume on the device, the CLI end to end.  All through the C-ABI.
"""

import functools
import json
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _request():
  from ffn_amd.inference import request as req_lib
  r = req_lib.InferenceRequest()
  r.image_mean = 128
  r.image_stddev = 33
  o = r.inference_options
  o.init_activation = 0.95
  o.pad_value = 0.05
  o.move_threshold = 0.9
  o.segment_threshold = 0.6
  o.min_segment_size = 1000
  o.min_boundary_dist.x = 1
  o.min_boundary_dist.y = 1
  o.min_boundary_dist.z = 1
  return r


@pytest.fixture(scope='module')
def hip_exe(fib25_model):
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference_utils
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None,
                                  inference_utils.Counters(), 1, device_id=0)
  yield exe
  exe.engine.close()


def _assert_shipped_default(eng):
  """The engine is in the state a fresh one ships in for the 33^3 FIB-25 model:
  conv32mt for a single FoV, run as ONE resident launch (flow 2), nothing chosen
  explicitly, next conv0_a (and the stack behind it) launched ahead, faces + paste fused."""
  assert eng.get_option('conv_variant') == 9
  assert not eng.variant_is_explicit
  assert eng.get_option('flow') == 2
  assert eng.get_option('speculate') == 1
  assert eng.get_option('fuse_paste') == 1
  assert eng.get_option('fuse_conv0a') == 1
  assert eng.get_option('stack_ahead') == 1  # (round 6: the next stack queued ahead too)


def _device_canvas(exe, model, image, **kwargs):
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  r = _request()
  counters = inference_utils.Counters()
  return inference.DeviceCanvas(
      model.info, exe.get_client(counters, direct=True), image,
      r.inference_options, counters=counters,
      movement_policy_fn=movement.get_policy_fn(r, model.info), **kwargs)


# ---------------------------------------------------------------------------
# N1: the BASELINE-size workload against reference-minted fixtures
# ---------------------------------------------------------------------------
# Every FoV step feeds its logits back into the inputs of later steps, so float
# noise is not only added up: where the object map is undecided it is amplified
# (x1000 over a few hundred steps on this phantom) until a threshold decision
# flips.  Two CORRECT f32 CPU implementations of the conv stack therefore do not
# stay on one trajectory (tools/cpu_f32_order_sensitivity.py,
# profiles/r02_f32_order_sensitivity.txt): the C oracle's sequential fmaf chain
# and torch-CPU / oneDNN part ways at step 1554 of 3,658 / 3,725.  Fixtures:
#   ref_canvas_cells250.npz         reference Canvas + C oracle forward
#   ref_canvas_cells250_onednn.npz  reference Canvas + torch-oneDNN f32 forward
#   ref_canvas_cells250_f64.npz     reference Canvas + f64 forward
# The oneDNN-f32 and the f64 runs are ONE trajectory (tests/test_oracle.py).  The
# exact-f32 kernel (variant 2) sums in the oracle's order and reproduces the
# first fixture; the split-product kernels (f32 accumulation of exact 16-term
# products) reproduce the oneDNN / f64 run -- step for step, voxel for voxel.
_FIXTURE_OF_VARIANT = {2: '', 6: '_f64', 8: '_f64', 9: '_f64'}
# move scores and seed logits ALONG a run, against the fixture of the trajectory the
# kernel is on: the per-step bound holds for the whole run (measured over the 3,725
# steps of the 250^3 runs: 1.9e-5 - 2.0e-5, final seed logits 5.8e-6; the pred < seed
# runs 1.4e-5; profiles/r04_pytest_gpu_run_tolerance.txt)
RUN_TOL = 1e-4


def _run_recorded(canvas, seeds):
  got_steps, got_moves = [], []
  thr = canvas.movement_policy.score_threshold
  deltas = canvas.movement_policy.deltas
  inner = canvas.update_at

  def recording_update(pos):
    pred = inner(pos)
    got_steps.append(tuple(int(v) for v in pos))
    got_moves.append(sorted(
        ((s, tuple(int(v) + int(p) for v, p in zip(o, pos)))
         for s, o, _ in pred.scored_move_offsets(deltas, thr)), reverse=True))
    return pred

  canvas.update_at = recording_update
  canvas.segment_all(seed_policy=functools.partial(seed_lib_fixed(), coords=seeds))
  return got_steps, got_moves


def seed_lib_fixed():
  from ffn_amd.inference import seed as seed_lib
  return seed_lib.PolicyFixed


def _check_against_fixture(canvas, g):
  seg = np.asarray(canvas.segmentation)
  want = g['segmentation'].astype(np.int32)
  inter = np.sum((seg > 0) & (want > 0) & (seg == want))
  union = np.sum((seg > 0) | (want > 0))
  assert inter == union, 'IoU %.6f' % (inter / max(union, 1))
  assert np.array_equal(seg, want)  # the -1 markers too
  ref_c = json.loads(str(g['counters']))
  for key in ('update_at-calls', 'voxels-segmented', 'voxels-overlapping',
              'skip_invalid_pos', 'segment_at-loop-calls'):
    assert canvas.counters[key].value == ref_c[key], key
  origins = json.loads(str(g['origins']))
  assert {int(k): [list(v.start_zyx), v.iters]
          for k, v in canvas.origins.items()} == {
              int(k): v for k, v in origins.items()}


@pytest.mark.parametrize('variant,flow', [(2, 0), (6, 0), (8, 0), (9, 0), (9, 1),
                                          (9, 2)])
def test_cells250_matches_reference_minted_run(hip_exe, fib25_model, variant, flow):
  """configs[1] at full size: the 250^3 phantom bench.py runs, first row of its
  seed grid.  The fixtures were minted by the reference's own Canvas
  (tools/make_golden.py --only cells250 [--forward onednn]); the GPU must visit
  the same FoV positions in the same order, queue the same moves and commit the
  same segment ids voxel for voxel (IoU 1.0)."""
  path = os.path.join(GOLDEN, 'ref_canvas_cells250%s.npz' %
                      _FIXTURE_OF_VARIANT[variant])
  if not os.path.exists(path):
    pytest.skip('fixture not minted')
  import hashlib
  from ffn_amd import synthetic
  g = np.load(path)
  vol = synthetic.cells_volume((250, 250, 250), seed=1234)
  assert hashlib.sha256(vol.tobytes()).hexdigest() == str(g['volume_sha256'])
  eng = hip_exe.engine
  eng.set_option('conv_variant', variant)
  # (9, 2) is what ships: conv32mt as one resident launch per step; (9, 0) its
  # per-layer launches, (9, 1) those with the flagged hand-off compiled in
  eng.set_option('flow', flow)
  try:
    canvas = _device_canvas(hip_exe, fib25_model, synthetic.normalize(vol))
    got_steps, got_moves = _run_recorded(canvas, g['seeds'])
    want_steps = [tuple(int(v) for v in p) for p in g['steps']]
    n = min(len(got_steps), len(want_steps))
    first_bad = next((k for k in range(n) if got_steps[k] != want_steps[k]),
                     None)
    assert first_bad is None and len(got_steps) == len(want_steps), (
        'variant %d: trajectory leaves the reference at step %s of %d / %d' %
        (variant, first_bad, len(got_steps), len(want_steps)))
    # queued moves: same targets; scores within the run-level tolerance
    off = 0
    max_err = 0.0
    for k, moves in enumerate(got_moves):
      nm = int(g['n_moves'][k])
      assert len(moves) == nm, k
      for j, (s, c) in enumerate(moves):
        assert c == tuple(int(v) for v in g['move_coords'][off + j]), (k, j)
        max_err = max(max_err, abs(s - float(g['move_scores'][off + j])))
      off += nm
    assert max_err <= (TOL if variant == 2 else RUN_TOL), max_err
    _check_against_fixture(canvas, g)
    sample = np.asarray(canvas.seed[0:33, 0:33, 192:225])
    want_s = g['final_seed_sample']
    assert np.array_equal(np.isnan(sample), np.isnan(want_s))
    seed_err = float(np.nanmax(np.abs(sample - want_s)))
    print('variant %d flow %d: %d steps, max move-score difference along the run '
          '%.3g, final seed sample %.3g' % (variant, flow, len(got_steps), max_err,
                                            seed_err))
    assert seed_err <= (TOL if variant == 2 else RUN_TOL)
    assert eng.get_option('stat_flow_timeouts') == 0
    canvas.close()
  finally:
    eng.restore_default_variant()
    eng.set_option('flow', 2)


def test_cells250_logit_tolerance_on_canvas_states(hip_exe, fib25_model):
  """The float tolerance, at the BASELINE size and on REAL canvas states: the
  (image, seed) FoVs in front of every 150th step of the reference run go
  through the stateless predict with every kernel; all agree with the exact-f32
  kernel within 2e-5 (observed <= 1e-5), i.e. well inside TOL = 1e-4."""
  path = os.path.join(GOLDEN, 'ref_canvas_cells250.npz')
  if not os.path.exists(path):
    pytest.skip('fixture not minted')
  from ffn_amd import synthetic
  g = np.load(path)
  vol = synthetic.cells_volume((250, 250, 250), seed=1234)
  image = synthetic.normalize(vol)
  eng = hip_exe.engine
  eng.set_option('conv_variant', 2)
  samples = []

  class _Stop(Exception):
    pass

  try:
    canvas = _device_canvas(hip_exe, fib25_model, image)
    pad = np.float32(canvas.options.pad_value)
    inner = canvas.update_at
    count = [0]

    def rec(pos):
      k = count[0]
      if k % 150 == 0:
        sl = tuple(slice(int(p) - 16, int(p) + 17) for p in pos)
        seed = np.array(canvas.seed[sl], np.float32)
        samples.append((k, image[sl].copy(),
                        np.where(np.isnan(seed), pad, seed).astype(np.float32)))
      count[0] += 1
      if k >= 1600:
        raise _Stop()
      return inner(pos)

    canvas.update_at = rec
    try:
      canvas.segment_all(seed_policy=functools.partial(seed_lib_fixed(),
                                                       coords=g['seeds']))
    except _Stop:
      pass
    canvas.close()
    assert len(samples) >= 10
    worst = {}
    for k, img, seed in samples:
      eng.set_option('conv_variant', 2)
      ref = eng.predict(seed[None], img[None])[0]
      for v in (6, 8, 9):
        eng.set_option('conv_variant', v)
        err = float(np.abs(eng.predict(seed[None], img[None])[0] - ref).max())
        worst[v] = max(worst.get(v, 0.0), err)
    print('max |logit - exact f32 kernel| on canvas states:', worst)
    assert max(worst.values()) <= 2e-5, worst
  finally:
    eng.restore_default_variant()
    eng.set_option('flow', 2)


def test_cells250_native_loop_same_result(hip_exe, fib25_model):
  """The same workload through ffn_canvas_segment_at (the default drive of
  bench.py / Runner.run) with the default kernel: final segmentation, origins
  and counters of the reference-minted (oneDNN forward) run."""
  path = os.path.join(GOLDEN, 'ref_canvas_cells250_onednn.npz')
  if not os.path.exists(path):
    pytest.skip('fixture not minted')
  from ffn_amd import synthetic
  g = np.load(path)
  vol = synthetic.cells_volume((250, 250, 250), seed=1234)
  _assert_shipped_default(hip_exe.engine)
  canvas = _device_canvas(hip_exe, fib25_model, synthetic.normalize(vol))
  assert canvas._native_loop_ok()
  canvas.segment_all(seed_policy=functools.partial(seed_lib_fixed(),
                                                   coords=g['seeds']))
  _check_against_fixture(canvas, g)
  canvas.close()


# ---------------------------------------------------------------------------
# uint8 canvases (ffn_canvas_create_u8)
# ---------------------------------------------------------------------------
def test_u8_canvas_bit_identical_to_f32_canvas(hip_exe, fib25_model):
  """Normalisation in the FoV gather == normalisation on the host
  (runner.py:383-385): same step results, same seed array, same PolicyPeaks
  seeds, bit for bit -- for a mean / stddev that are not exact in f32 too."""
  from ffn_amd import _lib
  from ffn_amd import seeding
  from ffn_amd import synthetic
  from ffn_amd.inference import inference
  from oracle import ffn_oracle
  eng = hip_exe.engine
  vol = synthetic.cells_volume((64, 72, 80), seed=9)
  for mean, std in ((128.0, 33.0), (127.3, 28.9)):
    img = (vol.astype(np.float32) - mean) / std
    a = eng.create_canvas(img)
    b = eng.create_canvas(inference.NormalizedU8Image(vol, mean, std))
    assert b.is_u8 and not a.is_u8
    params = _lib.StepParams(ffn_oracle.f32_logit(0.05),
                             ffn_oracle.f32_logit(0.9), 0.0)
    pos0 = (30, 36, 40)
    for h in (a, b):
      h.init_seed(pos0, ffn_oracle.f32_logit(0.95))
    for pos in (pos0, (30, 36, 48), (38, 36, 40), (30, 44, 44)):
      req = _lib.StepRequest()
      req.pos[:] = pos
      req.start_pos[:] = pos0
      req.num_candidates = 0
      ra = eng.step1(a, req, params)
      fa = (list(ra.face_score), list(ra.face_index), ra.start_logit,
            ra.num_above_move)
      rb = eng.step1(b, req, params)
      fb = (list(rb.face_score), list(rb.face_index), rb.start_logit,
            rb.num_above_move)
      assert fa == fb, pos
    sa, sb = a.read_seed(), b.read_seed()
    assert np.array_equal(sa, sb, equal_nan=True)
    assert np.sum(~np.isnan(sa)) > 33**3
    s = seeding.default_seeder(0)
    pa = s.peaks_canvas(a)
    pb = s.peaks_canvas(b)
    assert len(pa) > 10 and np.array_equal(pa, pb)
    a.close()
    b.close()


def test_runner_uses_u8_canvas_for_raw_volumes(fib25_model, tmp_path):
  """Runner.make_canvas hands raw uint8 data to the device (DEVICE_U8) and the
  result is the one of the host-normalised path."""
  from ffn_amd.inference import inference
  from ffn_amd.inference import runner as runner_lib
  from tests.test_gpu_parity import _runner_request_text
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  segs = []
  for device_u8 in (True, False):
    out_dir = str(tmp_path / ('out%d' % device_u8))
    request = _runner_request_text(g, tmp_path, out_dir)
    runner = runner_lib.Runner()
    runner.DEVICE_U8 = device_u8
    runner.start(request)
    canvas = runner.run((0, 0, 0), tuple(g['volume'].shape))
    assert isinstance(canvas.image, inference.NormalizedU8Image) == device_u8
    segs.append(np.asarray(canvas.segmentation).copy())
    runner.stop_executor()
  assert np.array_equal(segs[0], segs[1])
  assert np.array_equal(segs[0], g['segmentation'])


# ---------------------------------------------------------------------------
# .cpoint on the real device (f3)
# ---------------------------------------------------------------------------
def test_mid_segment_checkpoint_resume_on_device(hip_exe, fib25_model, tmp_path):
  """Saved mid-segment from the device canvas, the canvas destroyed, restored
  into a fresh DeviceCanvas, finished: equal to the uninterrupted run and to
  the reference-minted fixture (inference.py:728-843, runner.py:505-519)."""
  from ffn_amd import synthetic
  from tests import resume_case
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  image = synthetic.normalize(g['volume'])

  def make(path, interval):
    return _device_canvas(hip_exe, fib25_model, image, checkpoint_path=path,
                          checkpoint_interval_sec=interval)

  a, b, meta = resume_case.run_resume_case(make, g['seeds'], 30, tmp_path)
  assert meta['partial_segment_iters'] > 0
  resume_case.assert_same_final_state(a, b)
  assert np.array_equal(np.asarray(b.segmentation), g['segmentation'])
  a.close()
  b.close()


def test_runner_resumes_from_cpoint_and_removes_it(fib25_model, tmp_path):
  """Runner.run: an existing .cpoint is restored, the run finishes with the
  uninterrupted result and the checkpoint file is removed (runner.py:505-542)."""
  from ffn_amd.inference import runner as runner_lib
  from ffn_amd.inference import seed as seed_lib
  from ffn_amd.inference import storage
  from tests.test_gpu_parity import _runner_request_text
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  out_dir = str(tmp_path / 'out')
  request = _runner_request_text(g, tmp_path, out_dir)
  runner = runner_lib.Runner()
  runner.start(request)
  # leg 1: a canvas killed after 30 FoV steps, checkpointing every step
  canvas, _ = runner.make_canvas((0, 0, 0), tuple(g['volume'].shape))
  canvas.checkpoint_interval_sec = 1e-9
  steps = [0]
  inner = canvas.update_at

  class _Kill(Exception):
    pass

  def hooked(pos):
    if steps[0] >= 30:
      raise _Kill()
    steps[0] += 1
    return inner(pos)

  canvas.update_at = hooked
  with pytest.raises(_Kill):
    canvas.segment_all(seed_policy=runner.get_seed_policy(
        (0, 0, 0), tuple(g['volume'].shape)))
  canvas.close()
  cpoint = storage.checkpoint_path(out_dir, (0, 0, 0))
  assert os.path.exists(cpoint)
  # leg 2: Runner.run picks the file up
  done = runner.run((0, 0, 0), tuple(g['volume'].shape))
  assert done is not None and not os.path.exists(cpoint)
  with np.load(storage.segmentation_path(out_dir, (0, 0, 0)),
               allow_pickle=True) as d:
    want = g['segmentation'].copy()
    want[want < 0] = 0
    assert np.array_equal(d['segmentation'], want)
  runner.stop_executor()
  del seed_lib


# ---------------------------------------------------------------------------
# CLI (a22)
# ---------------------------------------------------------------------------
def _cli_args(g, tmp_path, out_dir):
  vol_path = str(tmp_path / 'vol.npy')
  np.save(vol_path, g['volume'])
  weights = os.path.join(GOLDEN, 'fib25_weights.npz')
  seeds = json.dumps({'coords': g['seeds'].tolist()}).replace('"', '\\"')
  request = '''
    image { npy: "%s" }
    image_mean: 128
    image_stddev: 33
    checkpoint_interval: 1800
    seed_policy: "PolicyFixed"
    seed_policy_args: "%s"
    model_checkpoint_path: "%s"
    model_name: "convstack_3d.ConvStack3DFFNModel"
    model_args: "{\\"depth\\": 12, \\"fov_size\\": [33, 33, 33], \\"deltas\\": [8, 8, 8]}"
    segmentation_output_dir: "%s"
    inference_options {
      init_activation: 0.95
      pad_value: 0.05
      move_threshold: 0.9
      min_boundary_dist { x: 1 y: 1 z: 1}
      segment_threshold: 0.6
      min_segment_size: 1000
    }''' % (vol_path, seeds, weights, out_dir)
  z, y, x = g['volume'].shape
  bbox = 'start { x:0 y:0 z:0 } size { x:%d y:%d z:%d }' % (x, y, z)
  return request, bbox


def test_run_inference_main_end_to_end(tmp_path):
  """run_inference.main([...]) -- the reference's CLI flow (run_inference.py:
  38-56): flags -> request -> Runner -> seg-*.npz + counters.txt."""
  import run_inference
  from ffn_amd.inference import storage
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  out_dir = str(tmp_path / 'out')
  request, bbox = _cli_args(g, tmp_path, out_dir)
  run_inference.main(['--inference_request', request, '--bounding_box', bbox])
  path = storage.segmentation_path(out_dir, (0, 0, 0))
  with np.load(path, allow_pickle=True) as d:
    want = g['segmentation'].copy()
    want[want < 0] = 0
    assert np.array_equal(d['segmentation'], want)
    counters = json.loads(str(d['counters']))
    assert counters['update_at-calls'] == len(g['steps'])
  ctr = os.path.join(out_dir, 'counters.txt')
  assert os.path.exists(ctr)
  text = open(ctr).read()
  assert 'update_at-calls' in text


def test_run_inference_main_sharded_assemble(tmp_path):
  """--subvolume_size ... --assemble: sub-boxes advance concurrently on the
  GPU, one global label volume is assembled and reconciled."""
  import run_inference
  from ffn_amd import synthetic
  vol = synthetic.cells_volume((80, 96, 112), seed=21, membrane_dilate=2)
  g = {'volume': vol,
       'seeds': np.array([[z, y, x] for z in (20, 40, 60)
                          for y in (24, 48, 72) for x in (24, 56, 88)])}
  out_dir = str(tmp_path / 'out')
  request, bbox = _cli_args(g, tmp_path, out_dir)
  request = request.replace('seed_policy: "PolicyFixed"',
                            'seed_policy: "PolicyPeaks"')
  request = '\n'.join(l for l in request.split('\n')
                      if 'seed_policy_args' not in l)
  merged_path = str(tmp_path / 'merged.npy')
  run_inference.main(['--inference_request', request, '--bounding_box', bbox,
                      '--subvolume_size', '72,64,56', '--batch_size', '4',
                      '--assemble', merged_path])
  merged = np.load(merged_path)
  assert merged.shape == vol.shape
  ids = np.unique(merged)
  assert len(ids) > 3 and ids[0] == 0
  assert np.mean(merged > 0) > 0.2
  assert os.path.exists(os.path.join(out_dir, 'counters.txt'))


@pytest.mark.gpu
def test_segment_many_in_the_library(fib25_model):
  """ffn_canvas_segment_many (reference executor.py:266-340):
  five device canvases of one engine under MultiCanvasDriver(native=True) --
  whole segment loops in C++, one batched ffn_canvas_step per round, Python
  only between segments -- against the per-step Python driver and the
  reference-minted runs: same steps, same segmentation, same counters."""
  import functools
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.inference import seed as seed_lib
  import bench
  names = ['cells72', 'cells56', 'cells72', 'cells56', 'cells56']
  gold = {n: np.load(os.path.join(GOLDEN, 'ref_canvas_%s.npz' % n))
          for n in set(names)}
  request = bench.make_request()
  runs = {}
  # 'carry' / True: the library's loops with / without the running canvases' next
  # step left in flight when a loop ends (ffn_canvas_segment_many_carry)
  for native in ('carry', True, False):
    counters = inference_utils.Counters()
    exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                    fib25_model.info, None, counters, 4)
    assert exe.engine.get_option('conv_variant') == 8  # batched: pinned
    canvases = []
    for n in names:
      sub = counters.get_sub_counters()
      canvases.append(inference.DeviceCanvas(
          fib25_model.info, exe.get_client(sub, direct=True),
          synthetic.normalize(gold[n]['volume']), request.inference_options,
          counters=sub, keep_history=True,
          movement_policy_fn=movement.get_policy_fn(request, fib25_model.info)))
    drv = inference.MultiCanvasDriver(exe.engine, batch_size=4, native=bool(native),
                                      carry=native == 'carry')
    assert drv.native == bool(native)
    drv.run((c, functools.partial(seed_lib.PolicyFixed, coords=gold[n]['seeds']))
            for c, n in zip(canvases, names))
    assert (exe.engine.get_option('stat_many_carried') > 0) == (native == 'carry')
    out = []
    for c, n in zip(canvases, names):
      out.append(dict(
          seg=np.array(np.asarray(c.segmentation)),
          seed=np.array(c._handle.read_seed()),
          counters={k: c.counters[k].value for k in (
              'update_at-calls', 'skip_threshold', 'skip_invalid_pos',
              'seed_got_too_weak', 'segment_at-loop-calls', 'voxels-segmented')},
          rejects=c.gate_rejects))
      assert np.array_equal(out[-1]['seg'], gold[n]['segmentation']), (native, n)
      assert out[-1]['counters']['update_at-calls'] == len(gold[n]['steps'])
      c.close()
    runs[native] = (out, drv.calls, drv.steps)
  total = sum(len(gold[n]['steps']) for n in names)
  for mode in (True, 'carry'):
    for a, b in zip(runs[mode][0], runs[False][0]):
      assert a['counters'] == b['counters'] and a['rejects'] == b['rejects']
      assert np.array_equal(a['seg'], b['seg'])
      assert np.array_equal(a['seed'], b['seed'], equal_nan=True)
  assert runs[True][2] == runs['carry'][2] == runs[False][2] == total
  # Python entered per segment, not per batched step
  print('engine calls: native %d, per-step %d, for %d FoV steps' % (
      runs[True][1], runs[False][1], total))
  assert runs[True][1] < runs[False][1] / 3


@pytest.mark.gpu
def test_two_canvas_groups_in_two_threads(fib25_model):
  """BASELINE configs[2] shape: more canvases open than FoVs per engine call --
  MultiCanvasDriver(groups=2): two host threads, each advancing its own group of
  canvases through its own ffn_canvas_segment_many calls on ONE engine (the
  library interleaves their steps: one of each in flight).  Every canvas equals
  its standalone, reference-minted run -- whatever it shared its calls and the
  GPU with -- and every job is done exactly once."""
  import functools
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.inference import seed as seed_lib
  import bench
  names = ['cells72', 'cells56', 'cells56', 'cells72', 'cells56', 'cells56',
           'cells72', 'cells56', 'cells72']
  gold = {n: np.load(os.path.join(GOLDEN, 'ref_canvas_%s.npz' % n))
          for n in set(names)}
  request = bench.make_request()
  counters = inference_utils.Counters()
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None, counters, 3)
  canvases = []

  def jobs():
    for n in names:  # created lazily, by whichever thread has a free slot
      sub = counters.get_sub_counters()
      c = inference.DeviceCanvas(
          fib25_model.info, exe.get_client(sub, direct=True),
          synthetic.normalize(gold[n]['volume']), request.inference_options,
          counters=sub,
          movement_policy_fn=movement.get_policy_fn(request, fib25_model.info))
      canvases.append((c, n))
      yield c, functools.partial(seed_lib.PolicyFixed, coords=gold[n]['seeds'])

  results = {}

  def on_done(c):
    results[id(c)] = (np.array(np.asarray(c.segmentation)),
                      c.counters['update_at-calls'].value)
    c.close()

  drv = inference.MultiCanvasDriver(exe.engine, batch_size=3, native=True,
                                    groups=2)
  drv.run(jobs(), on_done=on_done)
  assert len(canvases) == len(names) == len(results)
  total = 0
  for c, n in canvases:
    seg, calls = results[id(c)]
    assert np.array_equal(seg, gold[n]['segmentation']), n
    assert calls == len(gold[n]['steps']), n
    total += calls
  assert drv.steps == total
  exe.engine.close()


@pytest.mark.gpu
def test_cells250_whole_volume_against_reference_minted_run(hip_exe, fib25_model):
  """The WHOLE 250^3 bench volume -- every seed of the grid, 24,131 FoV steps,
  175 objects -- through the reference's own Canvas behind the torch-CPU /
  oneDNN f32 forward (tests/golden/ref_canvas_cells250_onednn_full.npz, 66
  minutes of CPU) against the same run on the GPU with the default kernels.
  A run is a feedback loop that amplifies float noise at threshold decisions
  (DESIGN.md 5.1), so this is MEASURED (profiles/r03_full250_parity.txt) and
  held to what north_star asks of a run: label IoU >= 0.999 -- plus a long
  bit-identical prefix: the first decision that differs is an argmax tie
  between two face voxels 14,069 steps in."""
  path = os.path.join(GOLDEN, 'ref_canvas_cells250_onednn_full.npz')
  if not os.path.exists(path):
    pytest.skip('fixture not minted')
  from ffn_amd import synthetic
  g = np.load(path)
  vol = synthetic.cells_volume((250, 250, 250), seed=1234)
  eng = hip_exe.engine
  _assert_shipped_default(eng)  # nothing chosen: what a user gets
  try:
    canvas = _device_canvas(hip_exe, fib25_model, synthetic.normalize(vol))
    got_steps, _ = _run_recorded(canvas, g['seeds'])
    want_steps = [tuple(int(v) for v in p) for p in g['steps']]
    n = min(len(got_steps), len(want_steps))
    first_bad = next((k for k in range(n) if got_steps[k] != want_steps[k]), n)
    seg = np.asarray(canvas.segmentation)
    want = g['segmentation'].astype(np.int32)
    inter = np.sum((seg > 0) & (want > 0) & (seg == want))
    union = np.sum((seg > 0) | (want > 0))
    iou = inter / max(union, 1)
    print('whole volume: %d steps (reference %d), positions identical for the '
          'first %d, labelled IoU %.6f, objects %d (reference %d)' % (
              len(got_steps), len(want_steps), first_bad, iou,
              len(canvas.origins), len(json.loads(str(g['origins'])))))
    assert first_bad >= 10000, first_bad
    assert iou >= 0.999, iou
    assert abs(len(got_steps) - len(want_steps)) <= 50
    canvas.close()
  finally:
    eng.restore_default_variant()
    eng.set_option('flow', 2)


# ---------------------------------------------------------------------------
# round 3: the next step's conv0_a queued behind the paste (engine option
# `speculate`, SpecArgs in ffn_conv0a.h)
# ---------------------------------------------------------------------------
def test_speculative_conv0a_leaves_the_run_unchanged(hip_exe, fib25_model):
  """ffn_canvas_segment_at with and without the speculative conv0_a launch: the
  same reference-minted run (segmentation, counters, every FoV position), and
  most steps do run on a launch made ahead of the host's turn-around.  A step
  whose launch chose another position than the loop pastes nothing and is made
  again (ffn_step_result.range_error 2): none does unless provoked."""
  from ffn_amd import synthetic
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  eng = hip_exe.engine
  _assert_shipped_default(eng)
  steps = len(g['steps'])
  stats = {}
  stack_ahead_default = eng.get_option('stack_ahead')
  try:
    # (speculate, fuse_paste: faces + paste of a step as ONE launch, fuse_conv0a:
    # the next step's conv0_a in that launch too -- it then gathers the canvas as
    # the paste next to it is leaving it)
    # fuse 2 / 3: five steps whose launch is declared a mismatch (test hook) --
    # they paste nothing and are made again
    # ahead (round 6, engine option stack_ahead): the next step's resident stack queued
    # behind that launch too, before the host has seen this step's record
    for spec, fuse, f0a, ahead in ((1, 0, 0, 0), (0, 0, 0, 0), (1, 1, 0, 0), (0, 1, 0, 0),
                                   (1, 2, 0, 0), (1, 1, 1, 0), (0, 1, 1, 0), (1, 3, 1, 0),
                                   (1, 1, 1, 1), (1, 3, 1, 1), (0, 1, 1, 1)):
      eng.set_option('speculate', spec)
      eng.set_option('stack_ahead', ahead)
      eng.set_option('fuse_paste', fuse & 1)
      eng.set_option('fuse_conv0a', f0a)
      eng.set_option('stat_reset', 0)
      eng.set_option('spec_force_mismatch', 5 if fuse >= 2 else 0)
      canvas = _device_canvas(hip_exe, fib25_model,
                              synthetic.normalize(g['volume']), keep_history=True)
      assert canvas._native_loop_ok()
      seen = []
      inner = canvas._segment_at_native

      def recording(start_pos, *a, _inner=inner, _c=canvas, **kw):
        n = _inner(start_pos, *a, **kw)
        seen.extend(tuple(int(v) for v in p) for p in _c.history[-n:] if n)
        return n

      canvas._segment_at_native = recording
      canvas.segment_all(seed_policy=functools.partial(seed_lib_fixed(),
                                                       coords=g['seeds']))
      assert np.array_equal(np.asarray(canvas.segmentation), g['segmentation'])
      assert canvas.counters['update_at-calls'].value == steps
      if seen:
        assert np.array_equal(np.array(seen), g['steps'])
      if ahead:
        stats['ahead', spec, fuse] = (eng.get_option('stat_ahead_used'),
                                      eng.get_option('stat_ahead_wasted'))
        spec_stats = (eng.get_option('stat_spec_launched'), eng.get_option('stat_spec_hits'))
        canvas.close()
        assert eng.get_option('stat_spec_mismatch') == (5 if fuse >= 2 else 0)
        stats['ahead_spec', spec, fuse] = spec_stats
        continue
      stats[spec, fuse, f0a] = (eng.get_option('stat_spec_launched'),
                                eng.get_option('stat_spec_hits'))
      assert eng.get_option('stat_spec_mismatch') == (5 if fuse >= 2 else 0)
      canvas.close()
  finally:
    eng.set_option('speculate', 1)
    eng.set_option('fuse_paste', 1)
    eng.set_option('fuse_conv0a', 1)
    eng.set_option('spec_force_mismatch', 0)
    eng.set_option('stack_ahead', stack_ahead_default)
  print('cells72, %d steps: conv0_a launched ahead %d times, used by %d steps'
        % ((steps,) + stats[1, 0, 0]))
  print('  stack_ahead: %d stacks queued ahead were used, %d were not (with 5 forced '
        'mismatches: %d / %d)' % (stats['ahead', 1, 1] + stats['ahead', 1, 3]))
  # every step that ran on a conv0_a made ahead also found its stack queued
  assert stats['ahead_spec', 1, 1] == stats[1, 1, 1]
  assert stats['ahead', 1, 1][0] == stats[1, 1, 1][1] > 0
  assert stats['ahead', 0, 1] == (0, 0)
  assert stats[0, 0, 0] == stats[0, 1, 0] == stats[0, 1, 1] == (0, 0)
  assert stats[1, 0, 0] == stats[1, 1, 0] == stats[1, 1, 1]
  # (a repeated step carries no hint: the step after it runs without a launch)
  for k in ((1, 2, 0), (1, 3, 1)):
    assert stats[k][0] == stats[1, 0, 0][0]
    assert stats[1, 0, 0][1] - 5 <= stats[k][1] <= stats[1, 0, 0][1]
  assert (stats[1, 0, 0][0] > steps // 2 and
          stats[1, 0, 0][1] > 0.6 * stats[1, 0, 0][0])


def test_speculative_conv0a_permuted_layout():
  """The same on BASELINE configs[4]'s FoV (zyx 21 x 41 x 41: the split-product
  kernels lay it out with permuted axes): a flood through a
  40 x 90 x 96 canvas (random weights, a move threshold below the pad value, so
  every face queues a move), speculation on and off."""
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.training.models import convstack_3d
  from oracle import ffn_oracle
  fov, deltas, depth = (21, 41, 41), (5, 10, 10), 3
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(fov[::-1]),
                                       deltas=list(deltas[::-1]), depth=depth)
  m.set_variables(ffn_oracle.random_weights(depth, seed=8, stddev=0.06))
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), m, m.info, None,
                                  inference_utils.Counters(), 1, device_id=0)
  eng = exe.engine
  r = _request()
  r.inference_options.move_threshold = 0.01
  vol = synthetic.normalize(synthetic.cells_volume((40, 90, 96), seed=3))
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
    n = canvas.segment_at((20, 45, 48))
    out[spec] = (n, [tuple(int(v) for v in p) for p in canvas.history],
                 np.array(np.asarray(canvas.seed)),
                 eng.get_option('stat_spec_launched'),
                 eng.get_option('stat_spec_hits'))
    canvas.close()
  eng.close()
  print('c5 FoV flood: %d steps, %d launched ahead, %d used' % (
      out[1][0], out[1][3], out[1][4]))
  assert out[1][0] == out[0][0] > 40
  assert out[1][1] == out[0][1]
  assert np.array_equal(out[1][2], out[0][2], equal_nan=True)
  assert out[0][3:] == (0, 0)
  assert out[1][4] > 0.5 * out[1][0]


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['cells56_pred25', 'cells72_pred27'])
def test_pred_smaller_than_seed_on_device(fib25_model, name):
  """A model that predicts a smaller mask than the seed it reads (ModelInfo
  pred_mask_size < input_seed_size; reference model.py:168-183, inference.py:
  218,410-411) on the GPU: `ffn_engine_set_pred_size` makes the canvas step score
  the faces around the centre of the pred box, count and disco-bias inside it and
  paste only it.  Against the run the reference's own Canvas made
  (tools/make_golden.py --only predcrop): every FoV position, the queued moves,
  the final labels -- through the Python loop and through the in-library one."""
  import copy
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference_utils
  path = os.path.join(GOLDEN, 'ref_canvas_%s.npz' % name)
  if not os.path.exists(path):
    pytest.skip('fixture not minted')
  g = np.load(path)
  pred = tuple(int(v) for v in g['pred_zyx'])
  model = copy.copy(fib25_model)
  model.info = copy.copy(fib25_model.info)
  model.info.pred_mask_size = np.array(pred[::-1])
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), model, model.info,
                                  None, inference_utils.Counters(), 1, device_id=0)
  try:
    assert exe.engine.pred_zyx == pred
    image = synthetic.normalize(g['volume'])
    # the stateless contract returns the pred box
    seed = np.full((1, 33, 33, 33), -2.0, np.float32)
    out = exe.engine.predict(seed, image[None, 4:37, 5:38, 6:39])
    assert out.shape[1:] == pred
    # (a) the Python loop, step by step
    canvas = _device_canvas(exe, model, image)
    got_steps, got_moves = _run_recorded(canvas, g['seeds'])
    assert got_steps == [tuple(int(v) for v in p) for p in g['steps']]
    off = 0
    for k, moves in enumerate(got_moves):
      nm = int(g['n_moves'][k])
      assert len(moves) == nm, k
      for j, (s, c) in enumerate(moves):
        assert c == tuple(int(v) for v in g['move_coords'][off + j]), (k, j)
        assert abs(s - float(g['move_scores'][off + j])) <= RUN_TOL
      off += nm
    assert np.array_equal(np.asarray(canvas.segmentation), g['segmentation'])
    seed_got = np.asarray(canvas.seed)
    assert np.array_equal(np.isnan(seed_got), np.isnan(g['seed_logits']))
    print('pred %r: final seed difference %.3g' % (
        pred, float(np.nanmax(np.abs(seed_got - g['seed_logits'])))))
    assert np.nanmax(np.abs(seed_got - g['seed_logits'])) <= RUN_TOL
    canvas.close()
    # (b) the in-library segment loop (speculative conv0_a, fused faces + paste)
    canvas = _device_canvas(exe, model, image)
    assert canvas._native_loop_ok()
    canvas.segment_all(seed_policy=functools.partial(seed_lib_fixed(),
                                                     coords=g['seeds']))
    assert np.array_equal(np.asarray(canvas.segmentation), g['segmentation'])
    ref_c = json.loads(str(g['counters']))
    for key in ('update_at-calls', 'voxels-segmented', 'skip_invalid_pos'):
      assert canvas.counters[key].value == ref_c[key], key
    canvas.close()
  finally:
    exe.engine.close()
