"""The library's seed loop (ffn_amd/csrc/ffn_host_loop.h SeedLoop ->
ffn_canvas_segment_all) on the CPU: tests/seed_loop_shim.cpp instantiates the
template over callbacks into the emulated device, whose numpy turn is the
specification tests/test_gpu_turn.py uses.  Against the reference-minted runs and
against the Python seed loop (`DeviceCanvas._segment_all_gen`) on the same
device, call budgets, checkpoints, a voided step, odd seed lists, a restrictor,
and the cases that must stay on the Python loop."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from ffn_amd import _lib
from ffn_amd import engine as hip_engine
from ffn_amd import synthetic
from ffn_amd.inference import inference
from ffn_amd.inference import inference_utils
from ffn_amd.inference import movement
from ffn_amd.inference import request as req_lib
from ffn_amd.inference import seed as seed_lib
from ffn_amd.training import model as ffn_model
from oracle import ffn_oracle
from tests import native_shim
from tests import restriction_ref
from tests.native_shim import ShimHandle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')

_TURN_CB = ctypes.CFUNCTYPE(
    ctypes.c_int, ctypes.POINTER(_lib.TurnRequest), ctypes.POINTER(ctypes.c_int32),
    ctypes.POINTER(_lib.TurnResult), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32),
    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32),
    ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32))
_BASE_FUNCS = ('shim_state_create', 'shim_state_destroy', 'shim_segment_at',
               'shim_segment_many', 'shim_segment_many_carry', 'shim_carry_active',
               'shim_history', 'shim_sizeof_params', 'shim_sizeof_result',
               'shim_set_hint_cb')
_SIZES = ('seed_record', 'seed_args', 'seed_result', 'turn_request')
_OFFSETS = ('seed_record_segment', 'seed_args_overlap_counts',
            'seed_args_min_segment_size', 'seed_result_in_segment')


@pytest.fixture(scope='module')
def lib(tmp_path_factory):
  out_dir = tmp_path_factory.mktemp('seed_loop_shim')
  base = native_shim.build_shim(out_dir)
  out = os.path.join(str(out_dir), 'seed_loop_shim.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', out,
                         os.path.join(HERE, 'seed_loop_shim.cpp')])
  so = ctypes.CDLL(out)
  for name in _BASE_FUNCS:
    getattr(so, name).restype = getattr(base, name).restype
    getattr(so, name).argtypes = getattr(base, name).argtypes
  so.shim_state_set_restriction.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int64]
  so.shim_take_restricted_skips.restype = ctypes.c_int64
  so.shim_take_restricted_skips.argtypes = [ctypes.c_void_p]
  so.shim_seed_state_create.restype = ctypes.c_void_p
  so.shim_seed_state_destroy.argtypes = [ctypes.c_void_p]
  so.shim_segment_all.restype = ctypes.c_int
  so.shim_segment_all.argtypes = [
      ctypes.c_void_p, ctypes.c_void_p, native_shim._STEP_CB, native_shim._READ_CB,
      _TURN_CB, ctypes.POINTER(_lib.SeedLoopArgs), ctypes.POINTER(_lib.SeedLoopResult)]
  for name in _SIZES:
    getattr(so, 'shim_sizeof_' + name).restype = ctypes.c_size_t
  for name in _OFFSETS:
    getattr(so, 'shim_offsetof_' + name).restype = ctypes.c_size_t
  return so


@pytest.fixture(scope='module', autouse=True)
def forward_memo():
  """The emulated device's forward pass, remembered by its inputs: every run of
  this module makes the same FoV steps, and only the first one computes them."""
  real = ffn_oracle.forward
  memo = {}

  def forward(image, seed, blob, depth):
    key = hashlib.sha1(np.ascontiguousarray(image).tobytes() +
                       np.ascontiguousarray(seed).tobytes()).digest()
    if key not in memo:
      memo[key] = real(image, seed, blob, depth)
    return memo[key].copy()

  ffn_oracle.forward = forward
  yield
  ffn_oracle.forward = real


class _Stop(Exception):
  """Raised in place of a library call: the interpreter taking over at a return."""


class SeedLoopHandle(restriction_ref.RestrictShimHandle):
  """Emulated canvas + `segment_at` and `segment_all` through the C++ loops
  (what DeviceCanvasHandle is on the GPU)."""

  def __init__(self, image):
    super().__init__(image)
    self._seed_state = self.shim.shim_seed_state_create()
    self.raw_rcs = []     # return code of every library call, legs of a retry included
    self.per_call = []    # (records, turns) of every `segment_all`
    self.stop_before = None  # raise _Stop instead of making call number ...
    self.fallbacks = []

  def segment_all(self, args):
    if self.stop_before is not None and len(self.per_call) == self.stop_before:
      raise _Stop()
    error = []

    def guarded(fn):
      def call(*a):
        try:
          return fn(*a)
        except BaseException as e:  # pylint:disable=broad-except
          error.append(e)
          return -1
      return call

    def step_cb(req, par, res):
      if self.fail_step is not None and len(self.steps_seen) == self.fail_step:
        self.fail_step = None
        return self.fail_code
      self.steps_seen.append(tuple(req.contents.pos))
      out = self.client.step(self, req.contents, par.contents)
      ctypes.memmove(res, ctypes.addressof(out), ctypes.sizeof(out))
      return 0

    def read_cb(pos, seed, seg):
      seed[0], seg[0] = self.read_point((pos[0], pos[1], pos[2]))
      return 0

    def turn_cb(rq, cand, out, max_overlaps, ids, counts, flags, cseed, cseg):
      r = rq.contents
      commit = ((list(r.lo), list(r.hi), r.segment_threshold, r.min_segment_size,
                 r.segment_id, r.max_existing_id) if r.do_commit else None)
      mark = (tuple(r.mark_pos), r.mark_mode) if r.mark_mode else None
      n = r.num_candidates
      cands = [(cand[3 * k], cand[3 * k + 1], cand[3 * k + 2]) for k in range(n)]
      got = self.segment_turn(commit, mark, cands, tuple(r.min_boundary_dist),
                              r.init_value if r.do_init else None)
      raw, actual, oids, ocnt, committed, chosen, fl, cs, cg = got
      assert len(oids) <= max_overlaps
      o = out.contents
      o.counts.raw_segmented_voxels, o.counts.actual_segmented_voxels = raw, actual
      o.counts.num_overlapped_ids = len(oids)
      o.committed, o.chosen = int(committed), int(chosen)
      for k in range(len(oids)):
        ids[k], counts[k] = int(oids[k]), int(ocnt[k])
      for k in range(n):
        flags[k], cseed[k], cseg[k] = int(fl[k]), float(cs[k]), int(cg[k])
      return 0

    cbs = (native_shim._STEP_CB(guarded(step_cb)),
           native_shim._READ_CB(guarded(read_cb)), _TURN_CB(guarded(turn_cb)))

    def once(a, r):
      rc = self.shim.shim_segment_all(self._state, self._seed_state, cbs[0], cbs[1],
                                      cbs[2], ctypes.byref(a), ctypes.byref(r))
      self.raw_rcs.append(rc)
      return rc

    rc, res = hip_engine.seed_loop_with_retry(once, args, self.fallbacks.append)
    if error:
      raise error[0]
    assert rc == 0, rc
    self.per_call.append((res.num_records, res.turns))
    return res


class SeedLoopClient(native_shim.ShimClient):

  def create_canvas(self, image):
    ShimHandle.client = self
    return SeedLoopHandle(image)


def _options():
  r = req_lib.InferenceRequest()
  o = r.inference_options
  o.init_activation, o.pad_value, o.move_threshold = 0.95, 0.05, 0.9
  o.segment_threshold, o.min_segment_size = 0.6, 1000
  o.min_boundary_dist.x = o.min_boundary_dist.y = o.min_boundary_dist.z = 1
  return r


def _canvas(lib, blob, volume, native=True, cls=None, normalize=True, **kwargs):
  """A DeviceCanvas over the shim; native=False: the same device, the seed loop
  in Python (what every canvas ran before ffn_canvas_segment_all)."""
  ShimHandle.shim = lib
  r = _options()
  info = ffn_model.ModelInfo(np.array([8, 8, 8]), np.array([33, 33, 33]),
                             np.array([33, 33, 33]), np.array([33, 33, 33]))
  client = SeedLoopClient(inference_utils.Counters(), blob, 12, (33, 33, 33),
                          (8, 8, 8))
  image = synthetic.normalize(volume) if normalize else volume
  c = (cls or inference.DeviceCanvas)(
      info, client, image, r.inference_options,
      counters=inference_utils.Counters(),
      movement_policy_fn=movement.get_policy_fn(r, info), **kwargs)
  if not native:
    c.NATIVE_SEED_LOOP = False
  return c


def _fixed(coords):
  return functools.partial(seed_lib.PolicyFixed, coords=np.asarray(coords))


def _work_counters(c, drop=()):
  return {k: t.value for k, t in c.counters
          if not k.endswith('-time-ms') and k not in drop}


def _state(c, drop=()):
  return {
      'segmentation': np.array(np.asarray(c.segmentation)),
      'seed': np.array(np.asarray(c.seed)).view(np.uint32),
      'origins': {k: (tuple(int(x) for x in v.start_zyx), int(v.iters))
                  for k, v in c.origins.items()},
      'overlaps': {k: np.asarray(v).tolist() for k, v in c.overlaps.items()},
      'max_id': c._max_id,
      'idx': c.seed_policy.idx,
      'gate_rejects': c.gate_rejects,
      'steps': list(c._handle.steps_seen),
      'counters': _work_counters(c, drop),
  }


def _assert_same(a, b):
  assert a.keys() == b.keys()
  for key in a:
    if isinstance(a[key], np.ndarray):
      assert np.array_equal(a[key], b[key]), key
    else:
      assert a[key] == b[key], key


_RUNS = {}


def _run(lib, blob, name, native, segments=None, ms=None):
  """One complete pass over a fixture, made once per module."""
  key = (name, native, segments, ms)
  if key not in _RUNS:
    g = np.load(os.path.join(GOLDEN, 'ref_canvas_%s.npz' % name))
    c = _canvas(lib, blob, g['volume'], native)
    if segments is not None:
      c.SEED_LOOP_SEGMENTS, c.SEED_LOOP_MS = segments, ms
    c.segment_all(seed_policy=_fixed(g['seeds']))
    _RUNS[key] = (c, _state(c))
  return _RUNS[key]


def test_struct_layout_matches_the_header(lib):
  assert ctypes.sizeof(_lib.SeedRecord) == lib.shim_sizeof_seed_record() == 144
  assert ctypes.sizeof(_lib.SeedLoopArgs) == lib.shim_sizeof_seed_args() == 248
  assert ctypes.sizeof(_lib.SeedLoopResult) == lib.shim_sizeof_seed_result() == 80
  assert ctypes.sizeof(_lib.TurnRequest) == lib.shim_sizeof_turn_request()
  assert _lib.SeedRecord.segment.offset == lib.shim_offsetof_seed_record_segment()
  assert (_lib.SeedLoopArgs.overlap_counts.offset ==
          lib.shim_offsetof_seed_args_overlap_counts())
  assert (_lib.SeedLoopArgs.min_segment_size.offset ==
          lib.shim_offsetof_seed_args_min_segment_size())
  assert (_lib.SeedLoopResult.in_segment.offset ==
          lib.shim_offsetof_seed_result_in_segment())


@pytest.mark.parametrize('name', ['cells56', 'cells72'])
def test_native_seed_loop_reproduces_reference_run(lib, fib25_blob, name):
  """segment_all through ffn_canvas_segment_all == the reference's own
  Canvas.segment_all (steps, segmentation, counters)."""
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_%s.npz' % name))
  c, st = _run(lib, fib25_blob, name, True)
  assert c.seed_loop_calls > 0 and c._handle.native_calls == 0
  assert np.array_equal(np.array(st['steps']).reshape(-1, 3), g['steps'])
  assert np.array_equal(st['segmentation'], g['segmentation'])
  ref = json.loads(str(g['counters']))
  for key in ('update_at-calls', 'voxels-segmented', 'skip_invalid_pos',
              'skip_threshold', 'seed_got_too_weak', 'segment_at-loop-calls'):
    if key in ref:
      assert c.counters[key].value == ref[key], key
  for key in ('seed-policy-calls', 'voxels-overlapping', 'segment_all-calls'):
    assert c.counters[key].value == ref[key], key


@pytest.mark.parametrize('name', ['cells56', 'cells72'])
def test_native_seed_loop_equals_python_seed_loop(lib, fib25_blob, name):
  nc, nst = _run(lib, fib25_blob, name, True)
  pc, pst = _run(lib, fib25_blob, name, False)
  assert nc.seed_loop_calls > 0 and 'seed_loop_calls' not in pc.__dict__
  assert pc._handle.native_calls > 0 and pc.turns > 0
  _assert_same(nst, pst)
  assert np.array_equal(nc._min_pos, pc._min_pos)
  assert np.array_equal(nc._max_pos, pc._max_pos)
  assert set(k for k, _ in nc.counters) == set(k for k, _ in pc.counters)


def test_call_budgets_do_not_change_the_result(lib, fib25_blob):
  """max_segments 1, 2 and no budget at all: the same final state; a call never
  attempts more segments than its budget."""
  _, want = _run(lib, fib25_blob, 'cells72', True)
  for segments, most in ((1, 1), (2, 2), (0, 10**9)):
    c, st = _run(lib, fib25_blob, 'cells72', True, segments, 0.0)
    _assert_same(st, want)
    assert all(n <= most for n, _ in c._handle.per_call)
    if segments == 1:
      assert len(c._handle.per_call) >= st['counters']['segment_at-loop-calls']
    if segments == 0:
      assert len(c._handle.per_call) == 1


def test_every_return_is_between_two_seeds(lib, fib25_blob):
  """One segment per call; after each return in turn the interpreter takes over
  and finishes the pass on the Python seed loop: always the all-Python result."""
  _, want = _run(lib, fib25_blob, 'cells72', False)
  full, _ = _run(lib, fib25_blob, 'cells72', True, 1, 0.0)
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  drop = ('segment_all-calls',)  # (two segment_all calls made this pass)
  want = dict(want, counters={k: v for k, v in want['counters'].items()
                              if k not in drop})
  for k in range(1, len(full._handle.per_call)):
    c = _canvas(lib, fib25_blob, g['volume'])
    c.SEED_LOOP_SEGMENTS, c.SEED_LOOP_MS = 1, 0.0
    c._handle.stop_before = k
    with pytest.raises(_Stop):
      c.segment_all(seed_policy=_fixed(g['seeds']))
    assert c.seed_loop_calls == k
    # nothing initialised or tested ahead: no turn record, no cached answers
    assert c._turn_rec is None and not c._cache
    policy = c.seed_policy
    c.NATIVE_SEED_LOOP = False
    c.segment_all(seed_policy=lambda canvas: policy)
    assert c.seed_loop_calls == k
    _assert_same(_state(c, drop), want)


def test_due_checkpoint_ends_the_call_after_one_segment(lib, fib25_blob, tmp_path):
  """A deadline that has passed: every call returns after one segment with
  nothing initialised ahead and the checkpoint is written there; restored into
  a new canvas, it finishes to the same segmentation."""
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  _, want = _run(lib, fib25_blob, 'cells72', True)
  path = str(tmp_path / 'ckpt.npz')
  c = _canvas(lib, fib25_blob, g['volume'], checkpoint_path=path,
              checkpoint_interval_sec=1e-9)
  c._handle.stop_before = 2
  with pytest.raises(_Stop):
    c.segment_all(seed_policy=_fixed(g['seeds']))
  assert [n for n, _ in c._handle.per_call] == [1, 1]
  assert c._turn_rec is None and os.path.exists(path)
  saved = np.load(path, allow_pickle=True)
  assert np.array_equal(saved['segmentation'], np.asarray(c.segmentation))
  assert int(saved['seed_policy_state'][1]) == c.seed_policy.idx
  r = _canvas(lib, fib25_blob, g['volume'])
  assert r.restore_checkpoint(path) == 0
  r.segment_all(seed_policy=_fixed(g['seeds']))
  assert r.seed_loop_calls > 0
  assert np.array_equal(np.asarray(r.segmentation), want['segmentation'])
  assert r._max_id == want['max_id'] and r.seed_policy.idx == want['idx']
  assert r.origins.keys() == want['origins'].keys()


@pytest.mark.parametrize('code', [_lib.ERR_RANGE, _lib.ERR_FLOW])
def test_voided_step_is_resumed_without_losing_or_repeating_a_step(lib, fib25_blob,
                                                                   code):
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  _, want = _run(lib, fib25_blob, 'cells72', True)
  c = _canvas(lib, fib25_blob, g['volume'])
  c._handle.fail_step, c._handle.fail_code = 40, code  # mid-segment
  c.segment_all(seed_policy=_fixed(g['seeds']))
  h = c._handle
  assert h.raw_rcs.count(code) == 1 and h.fallbacks == [code]
  assert h.raw_rcs[h.raw_rcs.index(code) + 1] == 0  # the resumed leg
  assert np.array_equal(np.array(h.steps_seen).reshape(-1, 3), g['steps'])
  _assert_same(_state(c), want)


def _both(lib, blob, volume, lists, **kwargs):
  """The passes `lists` on one canvas per path -> their states after each pass."""
  out = []
  for native in (True, False):
    c = _canvas(lib, blob, volume, native, **kwargs)
    states = []
    for coords in lists:
      c.segment_all(seed_policy=_fixed(coords))
      states.append(_state(c))
    out.append((c, states))
  (nc, ns), (pc, ps) = out
  assert nc.seed_loop_calls == len(lists) and 'seed_loop_calls' not in pc.__dict__
  for a, b in zip(ns, ps):
    _assert_same(a, b)
  return nc, ns


def test_odd_seed_lists(lib, fib25_blob):
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  seeds = g['seeds']
  done = np.argwhere(g['segmentation'][16:40, 16:40, 16:40] > 0) + 16
  assert len(done) > 300
  taken = done[::len(done) // 300][:300]
  # a seed listed twice: next to each other, and again after other seeds
  twice = np.concatenate([seeds[:1], seeds[:1], seeds, seeds[:2]])
  nc, ns = _both(lib, fib25_blob, g['volume'], [twice])
  assert np.array_equal(ns[0]['segmentation'], g['segmentation'])
  assert ns[0]['idx'] == len(twice)
  # the fixture's pass, then a list longer than one turn's 128 candidates with every
  # seed refused, then an empty one
  nc, ns = _both(lib, fib25_blob, g['volume'],
                 [seeds, taken, np.zeros((0, 3), np.int64)])
  assert ns[1]['idx'] == 300 and ns[1]['steps'] == ns[0]['steps']
  assert [n for n, _ in nc._handle.per_call][1:] == [0, 0]
  assert nc._handle.per_call[1][1] == 3  # 300 seeds: windows of 128, 128 and 44
  assert np.array_equal(ns[2]['segmentation'], g['segmentation'])
  # a first window without a valid seed, the seeds that start segments behind it
  g72 = np.load(os.path.join(GOLDEN, 'ref_canvas_cells72.npz'))
  first = g72['seeds'][:6]
  d72 = np.argwhere(_run(lib, fib25_blob, 'cells72', True)[1]['segmentation']
                    [16:56, 16:48, 16:64] > 0) + 16
  nc, ns = _both(lib, fib25_blob, g72['volume'], [first])
  refused = np.argwhere(ns[0]['segmentation'][16:56, 16:48, 16:64] > 0) + 16
  del d72
  late = np.concatenate([refused[::len(refused) // 140][:140], g72['seeds'][6:]])
  nc, ns = _both(lib, fib25_blob, g72['volume'], [first, late])
  assert ns[1]['idx'] == len(late) and len(ns[1]['steps']) > len(ns[0]['steps'])


class _Box:

  def __init__(self, start, size):
    self.start = np.array(start)
    self.end = self.start + np.array(size)


def test_restricted_pass_equals_python_seed_loop(lib, fib25_blob):
  """The canvas of tests/test_restrict_host_loop.py (mask, seed mask and shift
  mask on the device): the same result, skip_restriced_pos included."""
  g = np.load(os.path.join(GOLDEN, 'ref_masks.npz'))

  def restrictor():
    return movement.MovementRestrictor(
        mask=g['run_mask'], seed_mask=g['run_seed_mask'], shift_mask=g['run_shift'],
        shift_mask_fov=_Box((-6, -6, -4), (13, 13, 9)), shift_mask_threshold=4,
        shift_mask_scale=2)

  out = []
  for native in (True, False):
    c = _canvas(lib, fib25_blob, g['run_volume'], native, restrictor=restrictor())
    assert c._restrict_on
    c.segment_all(seed_policy=_fixed(g['run_seeds']))
    out.append((c, _state(c)))
  (nc, ns), (pc, ps) = out
  assert nc.seed_loop_calls > 0 and 'seed_loop_calls' not in pc.__dict__
  _assert_same(ns, ps)
  assert ns['counters']['skip_restriced_pos'] > 0 and nc._handle.flag4 > 0
  assert np.array_equal(ns['segmentation'], g['run_segmentation'])
  assert ns['steps'] == [tuple(int(v) for v in p) for p in g['run_steps']]


class _Hooked(inference.DeviceCanvas):
  """bench.py's NativeBenchCanvas pattern: the override drives the library's
  segment loop in legs of one step."""
  legs = 0

  def _segment_at_native(self, start_pos, max_steps=0, resume=False):
    n = super()._segment_at_native(start_pos, max_steps=1)
    self.legs += 1
    while self._native_active:
      n += super()._segment_at_native(start_pos, max_steps=1, resume=True)
      self.legs += 1
    return n


class _OwnOrder(seed_lib.PolicyFixed):

  def __next__(self):
    return super().__next__()


def test_what_needs_the_interpreter_keeps_the_python_loop(lib, fib25_blob):
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_cells56.npz'))
  policy = _fixed(g['seeds'])

  def check(c, policy=policy, **kw):
    c.segment_all(seed_policy=policy, **kw)
    assert 'seed_loop_calls' not in c.__dict__ and c._handle.per_call == []
    return c

  # a subclass overriding _segment_at_native: the fixture's steps, as before
  c = check(_canvas(lib, fib25_blob, g['volume'], cls=_Hooked))
  assert c.legs >= c.counters['update_at-calls'].value > 2
  assert np.array_equal(np.array(c._handle.steps_seen).reshape(-1, 3), g['steps'])
  assert np.array_equal(np.asarray(c.segmentation), g['segmentation'])
  # an instance hook on it (bench.py's recorded_pass)
  c = _canvas(lib, fib25_blob, g['volume'])
  inner, seen = c._segment_at_native, []
  c._segment_at_native = lambda pos, *a, **kw: seen.append(pos) or inner(pos, *a, **kw)
  check(c)
  assert len(seen) == c.counters['segment_at-loop-calls'].value > 0
  check(_canvas(lib, fib25_blob, g['volume'], keep_history=True))
  check(_canvas(lib, fib25_blob, g['volume']),
        policy=functools.partial(_OwnOrder, coords=g['seeds']))
  check(_canvas(lib, fib25_blob, g['volume']), partial_segment_iters=1)
  # ... and a plain canvas does take the library's loop
  c = _canvas(lib, fib25_blob, g['volume'])
  c.segment_all(seed_policy=policy)
  assert c.seed_loop_calls == 1


def test_seed_loop_under_sanitizers(tmp_path):
  """The shim and a stand-alone main over a stub device, built with
  -fsanitize=address,undefined and run as a program of its own."""
  exe = str(tmp_path / 'seed_loop_sanitize')
  subprocess.check_call(
      ['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined',
       '-fno-sanitize-recover=undefined', '-static-libasan', '-static-libubsan',
       '-o', exe, os.path.join(HERE, 'seed_loop_sanitize_main.cpp')])
  done = subprocess.run([exe], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stdout + done.stderr
  assert 'committed 3' in done.stdout and 'voided 1' in done.stdout
