"""The library's segment loop and turn with a MovementRestrictor,
on the CPU: ffn_amd/csrc/ffn_host_loop.h (tests/host_loop_restrict_shim.cpp)
over the emulated device, with the pos_blocked bit plane built in numpy
(tests/restriction_ref.py), against the Python loop with the host restrictor
and the reference-minted run of tests/golden/ref_masks.npz."""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from ffn_amd import synthetic
from ffn_amd.inference import inference
from ffn_amd.inference import inference_utils
from ffn_amd.inference import movement
from ffn_amd.inference import request as req_lib
from ffn_amd.inference import seed as seed_lib
from ffn_amd.training import model as ffn_model
from tests import native_shim
from tests import restriction_ref
from tests.conftest import GOLDEN
from tests.emulated_device import EmulatedDeviceClient
from tests.native_shim import ShimHandle

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(GOLDEN, 'ref_masks.npz')
WORK = ('skip_restriced_pos', 'skip_threshold', 'skip_invalid_pos',
        'update_at-calls', 'seed_got_too_weak', 'voxels-segmented')
_SHIM_FUNCS = ('shim_state_create', 'shim_state_destroy', 'shim_segment_at',
               'shim_segment_many', 'shim_segment_many_carry', 'shim_carry_active',
               'shim_history', 'shim_sizeof_params', 'shim_sizeof_result',
               'shim_set_hint_cb')


@pytest.fixture(scope='module')
def rshim(tmp_path_factory):
  out_dir = tmp_path_factory.mktemp('rshim')
  base = native_shim.build_shim(out_dir)
  out = os.path.join(str(out_dir), 'host_loop_restrict_shim.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-o', out,
                         os.path.join(HERE, 'host_loop_restrict_shim.cpp')])
  lib = ctypes.CDLL(out)
  for name in _SHIM_FUNCS:
    getattr(lib, name).restype = getattr(base, name).restype
    getattr(lib, name).argtypes = getattr(base, name).argtypes
  lib.shim_state_set_restriction.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_int64]
  lib.shim_take_restricted_skips.restype = ctypes.c_int64
  lib.shim_take_restricted_skips.argtypes = [ctypes.c_void_p]
  return lib


class _Box:

  def __init__(self, start, size):
    self.start = np.array(start)
    self.end = self.start + np.array(size)


def _restrictor(g):
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


def _canvas(rshim, blob, volume, restrictor, native):
  ShimHandle.shim = rshim
  r = _options()
  info = ffn_model.ModelInfo(np.array([8, 8, 8]), np.array([33, 33, 33]),
                             np.array([33, 33, 33]), np.array([33, 33, 33]))
  cls = restriction_ref.RestrictShimClient if native else EmulatedDeviceClient
  client = cls(inference_utils.Counters(), blob, 12, (33, 33, 33), (8, 8, 8))
  return inference.make_canvas(
      info, client, synthetic.normalize(volume), r.inference_options,
      counters=inference_utils.Counters(), restrictor=restrictor,
      keep_history=True, movement_policy_fn=movement.get_policy_fn(r, info))


def _record_segments(canvas):
  """Per segment: start, FoV positions, steps, the work counters after it."""
  segs = []
  inner = canvas._segment_at_gen

  def gen(start_pos, partial_segment_iters=0):
    n = yield from inner(start_pos, partial_segment_iters)
    c = canvas.counters
    segs.append((tuple(int(v) for v in start_pos),
                 [tuple(int(v) for v in p) for p in canvas.history], n,
                 {k: c[k].value for k in WORK}))
    return n

  canvas._segment_at_gen = gen
  return segs


def test_numpy_restriction_is_the_restrictors_test():
  """tests/restriction_ref.restriction (what the device must build) answers
  MovementRestrictor.is_valid_pos / is_valid_seed at every position of the
  fixture's canvas."""
  g = np.load(FIX)
  r = _restrictor(g)
  shape = g['run_mask'].shape
  bits = restriction_ref.restriction(shape, **restriction_ref.restrictor_args(r))
  for p in np.ndindex(*shape):
    assert bool(bits[p] & 1) == (not r.is_valid_pos(p)), p
    assert bool(bits[p] & 2) == (not r.is_valid_seed(p)), p
  assert 0 < np.count_nonzero(bits & 1) < bits.size


def test_restricted_library_loop_matches_python_loop(rshim, fib25_blob):
  """The fixture's restricted run through the library's loop (bit plane) and
  turn (flag 4) equals the Python loop with the host restrictor segment by
  segment -- positions, skip_restriced_pos, skip_threshold, skip_invalid_pos --
  and the reference's own run."""
  g = np.load(FIX)
  seeds = functools.partial(seed_lib.PolicyFixed, coords=g['run_seeds'])
  runs = []
  for native in (True, False):
    c = _canvas(rshim, fib25_blob, g['run_volume'], _restrictor(g), native)
    assert c._native_loop_ok() == native
    assert c._turn_ok() == native
    segs = _record_segments(c)
    c.segment_all(seed_policy=seeds)
    runs.append((c, segs))
  (nc, nsegs), (pc, psegs) = runs
  assert nc._handle.native_calls == len(nsegs) > 0
  assert nc.turns > 0 and pc.turns == 0
  assert len(nsegs) == len(psegs)
  for k, (a, b) in enumerate(zip(nsegs, psegs)):
    assert a == b, k
  assert np.array_equal(np.asarray(nc.segmentation), np.asarray(pc.segmentation))
  assert np.array_equal(np.asarray(nc.segmentation), g['run_segmentation'])
  steps = [p for s in nsegs for p in s[1]]
  assert steps == [tuple(int(v) for v in p) for p in g['run_steps']]
  ref = json.loads(str(g['run_counters']))
  for key in ('update_at-calls', 'skip_restriced_pos', 'skip_invalid_pos',
              'skip_threshold', 'voxels-segmented'):
    assert nc.counters[key].value == ref[key], key
  assert nc.counters['skip_restriced_pos'].value > 0


def test_restricted_turn_keeps_vetoed_seeds_in_its_record(rshim, fib25_blob):
  """A seed the device turn flags 4 (restrictor) stays in the turn's record
  with its point values: the seed loop's is_valid_pos answers from the cache
  (no device read) and the host restrictor then rejects it, as the reference
  does -- the seed is neither marked -1 nor started."""
  g = np.load(FIX)
  r = _restrictor(g)
  c = _canvas(rshim, fib25_blob, g['run_volume'], r, True)
  shape = g['run_mask'].shape
  vetoed = [p for p in np.ndindex(*shape)
            if c._in_bounds(p) and not r.is_valid_seed(p) and r.is_valid_pos(p)][:3]
  free = [p for p in np.ndindex(*shape)
          if c._in_bounds(p) and r.is_valid_seed(p) and r.is_valid_pos(p)][:1]
  assert len(vetoed) == 3 and free
  coords = np.array(vetoed + free)
  c.seed_policy = seed_lib.PolicyFixed(c, coords=coords)
  pol = c.seed_policy
  c._turn_armed = True
  first = next(pol)
  reads = c._handle.point_reads
  assert c.is_valid_pos(first, ignore_move_threshold=True)  # the turn runs here
  assert c._handle.flag4 == 3
  rec = c._turn_rec
  assert [rec['seen'][v] for v in vetoed] == [4, 4, 4]
  assert rec['seen'][free[0]] == 0 and rec['init'] == free[0]
  for v in vetoed:
    assert v in c._cache
  assert not r.is_valid_seed(first)
  for v in vetoed[1:]:
    assert c.is_valid_pos(v, ignore_move_threshold=True)
  assert c._handle.point_reads == reads  # answered from the record
  seg = c._handle.read_segmentation()
  assert all(seg[v] == 0 for v in vetoed)


def test_restrictor_reassignment_and_subclass(rshim, fib25_blob):
  """Assigning `restrictor` re-uploads it (and drops the cached eligibility); a
  subclass of MovementRestrictor keeps the Python loop."""
  g = np.load(FIX)
  c = _canvas(rshim, fib25_blob, g['run_volume'], None, True)
  assert c._native_loop_ok() and c._handle.bits is None
  c.restrictor = _restrictor(g)
  assert c._native_loop_ok() and c._turn_ok()
  want = restriction_ref.restriction(
      c.shape, **restriction_ref.restrictor_args(c.restrictor))
  assert np.array_equal(c._handle.read_restriction(), want)

  class Hooked(movement.MovementRestrictor):
    pass

  c.restrictor = Hooked(mask=g['run_mask'])
  assert not c._native_loop_ok() and not c._turn_ok()
  assert c._handle.bits is None  # cleared on the device
  c.restrictor = movement.MovementRestrictor(mask=g['run_mask'])
  assert c._native_loop_ok()
  c.restrictor.mask = np.zeros_like(g['run_mask'])
  assert c._handle.read_restriction().any()  # a snapshot ...
  c.refresh_restrictor()
  assert not c._handle.read_restriction().any()  # ... until refreshed
