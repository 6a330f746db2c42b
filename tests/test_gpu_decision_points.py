"""Decision points on the GPU (include/ffn_decision.h, ffn_amd/decision.py,
ffn_amd/utils/decision_point.py) against the numpy restatement
(tests/decision_ref.py) and the reference's own results
(tests/golden/ref_decision_points.npz)."""
import os

import numpy as np
import pytest

from tests import decision_ref
from tests.test_decision_points import (CASES, assert_matches_fixture,
                                        small_volume)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def ops():
  from ffn_amd import decision
  return decision.default_ops(0)


def check_expand(ops, seg, voxel_size, max_distances=(None,)):
  """watershed_expand == expand_spec: ids exactly, distances bit for bit."""
  want_ids, want_edt = decision_ref.expand_spec(seg, voxel_size)
  for maxd in max_distances:
    got_ids, got_edt = ops.watershed_expand(seg, voxel_size, maxd)
    want = want_ids.copy()
    if maxd is not None:
      want[want_edt > maxd] = 0
    assert got_ids.dtype == seg.dtype and got_ids.shape == seg.shape
    assert got_edt.dtype == np.float64
    assert got_edt.tobytes() == want_edt.tobytes(), (seg.shape, voxel_size, maxd)
    assert np.array_equal(got_ids, want), (seg.shape, voxel_size, maxd)
  return want_ids, want_edt


@pytest.mark.parametrize('voxel_size', [(1, 1, 1), (8, 8, 33)])
@pytest.mark.parametrize('name', sorted(CASES))
def test_expand_equals_spec_on_fixture_volumes(ops, name, voxel_size):
  # 40.0 bites with the 33-unit axis; 0.5 (7.0) is less than one voxel
  below_one_voxel = 0.5 * min(voxel_size) + (3.0 if min(voxel_size) > 1 else 0)
  ids, edt = check_expand(ops, CASES[name]['seg'], voxel_size,
                          (None, 40.0, below_one_voxel))
  unl = CASES[name]['seg'] == 0
  assert np.all(edt[unl] > below_one_voxel) and np.any(ids[unl] > 0)


def test_expand_dtypes(ops):
  seg64 = small_volume()
  ranks = np.unique(seg64, return_inverse=True)[1].reshape(seg64.shape)
  assert ranks.max() < 256
  results = []
  for dtype in (np.uint64, np.uint32, np.int32, np.uint8):
    seg = ranks.astype(dtype)
    check_expand(ops, seg, (8, 8, 33), (None, 40.0))
    results.append(ops.watershed_expand(seg, (8, 8, 33))[0].astype(np.int64))
  assert all(np.array_equal(results[0], r) for r in results[1:])


def test_expand_non_integer_voxel_size(ops):
  """Nearest up to f64 rounding: two products, two sums and a root leave each
  side within about 4 eps of the real value, hence 8 eps between them."""
  seg = small_volume()
  voxel_size = (4.3, 4.3, 35.7)
  sx, sy, sz = voxel_size
  got_ids, got_edt = ops.watershed_expand(seg, voxel_size)
  want_edt, _, _ = decision_ref.brute_force_expand(seg, voxel_size)
  assert np.all(np.abs(got_edt - want_edt) <= 8 * EPS * want_edt)
  lab = np.argwhere(seg > 0)
  lab_ids = seg[seg > 0]
  for v in np.ndindex(*seg.shape):
    tx = (lab[:, 2] - v[2]) * sx
    ty = (lab[:, 1] - v[1]) * sy
    tz = (lab[:, 0] - v[0]) * sz
    d = np.sqrt((tx * tx + ty * ty) + tz * tz)
    near = np.abs(d - got_edt[v]) <= 8 * EPS * got_edt[v]
    assert got_ids[v] in lab_ids[near], v


@pytest.mark.parametrize('shape', [(1, 65, 40), (65, 1, 33), (20, 33, 1),
                                   (1, 1, 65), (3, 130, 67)])
def test_expand_shapes_with_a_dimension_of_1_and_65(ops, shape):
  seg = decision_ref.synthetic_segmentation(shape, seed=sum(shape), gap=3,
                                            drop=0.3, dtype=np.uint32)
  assert np.any(seg == 0) and np.any(seg > 0)
  check_expand(ops, seg, (8, 8, 33), (None, 40.0))
  check_expand(ops, seg, (1, 1, 1))


@pytest.mark.parametrize('axis', [1, 0])
def test_expand_keeps_a_parabola_that_only_touches(ops, axis):
  seg, centre = decision_ref.touching_parabola_volume(axis)
  ids, edt = check_expand(ops, seg, (1, 1, 1))
  assert ids[centre] == 3 and edt[centre] == 2.0
  got, _ = ops.watershed_expand(seg, (1, 1, 1))
  assert got[centre] == 3


def test_expand_degenerate_volumes(ops):
  full = np.full((7, 9, 70), 9, np.uint64)
  ids, edt = ops.watershed_expand(full, (8, 8, 33), 40.0)
  assert np.array_equal(ids, full) and not edt.any()
  assert ops.contact_minima()['a'].size == 0
  empty = np.zeros((7, 9, 70), np.uint32)
  ids, edt = ops.watershed_expand(empty, (1, 1, 1))
  assert not ids.any() and np.all(np.isinf(edt)) and np.all(edt > 0)
  assert ops.contact_minima()['a'].size == 0
  one = empty.copy()
  one[3, 4, 5] = 2**32 - 2  # the largest id the device takes as it is
  ids, edt = check_expand(ops, one, (8, 8, 33))
  assert np.all(ids == 2**32 - 2)


def test_expand_mid_size_anisotropic(ops):
  """~160^3, a few hundred ids, (8, 8, 33) voxels, holes tens of voxels wide."""
  rng = np.random.RandomState(11)
  coarse = decision_ref.synthetic_segmentation((25, 27, 26), seed=11, gap=1,
                                               drop=0.2, dtype=np.uint32,
                                               block=(2, 6))
  seg = np.repeat(np.repeat(np.repeat(coarse, 6, 0), 6, 1), 6, 2)[:, :157, :155]
  seg[rng.rand(*seg.shape) < 0.002] = 0
  assert seg.shape == (150, 157, 155)
  assert 100 < len(np.unique(seg)) < 1000
  check_expand(ops, seg, (8, 8, 33), (None, 40.0))
  (ms, nbytes), _ = ops.last_timing()
  assert ms > 0 and nbytes >= seg.size * (4 + 60)


def fixture_call(name, seg=None, **kw):
  from ffn_amd.utils import decision_point
  case = CASES[name]
  return decision_point.find_decision_points(
      case['seg'] if seg is None else seg, case['voxel_size'],
      max_distance=case['max_distance'], subvol_box=case['subvol'],
      optimize_sparse=case['sparse'], sparse_noise_threshold=case['noise'],
      **kw)


@pytest.mark.parametrize('name', sorted(CASES))
def test_find_decision_points_equals_the_reference(name):
  seg = CASES[name]['seg'].copy()
  assert_matches_fixture(fixture_call(name, seg), CASES[name])
  assert np.array_equal(seg, CASES[name]['seg'])  # the input is left alone


def test_contact_minima_equals_the_fixture_candidates(ops):
  for name in ('iso', 'subvol', 'big_ids'):
    case = CASES[name]
    ops.expand(case['seg'], case['voxel_size'], case['max_distance'])
    box = None
    if case['subvol'] is not None:
      lo = case['subvol'][0][::-1]
      box = (lo, [a + b for a, b in zip(lo, case['subvol'][1][::-1])])
    got = ops.contact_minima(box)
    keys = ('a', 'b', 'off', 'z', 'y', 'x')
    order = np.lexsort([got[k] for k in keys[::-1]])
    want = case['cands']
    worder = np.lexsort([want[k] for k in keys[::-1]])
    for k in keys:
      assert np.array_equal(got[k][order], want[k][worder]), (name, k)
    assert got['dist'][order].tobytes() == want['dist'][worder].tobytes()
    _, (ms, nbytes) = ops.last_timing()
    assert ms > 0 and nbytes > 0


def test_subvol_box_object_equals_tuple():
  class Box:
    def to_slice3d(self):
      return np.index_exp[3:34, 7:36, 5:42]

  from ffn_amd.utils import decision_point
  case = CASES['subvol']
  assert case['subvol'] == ((5, 7, 3), (37, 29, 31))
  got = decision_point.find_decision_points(case['seg'], case['voxel_size'],
                                            subvol_box=Box())
  assert_matches_fixture(got, case)


def assert_same_dict(a, b):
  assert sorted(a) == sorted(b) and len(a) > 10
  for k in a:
    assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]), k


def test_device_inputs_equal_the_host_path():
  """An int32 device tensor, a raw (pointer, shape) and a DeviceCanvas'
  segmentation with -1 markers give the dict of the host path."""
  import torch
  import bench
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.training.models import convstack_3d
  from ffn_amd.utils import decision_point
  case = CASES['aniso_max']
  ranks = np.unique(case['seg'], return_inverse=True)[1].reshape(
      case['seg'].shape).astype(np.int32)
  marked = ranks.copy()
  marked[(ranks == 0) & (np.random.RandomState(3).rand(*ranks.shape) < 0.2)] = -1
  assert (marked == -1).sum() > 100
  kw = dict(voxel_size=case['voxel_size'], max_distance=40.0,
            subvol_box=((2, 3, 4), (30, 40, 25)))
  want = decision_point.find_decision_points(ranks.astype(np.uint64), **kw)

  tensor = torch.from_numpy(marked).to('cuda:0')
  assert_same_dict(decision_point.find_decision_points(tensor, **kw), want)
  assert torch.equal(tensor.cpu(), torch.from_numpy(marked))  # only read
  assert_same_dict(decision_point.find_decision_points(
      (tensor.data_ptr(), tuple(tensor.shape)), **kw), want)
  with pytest.raises(TypeError):
    decision_point.find_decision_points(tensor.to(torch.int64), **kw)

  model = convstack_3d.ConvStack3DFFNModel(fov_size=[33, 33, 33],
                                           deltas=[8, 8, 8], depth=12)
  model.load_checkpoint(os.path.join(GOLDEN, 'fib25_weights.npz'))
  request = bench.make_request()
  counters = inference_utils.Counters()
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), model,
                                  model.info, None, counters, 1)
  canvas = inference.DeviceCanvas(
      model.info, exe.get_client(counters, direct=True),
      np.zeros(marked.shape, np.float32), request.inference_options,
      counters=counters,
      movement_policy_fn=movement.get_policy_fn(request, model.info))
  canvas.segmentation[...] = marked
  assert_same_dict(decision_point.find_decision_points(canvas, **kw), want)
  assert_same_dict(
      decision_point.find_decision_points(canvas.segmentation, **kw), want)
  assert np.array_equal(np.asarray(canvas.segmentation), marked)
  canvas.close()


def test_more_candidates_than_the_first_cap(ops):
  case = CASES['iso']
  ops.expand(case['seg'], case['voxel_size'])
  want = ops.contact_minima()
  assert want['a'].size > 1000
  saved = ops.initial_cap
  try:
    ops.initial_cap = 100
    got = ops.contact_minima()
  finally:
    ops.initial_cap = saved
  keys = ('a', 'b', 'off', 'z', 'y', 'x')
  for k in keys + ('dist',):
    assert np.array_equal(got[k][np.lexsort([got[j] for j in keys[::-1]])],
                          want[k][np.lexsort([want[j] for j in keys[::-1]])])
  # the C-ABI reports the true count and writes nothing past cap
  import ctypes
  from ffn_amd import _lib
  lib = _lib.load()
  pa = np.zeros(8, np.uint64)
  pb = np.zeros(8, np.uint64)
  dist = np.zeros(8)
  off = np.full((8, 4), -7, np.int32)
  found = ctypes.c_size_t(0)
  rc = lib.ffn_decision_contact_minima(
      ops._h, None, None, 4, pa.ctypes.data, pb.ctypes.data, dist.ctypes.data,
      off.ctypes.data, ctypes.byref(found))
  assert rc != 0 and found.value == want['a'].size
  assert not pa.any() and np.all(off == -7)


def test_points_feed_process_many(fib25_model, tmp_path):
  """End to end: decision points of a segmentation become a
  ResegmentationRequest that process_many accepts (files are written)."""
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import resegmentation
  from ffn_amd.utils import decision_point
  from tests import test_resegmentation as tr
  g = np.load(os.path.join(GOLDEN, 'ref_reseg.npz'), allow_pickle=True)
  g = {k: g[k] for k in g.files}
  # searched where the request's 24 voxels of context exist on every side
  inner = ((24, 24, 24), (31, 31, 31))
  points = decision_point.find_decision_points(
      g['init_seg'], (1, 1, 1), max_distance=10.0, subvol_box=inner)
  assert len(points) >= 2
  chosen = {k: points[k] for k in sorted(points)[:2]}
  request = tr.build_request(g, tmp_path)
  del request.points[:]
  decision_point.to_resegmentation_points(chosen, request, inner)
  assert len(request.points) == 2
  chosen = {k: (v[0], v[1] + 24) for k, v in chosen.items()}
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None,
                                  inference_utils.Counters(), 2)
  runner = tr.StandInRunner(
      g, lambda counters: exe.get_client(counters, direct=True),
      request.inference)
  resegmentation.process_many(request, runner, (1, 1, 1), engine=exe.engine)
  written = sorted(os.listdir(str(tmp_path)))
  want = sorted('%d-%d_at_%d_%d_%d.npz' % (a, b, *chosen[(a, b)][1])
                for a, b in chosen)
  assert written == want


def test_more_pairs_than_the_first_table():
  """Every voxel an id of its own: more distinct pairs than the 2^18 slots the
  pair table starts with, so it has to grow, and 4,096 voxels per block against
  1,024 block-local slots, so most candidates go straight to the global table."""
  from ffn_amd import decision
  rng = np.random.default_rng(7)
  shape = (48, 48, 48)
  seg = (rng.permutation(48**3) + 1).astype(np.uint32).reshape(shape)
  seg[rng.random(shape) < 0.3] = 0
  voxel_size = (8, 8, 33)
  want = decision_ref.minimising_spec(
      decision_ref.candidates_spec(*decision_ref.expand_spec(seg, voxel_size)))
  pairs = np.unique(np.stack([want['a'], want['b']]), axis=1).shape[1]
  assert pairs > 1 << 18
  fresh = decision.DecisionOps(0)  # a table no earlier test has grown
  try:
    fresh.expand(seg, voxel_size)
    got = fresh.contact_minima()
  finally:
    fresh.close()
  keys = ('a', 'b', 'off', 'z', 'y', 'x')
  got_order = np.lexsort([got[j] for j in keys[::-1]])
  want_order = np.lexsort([want[j] for j in keys[::-1]])
  for k in keys:
    assert np.array_equal(got[k][got_order], want[k][want_order])
  assert got['dist'][got_order].tobytes() == want['dist'][want_order].tobytes()
