"""Resegmentation analysis on the GPU (include/ffn_analysis.h,
ffn_amd/analysis.py, ffn_amd/inference/resegmentation_analysis.py) against the
reference's own results (tests/golden/ref_reseg_analysis.npz) and the numpy /
scipy restatement (tests/reseg_analysis_ref.py)."""
import ctypes
import os

import numpy as np
import pytest

from ffn_amd.inference import request as request_lib
from ffn_amd.inference import resegmentation_analysis as analysis_lib
from tests import reseg_analysis_ref as ra
from tests.test_reseg_analysis import (CASES, ENDPOINTS, PAIRS, call_endpoint,
                                       call_pair, check_endpoint_result,
                                       check_pair_result, seg_volume,
                                       shared_volume_cases)

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope='module')
def analyzer():
  from ffn_amd import analysis
  return analysis.default_analyzer(0)


# ---- the reference's results ------------------------------------------------------

@pytest.mark.parametrize('name', PAIRS)
def test_pair_resegmentation_equals_the_reference(name, tmp_path):
  """Integer fields equal; iou, consistencies and every max_edt equal as f32
  (what the proto's float fields hold)."""
  case = CASES[name]
  path = ra.write_case_file(case, tmp_path)
  if isinstance(case['want'], str):
    with pytest.raises(getattr(analysis_lib, case['want'])):
      call_pair(case, path)
    return
  check_pair_result(call_pair(case, path), case, name)


@pytest.mark.parametrize('name', ENDPOINTS)
def test_endpoint_resegmentation_equals_the_reference(name, tmp_path):
  case = CASES[name]
  path = ra.write_case_file(case, tmp_path)
  if isinstance(case['want'], str):
    with pytest.raises(getattr(analysis_lib, case['want'])):
      call_endpoint(case, path)
    return
  check_endpoint_result(call_endpoint(case, path), case, name)


def test_reference_surface_on_masks(analyzer):
  from scipy import ndimage
  rng = np.random.default_rng(5)
  reseg = rng.random((2, 9, 10, 11)) < 0.4
  want = (reseg[0] & reseg[1]).sum() / float(reseg.max(axis=0).sum())
  assert analysis_lib.compute_iou(reseg) == want
  assert np.isnan(analysis_lib.compute_iou(np.zeros((2, 3, 3, 3), bool)))
  seg1 = rng.random((9, 10, 11)) < 0.3
  seg2 = seg1 ^ (rng.random((9, 10, 11)) < 0.2)
  res = request_lib.SegmentResult()
  analysis_lib.evaluate_segmentation_result(
      reseg[0], np.array([1, 10]), np.array([[2, 2, 2], [9, 8, 8]]), (2, 2, 2),
      (3, 3, 3), seg1, seg2, (33, 8, 8), res)
  assert res.num_voxels == reseg[0].sum() and res.deleted_voxels == 1
  assert res.max_edt == np.float32(ndimage.distance_transform_edt(
      reseg[0], sampling=(33, 8, 8)).max())
  assert res.segment_a_consistency == np.float32(
      reseg[0][seg1].sum() / seg1.sum())
  assert res.segment_b_consistency == np.float32(
      reseg[0][seg2].sum() / seg2.sum())


# ---- batches ------------------------------------------------------------------------

def pair_input(case):
  """The PairInput evaluate_pair_resegmentation forms for a fixture case."""
  from ffn_amd import analysis
  z, y, x = case['point_zyx']
  ar = case['analysis_radius_zyx']
  seg = case['seg'][z - ar[0]:z + ar[0] + 1, y - ar[1]:y + ar[1] + 1,
                    x - ar[2]:x + ar[2] + 1]
  delta = [r - a for r, a in zip(case['radius_zyx'], ar)]
  return analysis.PairInput(case['probs'], seg, delta, case['id_a'],
                            case['id_b'])


def test_every_fixture_pair_in_one_device_batch(analyzer):
  """Boxes of different shapes in one call, and in calls of 1 and 3 points:
  the rows of the single calls, which are the restatement's.  (evaluate_pairs
  takes one radius and one volume per call, so the mixed batch is formed at
  the Analyzer.)"""
  from ffn_amd import analysis
  names = [n for n in PAIRS if CASES[n]['probs'].shape[0] == 2]
  assert len(names) >= 12
  assert len({CASES[n]['probs'].shape for n in names}) >= 5
  for voxel in ((1, 1, 1), (33, 8, 8)):
    for threshold in (0.5, 0.9):
      table = analysis.object_table(threshold)
      items = [pair_input(CASES[n]) for n in names]
      counts, edt = analyzer.pair_stats(items, table, voxel)
      assert counts.shape == (len(names), 10) and edt.shape == (len(names), 4)
      for k, item in enumerate(items):
        want_counts, want_edt = ra.pair_stats(
            item.probs, item.seg, item.offset_zyx, item.id_a, item.id_b,
            ra.object_mask(np.arange(256), threshold), voxel)
        assert np.array_equal(counts[k], want_counts), names[k]
        assert edt[k].tobytes() == want_edt.tobytes(), (names[k], edt[k],
                                                        want_edt)
      for size in (1, 3):
        for first in range(0, len(items), size):
          c, e = analyzer.pair_stats(items[first:first + size], table, voxel)
          assert np.array_equal(c, counts[first:first + size])
          assert e.tobytes() == edt[first:first + size].tobytes()
  analyzer.pair_stats(items[:2], table)
  (ms, voxels), _ = analyzer.last_timing()
  assert ms > 0 and voxels == items[0].seg.size + items[1].seg.size


def same_results(got, want):
  assert len(got) == len(want)
  for a, b in zip(got, want):
    if isinstance(b, Exception):
      assert type(a) is type(b), (a, b)
    else:
      assert a.to_text() == b.to_text()


def test_evaluate_pairs_in_batches_equals_single_calls(tmp_path):
  pair, _, names = shared_volume_cases(tmp_path)
  files = [names[2], names[0], str(tmp_path / '1-2_at_3_4_5.npz'), names[3],
           names[0], names[0], names[3]]
  args = (seg_volume(pair), pair['radius_zyx'], pair['analysis_radius_zyx'],
          pair['voxel_size_zyx'], pair['threshold'])
  single = []
  for f in files:
    try:
      single.append(analysis_lib.evaluate_pair_resegmentation(f, *args))
    except Exception as e:  # pylint:disable=broad-except
      single.append(e)
  check_pair_result(single[1], pair, 'reseg_pair')
  assert [type(s).__name__ for s in single if isinstance(s, Exception)] == [
      'IncompleteResegmentationError', 'FileNotFoundError',
      'InvalidBaseSegmentatonError', 'InvalidBaseSegmentatonError']
  for batch in (None, 1, 3, len(files)):
    same_results(analysis_lib.evaluate_pairs(files, *args, batch=batch), single)


def test_evaluate_endpoints_in_batches_equals_single_calls(tmp_path):
  _, end, names = shared_volume_cases(tmp_path)
  # the pair file read as an endpoint: object A's map, seeded from id_a
  files = [names[1], names[0], str(tmp_path / '1-0_at_3_4_5.npz'), names[3],
           names[1]]
  args = (seg_volume(end), end['radius_zyx'], end['threshold'])
  single = []
  for f in files:
    try:
      single.append(analysis_lib.evaluate_endpoint_resegmentation(f, *args))
    except Exception as e:  # pylint:disable=broad-except
      single.append(e)
  check_endpoint_result(single[0], end, 'reseg_endpoint')
  assert isinstance(single[1], request_lib.EndpointResegmentationResult)
  assert isinstance(single[2], FileNotFoundError)
  assert isinstance(single[3], analysis_lib.InvalidBaseSegmentatonError)
  for batch in (None, 1, 3, len(files)):
    same_results(analysis_lib.evaluate_endpoints(files, *args, batch=batch),
                 single)


# ---- the kernels against the restatement ------------------------------------------

SHAPES = [((17, 40, 9), (17, 40, 9), (0, 0, 0)),
          ((1, 65, 130), (1, 65, 130), (0, 0, 0)),
          ((23, 50, 70), (17, 40, 9), (3, 7, 60)),
          ((5, 70, 140), (1, 65, 130), (4, 5, 10)),
          ((65, 3, 64), (65, 1, 64), (0, 1, 0)),
          ((30, 31, 33), (21, 31, 33), (9, 0, 0)),
          ((2, 2, 300), (1, 1, 257), (1, 0, 43))]


def random_batch(seed):
  from ffn_amd import analysis
  rng = np.random.default_rng(seed)
  items = []
  for k, (box, crop, offset) in enumerate(SHAPES):
    q, seg, off, id_a, id_b = ra.random_pair_point(
        rng, box, crop, offset, fill=(0.3, 0.5, 0.7)[k % 3])
    items.append(analysis.PairInput(q, seg, off, id_a, id_b))
  return items


def restated(items, table, voxel):
  rows = [ra.pair_stats(p.probs, p.seg, p.offset_zyx, p.id_a, p.id_b, table,
                        voxel) for p in items]
  return (np.array([r[0] for r in rows], np.uint64),
          np.array([r[1] for r in rows]))


@pytest.mark.parametrize('voxel', [(1, 1, 1), (33, 8, 8)])
def test_pair_stats_on_random_boxes_is_exact(analyzer, voxel):
  from ffn_amd import analysis
  items = random_batch(7)
  for threshold in (0.5, 0.75):
    table = analysis.object_table(threshold)
    counts, edt = analyzer.pair_stats(items, table, voxel)
    want_counts, want_edt = restated(items, table, voxel)
    assert counts[:, :6].min() > 0  # every mask of every point has voxels
    assert np.all(np.isfinite(want_edt)) and want_edt.min() > 0
    assert np.array_equal(counts, want_counts)
    # integer voxel sizes: squared distances are exact, one correctly rounded
    # root: scipy's f64 bit for bit
    assert edt.tobytes() == want_edt.tobytes(), (edt, want_edt)


def test_pair_stats_non_integer_voxel_size(analyzer):
  """8 eps relative: two products, two sums and a root leave each side within
  about 4 eps of the real value (the bound test_expand_non_integer_voxel_size
  derives for the same arithmetic)."""
  from ffn_amd import analysis
  items = random_batch(8)
  table = analysis.object_table(0.5)
  voxel = (35.7, 4.3, 4.3)
  counts, edt = analyzer.pair_stats(items, table, voxel)
  want_counts, want_edt = restated(items, table, voxel)
  assert np.array_equal(counts, want_counts)
  print('\nmax relative difference / eps:',
        (np.abs(edt - want_edt) / (EPS * want_edt)).max())
  assert np.all(np.abs(edt - want_edt) <= 8 * EPS * want_edt), (edt, want_edt)


def test_empty_and_full_masks(analyzer):
  from ffn_amd import analysis
  table = analysis.object_table(0.5)
  shape = (6, 7, 70)
  probs = np.zeros((2,) + shape, np.uint8)
  probs[1] = 255
  seg = np.full(shape, 9, np.uint64)
  item = analysis.PairInput(probs, seg, (0, 0, 0), 9, 4)
  for voxel in ((1, 1, 1), (33, 8, 8)):
    counts, edt = analyzer.pair_stats([item], table, voxel)
    n = seg.size
    assert counts[0].tolist() == [0, n, 0, n, n, 0, 0, 0, n, 0]
    # A empty, B full, S1 full, S2 empty
    assert edt[0].tolist() == [0.0, float('inf'), float('inf'), 0.0]
  one = probs.copy()
  one[1, 5, 6, 69] = 1  # a single 0 voxel in the far corner pins B
  _, edt = analyzer.pair_stats(
      [analysis.PairInput(one, seg, (0, 0, 0), 9, 4)], table, (33, 8, 8))
  assert edt[0, 1] == np.sqrt((5 * 33.0)**2 + (6 * 8.0)**2 + (69 * 8.0)**2)
  with pytest.raises(Exception, match='crop leaves the box'):
    analyzer.pair_stats([analysis.PairInput(probs, seg, (0, 0, 1), 9, 4)], table)
  assert analyzer.pair_stats([], table)[0].shape == (0, 10)


def endpoint_batch(seed):
  from ffn_amd import analysis
  rng = np.random.default_rng(seed)
  items = []
  for box, _, _ in SHAPES:
    q, seg, _, id_a, _ = ra.random_pair_point(rng, box, box, (0, 0, 0), n_ids=8)
    items.append(analysis.EndpointInput(q[0], seg, id_a))
  # an id that occurs but is never overlapped, asked for and not asked for
  q = np.zeros((4, 5, 6), np.uint8)
  seg = np.full((4, 5, 6), 3, np.uint64)
  seg[0, 0, 0] = 8
  q[0, 0, 0] = 255
  items.append(analysis.EndpointInput(q, seg, 3))
  items.append(analysis.EndpointInput(q, seg))
  items.append(analysis.EndpointInput(q, seg, 77))  # absent
  return items


def test_endpoint_overlaps_equal_the_restatement(analyzer):
  from ffn_amd import analysis
  items = endpoint_batch(21)
  for threshold in (0.5, 0.9):
    table = analysis.object_table(threshold)
    got = analyzer.endpoint_overlaps(items, table)
    want = [ra.endpoint_overlaps(p.probs, p.seg, table, p.id) for p in items]
    assert got == want
    for size in (1, 3):
      for first in range(0, len(items), size):
        assert analyzer.endpoint_overlaps(items[first:first + size],
                                          table) == want[first:first + size]
  assert got[-3][1] == {8: (1, 1), 3: (0, 119)}
  assert got[-2][1] == {8: (1, 1)} and got[-1][1] == {8: (1, 1)}
  assert 0 in got[0][1]  # the background counts as an id
  analyzer.endpoint_overlaps(items[-3:], table)
  _, (ms, voxels) = analyzer.last_timing()
  assert ms > 0 and voxels == 3 * 120


def test_more_ids_than_the_first_capacities(analyzer):
  """More distinct ids than the caller's first row buffer, than a block's LDS
  table and than the first per-point global table."""
  from ffn_amd import _lib
  from ffn_amd import analysis
  rng = np.random.default_rng(3)
  shape = (20, 21, 22)  # 9240 voxels, every one an id of its own
  seg = (rng.permutation(np.prod(shape)).astype(np.uint64) * 2**33 +
         5).reshape(shape)
  seg[0, 0, :2] = 0
  q = rng.integers(0, 256, shape).astype(np.uint8)
  few = analysis.EndpointInput(q[:3], np.minimum(seg[:3], 2**33 * 40 + 5))
  items = [few, analysis.EndpointInput(q, seg), few]
  table = analysis.object_table(0.5)
  want = [ra.endpoint_overlaps(p.probs, p.seg, table) for p in items]
  assert len(want[1][1]) > 4096
  saved = analyzer.initial_cap
  try:
    analyzer.initial_cap = 100
    got = analyzer.endpoint_overlaps(items, table)
  finally:
    analyzer.initial_cap = saved
  assert got == want
  # the C-ABI reports the true count and writes nothing past cap
  lib = _lib.load()
  descs = (_lib.EndpointDesc * 1)()
  probs, segc = np.ascontiguousarray(q), np.ascontiguousarray(seg)
  descs[0].probs, descs[0].seg = probs.ctypes.data, segc.ctypes.data
  descs[0].shape_zyx[:] = shape
  rows = np.full(8, -7, np.int32)
  old = np.zeros(8, np.uint64)
  cnt = np.zeros((8, 2), np.uint32)
  num_new = np.zeros(1, np.uint64)
  found = ctypes.c_size_t(0)
  rc = lib.ffn_analyzer_endpoint_overlaps(
      analyzer._h, descs, 1, table.ctypes.data, 4, rows.ctypes.data,
      old.ctypes.data, cnt.ctypes.data, num_new.ctypes.data,
      ctypes.byref(found))
  assert rc != 0 and found.value == len(want[1][1])
  assert np.all(rows == -7) and not old.any()


# ---- end to end -----------------------------------------------------------------------

def case_from_file(path, request, point_num, init_seg):
  """A restatement case from a file process_many wrote."""
  p = request.points[point_num]
  with np.load(path, allow_pickle=True) as d:
    probs = d['probs']
    deletes = [np.asarray(v) for v in d['deletes']]
    histories = [np.asarray(v).reshape(-1, 3) for v in d['histories']]
    starts = [np.array(v).reshape(-1, 3) for v in d['start_points']]
  r, ar = request.radius, request.analysis_radius
  return {'kind': 'pair' if p.HasField('id_b') else 'endpoint',
          'probs': probs, 'seg': init_seg, 'deletes': deletes,
          'histories': histories, 'start_points': starts,
          'point_zyx': [p.point.z, p.point.y, p.point.x],
          'radius_zyx': [r.z, r.y, r.x],
          'analysis_radius_zyx': [ar.z, ar.y, ar.x],
          'voxel_size_zyx': [1, 1, 1], 'threshold': 0.6,
          'id_a': p.id_a, 'id_b': p.id_b}


def test_process_many_feeds_evaluate_request(fib25_model, tmp_path):
  """process_many on the ref_reseg.npz request, then evaluate_request on what
  it wrote: the restatement's numbers for the same files."""
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import resegmentation
  from tests import test_resegmentation as tr
  g = np.load(os.path.join(ra.GOLDEN, 'ref_reseg.npz'), allow_pickle=True)
  g = {k: g[k] for k in g.files}
  request = tr.build_request(g, tmp_path)
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None,
                                  inference_utils.Counters(), 2)
  runner = tr.StandInRunner(
      g, lambda counters: exe.get_client(counters, direct=True),
      request.inference)
  resegmentation.process_many(request, runner, (1, 1, 1), engine=exe.engine)
  assert len(os.listdir(str(tmp_path))) == 2
  got = analysis_lib.evaluate_request(request, runner.init_seg_volume,
                                      (1, 1, 1), threshold=0.6)
  assert len(got) == 2
  paths = [analysis_lib.result_path(request, n) for n in range(2)]
  pair = case_from_file(paths[0], request, 0, g['init_seg'])
  pair['want'] = ra.evaluate_pair(pair)
  assert not isinstance(pair['want'], str)
  check_pair_result(got[0], pair, 'pair')
  assert got[0].eval.from_a.num_voxels > 1000 and 0 < got[0].eval.iou < 1
  end = case_from_file(paths[1], request, 1, g['init_seg'])
  want = ra.evaluate_endpoint(end)
  assert ra.endpoint_result_fields(got[1]) == dict(
      want, segmentation_radius=[24, 24, 24])
  assert got[1].source.num_overlapping > 1000
