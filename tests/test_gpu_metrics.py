"""Segmentation metrics on the device (include/ffn_metrics.h through
ffn_amd/metrics.py) against the numpy specification tests/metrics_ref.py.

Everything the device computes is an integer, so every comparison is exact
equality of arrays; no tolerance anywhere.  Shapes: rows of 1, 63, 64, 65, 130
and 257 voxels against the 64 lanes of a wave, whole and with a box whose x
range starts and ends off a multiple of 64, with 8 % of either volume zeroed so
that ignored voxels land inside runs; 40^3 of per-voxel random ids for a crowded
block table (more distinct pairs in a 4,096-voxel span than its 2,048 LDS slots)
and a global table that has to grow (more pairs than its first 2^15 slots);
200 x 208 x 208 for the grid cap, above 2,048 blocks x 4,096 voxels, where spans
lengthen."""

import numpy as np
import pytest

from ffn_amd import _lib
from ffn_amd import metrics
from tests import metrics_ref
from tests.partitions_ref import voronoi_labels

pytestmark = pytest.mark.gpu

WAVE_SHAPES = [(3, 5, 1), (2, 3, 63), (2, 3, 64), (2, 3, 65), (1, 1, 257),
               (5, 7, 130)]


@pytest.fixture(scope='module')
def ops():
  h = metrics.MetricOps(0)
  yield h
  h.close()


def _pair(shape, seed, n_gt=7, n_seg=9, zeros=0.08):
  gt = voronoi_labels(shape, n_gt, seed)
  seg = voronoi_labels(shape, n_seg, seed + 1000, dtype=np.int32, id_base=2,
                       id_step=3)
  rng = np.random.RandomState(seed)
  gt[rng.rand(*shape) < zeros] = 0
  seg[rng.rand(*shape) < zeros] = 0
  return gt, seg


def _assert_table(got, want):
  assert got.gt_ids.dtype == got.seg_ids.dtype == got.counts.dtype == np.uint64
  for g, w in zip(got, want):
    assert np.array_equal(g, w)


def _x_box(shape):
  """A box whose x range starts and ends off a multiple of 64."""
  z, y, x = shape
  return ((0, 0, 1), (z, y, x - 2)) if x >= 4 else ((0, 1, 0), (z, y - 1, x))


# ---- contingency -----------------------------------------------------------------


@pytest.mark.parametrize('shape', WAVE_SHAPES, ids=str)
@pytest.mark.parametrize('ignore', [True, False])
def test_rows_against_the_wave(ops, shape, ignore):
  gt, seg = _pair(shape, seed=sum(shape))
  for core in (None, _x_box(shape)):
    got = ops.contingency(gt, seg, core=core, ignore_gt_zero=ignore)
    _assert_table(got, metrics_ref.contingency(gt, seg, core, ignore))
    ms, nbytes = ops.last_timing()
    lo, hi = core if core else ((0, 0, 0), shape)
    assert nbytes == np.prod(np.subtract(hi, lo)) * (8 + 4)


@pytest.mark.parametrize('gt_dtype', [np.uint32, np.uint64])
@pytest.mark.parametrize('seg_dtype', [np.int32, np.int64])
def test_width_combinations(ops, gt_dtype, seg_dtype):
  shape = (5, 7, 130)
  gt, seg = _pair(shape, seed=3)
  gt, seg = gt.astype(gt_dtype), seg.astype(seg_dtype)
  box = ((1, 2, 3), (5, 6, 129))
  for core in (None, box):
    _assert_table(ops.contingency(gt, seg, core=core),
                  metrics_ref.contingency(gt, seg, core))


@pytest.fixture(scope='module')
def crowded():
  rng = np.random.RandomState(0)
  shape = (40, 40, 40)
  gt = rng.randint(1, 301, shape).astype(np.uint64)
  seg = rng.randint(0, 301, shape).astype(np.int32)
  return gt, seg, metrics_ref.contingency(gt, seg)


def test_crowded_block_table_and_growing_global_table(crowded):
  gt, seg, want = crowded
  # the two facts this case exists for
  assert len(want[0]) > 1 << 15
  keys = (gt.ravel() << np.uint64(32)) | seg.ravel().astype(np.uint64)
  assert gt.size % 4096 != 0 and -(-gt.size // 4096) == 16  # 16 spans of 4,096
  for lo in range(0, gt.size, 4096):
    assert len(np.unique(keys[lo:lo + 4096])) > 2048
  fresh = metrics.MetricOps(0)  # its global table still has its first size
  try:
    _assert_table(fresh.contingency(gt, seg), want)
  finally:
    fresh.close()


@pytest.fixture(scope='module')
def large():
  """200 x 208 x 208: Voronoi cells of a 50 x 52 x 52 grid, every voxel
  repeated 4 times along each axis, the segmentation shifted off that grid."""
  small_gt, small_seg = _pair((50, 52, 52), seed=5, n_gt=40, n_seg=60, zeros=0.0)
  up = lambda v: v.repeat(4, 0).repeat(4, 1).repeat(4, 2)
  gt = up(small_gt)
  seg = np.roll(up(small_seg), (1, 2, 3), (0, 1, 2))
  rng = np.random.RandomState(6)
  gt.reshape(-1)[rng.randint(0, gt.size, gt.size // 12)] = 0
  return gt, seg


def test_grid_cap(ops, large):
  gt, seg = large
  assert gt.shape == (200, 208, 208) and gt.size > 2048 * 4096
  core = ((16, 16, 16), (184, 192, 192))
  for c in (None, core):
    _assert_table(ops.contingency(gt, seg, core=c),
                  metrics_ref.contingency(gt, seg, c))


def test_device_tensors(ops):
  import torch
  shape = (5, 7, 130)
  gt, seg = _pair(shape, seed=8)
  assert gt.dtype == np.uint64 and seg.dtype == np.int32
  gt_dev = torch.from_numpy(gt).to('cuda:0')
  seg_dev = torch.from_numpy(seg).to('cuda:0')
  assert gt_dev.dtype == torch.uint64 and seg_dev.dtype == torch.int32
  box = ((1, 0, 5), (4, 7, 127))
  for core in (None, box):
    want = metrics_ref.contingency(gt, seg, core)
    _assert_table(ops.contingency(gt_dev, seg_dev, core=core), want)
    _assert_table(ops.contingency(gt, seg_dev, core=core), want)
    _assert_table(ops.contingency(gt, seg, core=core), want)


def test_canvas_segmentation_on_the_device(ops, fib25_model):
  """A live canvas' segmentation, copied on the device without its -1
  markers, scores as its host read-out does."""
  import torch
  from ffn_amd import engine as hip_engine
  from ffn_amd import labels
  shape = (12, 20, 70)
  gt, seg = _pair(shape, seed=9)
  seg[np.random.RandomState(1).rand(*shape) < 0.05] = -1
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=1, device_id=0)
  try:
    canvas = eng.create_canvas(np.zeros(shape, np.float32))
    canvas.write_segmentation((0, 0, 0), shape, seg)
    dev = torch.empty(shape, dtype=torch.int32, device='cuda:0')
    labels.default_ops(0).copy_canvas(canvas._h, dev.data_ptr())
    host = canvas.read_segmentation()
    assert (host == -1).any()
    want = metrics_ref.contingency(gt, np.maximum(host, 0))
    _assert_table(ops.contingency(gt, dev), want)
    _assert_table(ops.contingency(gt, host), want)
    canvas.close()
  finally:
    eng.close()


def _raw_contingency(ops, gt, seg, cap, lo=None, hi=None):
  import ctypes
  pg, ps, pc = (np.zeros(max(cap, 1), np.uint64) for _ in range(3))
  found = ctypes.c_size_t(0)
  i64 = lambda v: None if v is None else (ctypes.c_int64 * 3)(*v)
  rc = ops._lib.ffn_metrics_contingency(
      ops._h, gt.ctypes.data, gt.dtype.itemsize, 0, seg.ctypes.data,
      seg.dtype.itemsize, 0, i64(gt.shape), i64(lo), i64(hi), 1, cap,
      pg.ctypes.data, ps.ctypes.data, pc.ctypes.data, ctypes.byref(found))
  return rc, found.value


def test_errors(ops, crowded):
  ERR_ARG = -1
  gt, seg = _pair((2, 3, 65), seed=2)
  seg = seg.astype(np.uint32)
  rc, _ = _raw_contingency(ops, gt, seg, 1 << 10)
  assert rc == 0
  # an id of 2^32 - 1, in either volume and at either width
  for vol in ('gt', 'seg'):
    bad_gt, bad_seg = gt.copy(), seg.copy()
    (bad_gt if vol == 'gt' else bad_seg)[1, 2, 40] = 2**32 - 1
    rc, _ = _raw_contingency(ops, bad_gt, bad_seg, 1 << 10)
    assert rc == ERR_ARG, vol
    with pytest.raises(_lib.FFNHipError, match='2\\^32 - 1'):
      _lib.check(rc)
  # a box outside the volume, or the wrong way round
  for lo, hi in (((0, 0, 0), (2, 3, 66)), ((0, -1, 0), (2, 3, 65)),
                 ((0, 2, 0), (2, 1, 65))):
    rc, _ = _raw_contingency(ops, gt, seg, 1 << 10, lo, hi)
    assert rc == ERR_ARG, (lo, hi)
  with pytest.raises(_lib.FFNHipError):
    ops.contingency(gt, seg, core=((0, 0, 0), (3, 3, 65)))
  # a cap too small: the true number comes back, and the Python retry fits
  want = metrics_ref.contingency(gt, seg)
  rc, found = _raw_contingency(ops, gt, seg, 3)
  assert rc == ERR_ARG and found == len(want[0]) > 3
  big_gt, big_seg, big_want = crowded
  assert len(big_want[0]) > 1 << 15  # the Python layer's first cap
  _assert_table(ops.contingency(big_gt, big_seg), big_want)
  # ids beyond 32 bits in a host volume are remapped and come back
  wide = gt + np.uint64(2**40)
  wide[gt == 0] = 0
  got = ops.contingency(wide, seg)
  assert np.array_equal(got.gt_ids, want[0] + np.uint64(2**40))
  assert np.array_equal(got.seg_ids, want[1])
  assert np.array_equal(got.counts, want[2])


# ---- skeletons -------------------------------------------------------------------


def _assert_edges(got, want):
  assert np.array_equal(got.class_counts, want['class_counts'])
  assert np.array_equal(got.class_lengths, want['class_lengths'])
  runs = sorted(want['runs'].items())
  assert got.run_skeletons.tolist() == [k[0] for k, _ in runs]
  assert got.run_segments.tolist() == [k[1] for k, _ in runs]
  assert got.run_lengths.tolist() == [v for _, v in runs]
  assert got.mergers.tolist() == want['mergers']
  assert np.array_equal(got.node_segment, want['node_segment'])
  assert np.array_equal(got.edge_class, want['edge_class'])


@pytest.mark.parametrize('min_nodes', [2, 1])
def test_skeleton_rules(ops, min_nodes):
  O, M, S, C = metrics.OMITTED, metrics.MERGED, metrics.SPLIT, metrics.CORRECT
  seg = np.array([5, 5, 5, 6, 6, 0, 7, 7, 7, 7, 5], np.int32).reshape(1, 1, 11)
  nodes = np.zeros((11, 3), np.int32)
  nodes[:, 2] = np.arange(11)
  skel = np.array([1] * 8 + [2] * 3, np.uint32)
  edges = np.array([(k, k + 1) for k in range(7)] + [(8, 9), (9, 10)], np.int32)
  got = ops.skeleton_edges(seg, metrics.Skeletons(nodes, skel, edges), min_nodes)
  if min_nodes == 2:
    classes, mergers, runs = [C, C, S, C, O, O, M, M, M], [7], [2048, 1024]
  else:
    classes, mergers, runs = [M, M, M, C, O, O, M, M, M], [5, 7], [1024]
  assert got.edge_class.tolist() == classes
  assert got.mergers.tolist() == mergers
  assert got.run_skeletons.tolist() == [1] * len(runs)
  assert got.run_segments.tolist() == [5, 6][-len(runs):]
  assert got.run_lengths.tolist() == runs
  assert got.class_counts.tolist() == [classes.count(k) for k in range(4)]
  assert got.class_lengths.tolist() == [1024 * classes.count(k)
                                        for k in range(4)]
  assert got.node_segment.tolist() == seg.ravel().tolist()
  erl = metrics.skeleton_scores(got)['expected_run_length']
  assert abs(erl - (5 / 9 if min_nodes == 2 else 1 / 9)) < 1e-12


@pytest.fixture(scope='module')
def skeleton_case():
  shape = (48, 64, 64)
  seg = voronoi_labels(shape, 150, 21, dtype=np.int32)
  nodes, skel, edges = metrics_ref.random_walk_skeletons(shape, 40, 200, 22)
  outside = ((nodes < 0) | (nodes >= np.asarray(shape))).any(1)
  assert outside.any() and not outside.all()
  size = (4.0, 1.5, 1.0)
  return seg, metrics.Skeletons(nodes, skel, edges, size), \
      metrics_ref.edge_lengths_q(nodes, edges, size)


@pytest.mark.parametrize('min_nodes', [1, 3])
def test_skeletons_at_size(ops, skeleton_case, min_nodes):
  import torch
  seg, skeletons, length = skeleton_case
  seg_dev = torch.from_numpy(seg).to('cuda:0')
  for core in (None, ((4, 4, 4), (44, 60, 60))):
    want = metrics_ref.skeleton_edges(
        seg, skeletons.nodes_zyx, skeletons.node_skeleton, skeletons.edges,
        length, min_nodes, core)
    assert all(want['class_counts'] > 0) and want['mergers']
    _assert_edges(ops.skeleton_edges(seg, skeletons, min_nodes, core), want)
    _assert_edges(ops.skeleton_edges(seg.astype(np.uint64), skeletons,
                                     min_nodes, core), want)
    _assert_edges(ops.skeleton_edges(seg_dev, skeletons, min_nodes, core), want)


def test_skeleton_errors(ops):
  seg = np.ones((2, 2, 4), np.int32)
  nodes = np.zeros((3, 3), np.int32)
  with pytest.raises(ValueError, match='two skeletons'):
    ops.skeleton_edges(seg, metrics.Skeletons(
        nodes, np.array([1, 2, 2], np.uint32), np.array([[0, 1]], np.int32)))
  with pytest.raises(ValueError, match='\\[1, 2\\*\\*32 - 2\\]'):
    ops.skeleton_edges(seg, metrics.Skeletons(
        nodes, np.array([1, 0, 2], np.uint32), np.zeros((0, 2), np.int32)))
  # the library checks for itself
  import ctypes
  skel = np.array([1, 2, 2], np.uint32)
  edges = np.array([[0, 1]], np.int32)
  length = np.array([1024], np.uint32)
  out = np.zeros(8, np.uint64)
  n = ctypes.c_size_t(0)
  rc = ops._lib.ffn_metrics_skeleton(
      ops._h, seg.ctypes.data, 4, 0, (ctypes.c_int64 * 3)(*seg.shape), None,
      None, 3, nodes.ctypes.data, skel.ctypes.data, 1, edges.ctypes.data,
      length.ctypes.data, 2, out.ctypes.data, out[4:].ctypes.data, 0, None,
      None, None, ctypes.byref(n), 0, None, ctypes.byref(n), None, None)
  assert rc == -1


# ---- determinism -----------------------------------------------------------------


def test_twice_on_one_handle_is_byte_identical(ops, crowded, skeleton_case):
  gt, seg, _ = crowded
  a, b = ops.contingency(gt, seg), ops.contingency(gt, seg)
  for x, y in zip(a, b):
    assert x.tobytes() == y.tobytes()
  seg, skeletons, _ = skeleton_case
  a, b = (ops.skeleton_edges(seg, skeletons, 1) for _ in range(2))
  for x, y in zip(a, b):
    assert x.tobytes() == y.tobytes()
