"""Segmentation metrics without a GPU: the numpy specification
(tests/metrics_ref.py) against the worked examples of DESIGN.md, the host half
of the product (metrics.segmentation_scores / skeleton_scores, pure functions
of integer tables) against the specification, and evaluate_segmentation.py end
to end over an ops stand-in backed by the specification.

Integers are compared exactly.  Floats: 1e-12 on the worked examples; 1e-9
relative between product and specification -- both sum <= 1e5 non-negative
f64 terms, which bounds their distance by about 1e-11."""

import json
from fractions import Fraction

import numpy as np
import pytest

import evaluate_segmentation
from ffn_amd import metrics
from tests import metrics_ref
from tests.partitions_ref import voronoi_labels

GT = np.array([1, 1, 1, 1, 2, 2, 2, 2, 2, 0, 0], np.uint64).reshape(1, 1, 11)
SEG = np.array([5, 5, 5, 6, 6, 7, 7, 0, 0, 5, 9], np.int32).reshape(1, 1, 11)

# the skeleton example: eleven nodes along x, two skeletons, chain edges
NODE_SEG = np.array([5, 5, 5, 6, 6, 0, 7, 7, 7, 7, 5], np.int32)
NODES = np.stack([np.zeros(11, np.int32), np.zeros(11, np.int32),
                  np.arange(11, dtype=np.int32)], 1)
NODE_SKEL = np.array([1] * 8 + [2] * 3, np.uint32)
EDGES = np.array([(k, k + 1) for k in range(7)] + [(8, 9), (9, 10)], np.int32)
O, M, S, C = (metrics_ref.OMITTED, metrics_ref.MERGED, metrics_ref.SPLIT,
              metrics_ref.CORRECT)


def _product_table(table):
  return metrics.ContingencyTable(*table)


def _product_edges(r):
  runs = sorted(r['runs'].items())
  return metrics.SkeletonEdges(
      r['class_counts'], r['class_lengths'],
      np.array([k[0] for k, _ in runs], np.uint64),
      np.array([k[1] for k, _ in runs], np.uint64),
      np.array([v for _, v in runs], np.uint64),
      np.array(r['mergers'], np.uint64), r['node_segment'], r['edge_class'])


class SpecOps:
  """MetricOps whose device is the specification (no GPU): what the root
  script sees of ffn_amd.metrics."""

  def contingency(self, gt, seg, core=None, ignore_gt_zero=True):
    return _product_table(metrics_ref.contingency(gt, seg, core,
                                                  ignore_gt_zero))

  def skeleton_edges(self, seg, skeletons, merge_min_nodes=2, core=None):
    length = metrics_ref.edge_lengths_q(skeletons.nodes_zyx, skeletons.edges,
                                        skeletons.voxel_size_zyx)
    return _product_edges(metrics_ref.skeleton_edges(
        seg, skeletons.nodes_zyx, skeletons.node_skeleton, skeletons.edges,
        length, merge_min_nodes, core))


# ---- the worked examples ---------------------------------------------------------


def test_worked_example_table():
  g, s, c = metrics_ref.contingency(GT, SEG)
  assert list(zip(g.tolist(), s.tolist(), c.tolist())) == [
      (1, 5, 3), (1, 6, 1), (2, 0, 2), (2, 6, 1), (2, 7, 2)]
  g, s, c = metrics_ref.contingency(GT, SEG, ignore_gt_zero=False)
  assert list(zip(g.tolist(), s.tolist(), c.tolist())) == [
      (0, 5, 1), (0, 9, 1), (1, 5, 3), (1, 6, 1), (2, 0, 2), (2, 6, 1),
      (2, 7, 2)]
  g, s, c = metrics_ref.contingency(GT, SEG, core=((0, 0, 2), (1, 1, 6)))
  assert list(zip(g.tolist(), s.tolist(), c.tolist())) == [
      (1, 5, 1), (1, 6, 1), (2, 6, 1), (2, 7, 1)]


@pytest.mark.parametrize('scores', [metrics_ref.segmentation_scores,
                                    metrics.segmentation_scores],
                         ids=['specification', 'product'])
def test_worked_example_voxel_scores(scores):
  table = _product_table(metrics_ref.contingency(GT, SEG))
  r = scores(table, 'segment')
  assert (r['n_voxels'], r['sum_sq_pairs'], r['sum_sq_gt'],
          r['sum_sq_seg']) == (9, 19, 41, 21)
  assert abs(r['rand_precision'] - 19 / 21) < 1e-12
  assert abs(r['rand_recall'] - 19 / 41) < 1e-12
  assert abs(r['adapted_rand_error'] - 12 / 31) < 1e-12
  assert abs(r['vi_merge'] - 2 / 9) < 1e-12
  assert abs(r['vi_split'] - 1.2060836635859267) < 1e-12
  assert (r['n_split_objects'], r['n_missed_objects'],
          r['n_merging_segments']) == (2, 0, 1)
  r = scores(table, 'singletons')
  assert (r['n_voxels'], r['sum_sq_pairs'], r['sum_sq_gt'],
          r['sum_sq_seg']) == (9, 17, 41, 19)
  assert abs(r['adapted_rand_error'] - 13 / 30) < 1e-12
  assert abs(r['vi_split'] - 1.428305885808149) < 1e-12
  assert abs(r['vi_merge'] - 2 / 9) < 1e-12


def test_worked_example_objects():
  table = _product_table(metrics_ref.contingency(GT, SEG))
  r = metrics.segmentation_scores(table)
  o = r['objects']
  assert o['id'].tolist() == [1, 2]
  assert o['size'].tolist() == [4, 5]
  assert o['pieces'].tolist() == [2, 2]
  assert o['best_segment'].tolist() == [5, 7]
  assert o['best_overlap'].tolist() == [3, 2]
  np.testing.assert_allclose(o['best_iou'], [3 / 4, 2 / 5], rtol=0, atol=1e-15)
  s = r['segments']
  assert s['id'].tolist() == [5, 6, 7]
  assert s['size'].tolist() == [3, 2, 2]
  assert s['objects'].tolist() == [1, 2, 1]
  # min_overlap 2: the one-voxel overlaps are no pieces
  r = metrics.segmentation_scores(table, min_overlap=2)
  assert r['objects']['pieces'].tolist() == [1, 1]
  assert r['segments']['objects'].tolist() == [1, 0, 1]
  assert (r['n_split_objects'], r['n_merging_segments']) == (0, 0)


def test_best_segment_tie_goes_to_the_smaller_id():
  table = metrics.ContingencyTable(np.array([4, 4, 4], np.uint64),
                                   np.array([9, 3, 0], np.uint64),
                                   np.array([2, 2, 7], np.uint64))
  for fn in (metrics.segmentation_scores, metrics_ref.segmentation_scores):
    r = fn(table)
    o = r['objects']
    best = (o['best_segment'].tolist() if isinstance(o, dict) and 'id' in o
            else [o[4]['best_segment']])
    assert best == [3]


@pytest.mark.parametrize('min_nodes,mergers,classes,runs,erl', [
    (2, [7], [C, C, S, C, O, O, M, M, M], {(1, 5): 2048, (1, 6): 1024},
     Fraction(5, 9)),
    (1, [5, 7], [M, M, M, C, O, O, M, M, M], {(1, 6): 1024}, Fraction(1, 9)),
])
def test_worked_example_skeleton(min_nodes, mergers, classes, runs, erl):
  seg = NODE_SEG.reshape(1, 1, 11)
  length = metrics_ref.edge_lengths_q(NODES, EDGES, (1, 1, 1))
  assert length.tolist() == [1024] * 9
  r = metrics_ref.skeleton_edges(seg, NODES, NODE_SKEL, EDGES, length, min_nodes)
  assert r['mergers'] == mergers
  assert r['edge_class'].tolist() == classes
  assert r['runs'] == runs
  assert r['node_segment'].tolist() == NODE_SEG.tolist()
  assert r['class_counts'].tolist() == [classes.count(k) for k in range(4)]
  assert r['class_lengths'].tolist() == [1024 * classes.count(k)
                                         for k in range(4)]
  num, den, value = metrics_ref.expected_run_length(r)
  assert Fraction(num, den) == erl
  s = metrics.skeleton_scores(_product_edges(r))
  assert abs(s['expected_run_length'] - float(erl)) < 1e-12
  assert abs(value - float(erl)) < 1e-12
  assert s['n_edges'] == 9 and s['correct_edges'] == classes.count(C)
  assert abs(s['merged_length_fraction'] - classes.count(M) / 9) < 1e-12
  assert metrics.edge_lengths_q(metrics.Skeletons(
      NODES, NODE_SKEL, EDGES)).tolist() == length.tolist()


# ---- product host half against the specification --------------------------------


def _random_pair(seed, shape=(12, 20, 24)):
  gt = voronoi_labels(shape, 17, seed)
  seg = voronoi_labels(shape, 23, seed + 100, dtype=np.uint32, id_base=3,
                       id_step=5)
  rng = np.random.RandomState(seed)
  gt[rng.rand(*shape) < 0.08] = 0
  seg[rng.rand(*shape) < 0.08] = 0
  return gt, seg


FLOATS = ('rand_precision', 'rand_recall', 'adapted_rand_error', 'vi_split',
          'vi_merge', 'mean_best_iou')
INTS = ('n_voxels', 'sum_sq_pairs', 'sum_sq_gt', 'sum_sq_seg',
        'n_split_objects', 'n_missed_objects', 'n_merging_segments')


@pytest.mark.parametrize('background', ['segment', 'singletons'])
@pytest.mark.parametrize('min_overlap', [1, 40])
def test_segmentation_scores_match_specification(background, min_overlap):
  for seed in (1, 2):
    gt, seg = _random_pair(seed)
    table = metrics_ref.contingency(gt, seg)
    want = metrics_ref.segmentation_scores(table, background, min_overlap)
    got = metrics.segmentation_scores(_product_table(table), background,
                                      min_overlap)
    for key in INTS:
      assert got[key] == want[key], key
      assert isinstance(got[key], int), key
    for key in FLOATS:
      assert abs(got[key] - want[key]) <= 1e-9 * abs(want[key]), key
    o = got['objects']
    assert o['id'].tolist() == sorted(want['objects'])
    for k, i in enumerate(o['id'].tolist()):
      w = want['objects'][i]
      assert (int(o['size'][k]), int(o['pieces'][k]), int(o['best_segment'][k]),
              int(o['best_overlap'][k])) == (
                  w['size'], w['pieces'], w['best_segment'], w['best_overlap'])
      assert abs(o['best_iou'][k] - w['best_iou']) <= 1e-9 * w['best_iou']
    s = got['segments']
    assert s['id'].tolist() == sorted(want['segments'])
    for k, j in enumerate(s['id'].tolist()):
      w = want['segments'][j]
      assert (int(s['size'][k]), int(s['objects'][k])) == (w['size'],
                                                           w['objects'])


def test_unsorted_table_scores_the_same():
  gt, seg = _random_pair(3)
  table = metrics_ref.contingency(gt, seg)
  perm = np.random.RandomState(0).permutation(len(table[0]))
  a = metrics.segmentation_scores(_product_table(table))
  b = metrics.segmentation_scores(_product_table([t[perm] for t in table]))
  for key in INTS + FLOATS:
    assert a[key] == b[key], key  # bit for bit: summed in sorted order


def test_skeleton_scores_match_specification():
  shape = (16, 24, 24)
  seg = voronoi_labels(shape, 12, 5, dtype=np.uint32)
  nodes, skel, edges = metrics_ref.random_walk_skeletons(shape, 8, 60, 11)
  length = metrics_ref.edge_lengths_q(nodes, edges, (4.0, 1.5, 1.0))
  assert np.array_equal(length, metrics.edge_lengths_q(
      metrics.Skeletons(nodes, skel, edges, (4.0, 1.5, 1.0))))
  for min_nodes in (1, 3):
    r = metrics_ref.skeleton_edges(seg, nodes, skel, edges, length, min_nodes)
    assert r['class_counts'][O] > 0 and r['class_counts'][C] > 0
    num, den, value = metrics_ref.expected_run_length(r)
    s = metrics.skeleton_scores(_product_edges(r))
    assert s['sum_sq_run_lengths'] == num
    assert abs(s['expected_run_length'] - value) <= 1e-9 * value
    total = int(r['class_lengths'].sum())
    for k, name in enumerate(metrics.EDGE_CLASSES):
      assert s['%s_edges' % name] == int(r['class_counts'][k])
      assert abs(s['%s_length_fraction' % name] -
                 int(r['class_lengths'][k]) / total) <= 1e-12


# ---- properties ------------------------------------------------------------------


def test_identical_volumes_score_perfectly():
  gt = voronoi_labels((8, 12, 16), 9, 4)
  r = metrics.segmentation_scores(_product_table(metrics_ref.contingency(gt, gt)))
  assert r['adapted_rand_error'] == 0.0
  assert r['vi_split'] == 0.0 and r['vi_merge'] == 0.0
  assert np.all(r['objects']['best_iou'] == 1.0)
  assert r['n_split_objects'] == r['n_merging_segments'] == 0


def test_one_segment_has_no_split():
  gt = voronoi_labels((8, 12, 16), 9, 4)
  seg = np.full(gt.shape, 7, np.uint32)
  r = metrics.segmentation_scores(_product_table(metrics_ref.contingency(gt, seg)))
  assert r['vi_split'] == 0.0
  assert r['rand_recall'] == 1.0
  assert r['vi_merge'] > 0.0 and r['n_merging_segments'] == 1


def test_swapping_the_volumes_swaps_the_scores():
  a = voronoi_labels((8, 12, 16), 9, 4)
  b = voronoi_labels((8, 12, 16), 13, 5)
  ab = metrics.segmentation_scores(_product_table(metrics_ref.contingency(a, b)))
  ba = metrics.segmentation_scores(_product_table(metrics_ref.contingency(b, a)))
  assert ab['sum_sq_pairs'] == ba['sum_sq_pairs']
  assert ab['sum_sq_gt'] == ba['sum_sq_seg']
  assert ab['rand_precision'] == ba['rand_recall']
  assert ab['rand_recall'] == ba['rand_precision']
  # the entropies are summed in another row order: equal up to rounding
  assert abs(ab['vi_split'] - ba['vi_merge']) <= 1e-12
  assert abs(ab['vi_merge'] - ba['vi_split']) <= 1e-12


# ---- the script ------------------------------------------------------------------


def test_script_scores_two_segmentations(tmp_path, monkeypatch):
  monkeypatch.setattr(metrics, 'default_ops', lambda device_id=0: SpecOps())
  shape = (12, 20, 24)
  gt, seg_a = _random_pair(7, shape)
  _, seg_b = _random_pair(8, shape)
  nodes, skel, edges = metrics_ref.random_walk_skeletons(shape, 5, 40, 3)
  np.save(tmp_path / 'gt.npy', gt)
  np.save(tmp_path / 'a.npy', seg_a)
  np.save(tmp_path / 'b.npy', seg_b)
  np.savez(tmp_path / 'skel.npz', nodes_zyx=nodes, node_skeleton=skel,
           edges=edges, voxel_size_zyx=np.array([2.0, 1.0, 1.0]))
  out = tmp_path / 'scores.json'
  core = ((2, 3, 1), (10, 17, 22))
  evaluate_segmentation.main([
      '--groundtruth', str(tmp_path / 'gt.npy'),
      '--segmentation', 'a:%s' % (tmp_path / 'a.npy'),
      '--segmentation', 'b:%s' % (tmp_path / 'b.npy'),
      '--skeletons', str(tmp_path / 'skel.npz'),
      '--core', '2,3,1:10,17,22', '--background', 'singletons',
      '--merge_min_nodes', '3', '--output', str(out)])
  result = json.loads(out.read_text())
  assert sorted(result) == ['a', 'b']
  for name, seg in (('a', seg_a), ('b', seg_b)):
    assert sorted(result[name]) == ['skeletons', 'voxels']
    v = result[name]['voxels']
    assert 'objects' not in v and 'segments' not in v
    want = metrics_ref.segmentation_scores(
        metrics_ref.contingency(gt, seg, core), 'singletons')
    assert v['n_voxels'] == want['n_voxels'] == int(
        (gt[2:10, 3:17, 1:22] != 0).sum())
    for key in INTS:
      assert v[key] == want[key], key
    for key in FLOATS:
      assert abs(v[key] - want[key]) <= 1e-9 * abs(want[key]), key
    length = metrics_ref.edge_lengths_q(nodes, edges, (2.0, 1.0, 1.0))
    r = metrics_ref.skeleton_edges(seg, nodes, skel, edges, length, 3, core)
    s = result[name]['skeletons']
    assert s['mergers'] == r['mergers']
    assert s['correct_edges'] == int(r['class_counts'][C])
    assert abs(s['expected_run_length'] -
               metrics_ref.expected_run_length(r)[2]) <= 1e-12
  assert result['a']['voxels'] != result['b']['voxels']


def test_script_per_object_and_directory(tmp_path, monkeypatch):
  monkeypatch.setattr(metrics, 'default_ops', lambda device_id=0: SpecOps())
  from ffn_amd.inference import storage
  gt, seg = _random_pair(9)
  calls = []

  def load(path, corner):
    calls.append((path, tuple(corner)))
    return seg.astype(np.uint64), {}

  monkeypatch.setattr(storage, 'load_segmentation', load)
  np.save(tmp_path / 'gt.npy', gt)
  result = evaluate_segmentation.main([
      '--groundtruth', str(tmp_path / 'gt.npy'), '--segmentation',
      'run:%s' % (tmp_path / 'results'), '--corner', '0,8,16', '--per_object'])
  assert calls == [(str(tmp_path / 'results'), (0, 8, 16))]
  v = result['run']['voxels']
  assert sorted(v['objects']) == ['best_iou', 'best_overlap', 'best_segment',
                                  'id', 'pieces', 'size']
  assert len(v['objects']['id']) == v['n_objects']
  json.dumps(result)
  with pytest.raises(ValueError, match='--corner'):
    evaluate_segmentation.main([
        '--groundtruth', str(tmp_path / 'gt.npy'), '--segmentation',
        'run:%s' % (tmp_path / 'results')])
