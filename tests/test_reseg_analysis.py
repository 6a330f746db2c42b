"""Resegmentation analysis without a GPU: the numpy restatement
(tests/reseg_analysis_ref.py) against the reference's own results
(tests/golden/ref_reseg_analysis.npz, minted by
tools/make_golden_reseg_analysis.py), the result messages, and the host
plumbing of ffn_amd/inference/resegmentation_analysis.py with the restatement
as its per-voxel backend."""
import os

import numpy as np
import pytest

from ffn_amd.inference import request as request_lib
from ffn_amd.inference import resegmentation_analysis as analysis_lib
from tests import reseg_analysis_ref as ra

CASES = ra.load_cases()
PAIRS = sorted(n for n, c in CASES.items() if c['kind'] == 'pair')
ENDPOINTS = sorted(n for n, c in CASES.items() if c['kind'] == 'endpoint')


def seg_volume(case):
  return case['seg'][np.newaxis]


def test_fixture_covers_what_it_should():
  assert len(PAIRS) >= 13 and len(ENDPOINTS) >= 6
  assert {'reseg_pair', 'reseg_endpoint'} <= set(CASES)
  raising = {c['want'] for c in CASES.values() if isinstance(c['want'], str)}
  assert raising == {'IncompleteResegmentationError',
                     'InvalidBaseSegmentatonError'}
  good = [CASES[n] for n in PAIRS if not isinstance(CASES[n]['want'], str)]
  assert {tuple(c['voxel_size_zyx']) for c in good} == {(1, 1, 1), (33, 8, 8)}
  assert {c['threshold'] for c in good} == {0.5, 0.6, 0.9}
  assert any(c['radius_zyx'] == c['analysis_radius_zyx'] for c in good)
  assert any(c['radius_zyx'] != c['analysis_radius_zyx'] for c in good)
  assert any(len(c['start_points'][0]) > 1 for c in good)
  assert any(c['want']['from_a_has_deleted_voxels'] == 0 for c in good)
  assert any(c['want']['from_b_deleted_voxels'] > 0 for c in good)
  assert all((c['probs'] == 0).any() for c in good)
  assert os.path.getsize(ra.FIXTURE) < 256 * 1024


@pytest.mark.parametrize('name', PAIRS)
def test_restatement_reproduces_the_reference_pairs(name):
  case = CASES[name]
  got = ra.evaluate_pair(case)
  if isinstance(case['want'], str):
    assert got == case['want']
  else:
    ra.assert_pair_fields(got, case['want'], name)


@pytest.mark.parametrize('name', ENDPOINTS)
def test_restatement_reproduces_the_reference_endpoints(name):
  case = CASES[name]
  got = ra.evaluate_endpoint(case)
  if isinstance(case['want'], str):
    assert got == case['want']
  else:
    ra.assert_endpoint_fields(got, case['want'], name)


def test_object_table_is_numpys_comparison():
  from ffn_amd import analysis
  from ffn_amd.inference import storage
  q = np.arange(256, dtype=np.uint8)
  for threshold in (0.5, 0.6, 0.9, np.float32(0.6), 0.0, 1.0):
    want = np.nan_to_num(storage.dequantize_probability(q)) >= threshold
    table = analysis.object_table(threshold)
    assert table.dtype == np.uint8 and table.shape == (256,)
    assert np.array_equal(table.astype(bool), want)
    assert np.array_equal(table.astype(bool), ra.object_mask(q, threshold))
  assert not analysis.object_table(0.5)[0]  # never visited: not object


# ---- messages -------------------------------------------------------------------

def test_map_field_behaves_like_protobufs():
  m = request_lib.EndpointResegmentationResult()
  assert len(m.overlaps) == 0 and not m.HasField('overlaps')
  assert m.to_text() == ''
  m.overlaps[7].num_overlapping = 4  # created on first access
  m.overlaps[7].num_original = 9
  m.overlaps[2**40].num_original = 1
  m.overlaps[0]  # pylint:disable=pointless-statement
  assert len(m.overlaps) == 3 and sorted(m.overlaps) == [0, 7, 2**40]
  assert [k for k in m.overlaps] == [7, 2**40, 0]
  assert 7 in m.overlaps and 8 not in m.overlaps
  m.source.CopyFrom(m.overlaps[7])
  m.overlaps[7].num_original = 10  # the copy is a copy
  assert m.source.num_original == 9
  with pytest.raises(AttributeError):
    m.overlaps = {}
  text = m.to_text()
  assert text == (
      'overlaps {\n  key: 0\n  value {\n  }\n}\n'
      'overlaps {\n  key: 7\n  value {\n    num_overlapping: 4\n'
      '    num_original: 10\n  }\n}\n'
      'overlaps {\n  key: 1099511627776\n  value {\n    num_original: 1\n  }\n'
      '}\n'
      'source {\n  num_overlapping: 4\n  num_original: 9\n}\n')
  back = request_lib.parse_text(text, request_lib.EndpointResegmentationResult())
  assert back == m and back.to_text() == text
  import copy
  clone = copy.deepcopy(m)
  clone.overlaps[7].num_overlapping = 5
  assert m.overlaps[7].num_overlapping == 4 and clone != m
  # protobuf writes short forms too
  short = request_lib.parse_text(
      'overlaps { key: 3 value { num_original: 2 } } overlaps < key: 4 >',
      request_lib.EndpointResegmentationResult())
  assert short.overlaps[3].num_original == 2 and sorted(short.overlaps) == [3, 4]


def test_result_messages_round_trip_through_text():
  e = request_lib.EndpointResegmentationResult()
  e.id = 2**63 + 5
  e.start.x, e.start.y, e.start.z = 1, 2, 3
  e.num_voxels = 77
  e.segmentation_radius.z = 9
  e.tag = 'run "a"'
  e.overlaps[5].num_overlapping = 1
  blob = e.SerializeToString()
  back = request_lib.EndpointResegmentationResult()
  back.ParseFromString(blob)
  assert back == e and back.id == 2**63 + 5 and back.tag == 'run "a"'

  p = request_lib.PairResegmentationResult()
  p.id_a, p.id_b = 11, 2**40
  p.point.x = 4
  p.eval.radius.y = 3
  p.eval.iou = 0.1
  p.eval.max_edt_a = float('inf')
  p.eval.num_voxels_b = 12
  p.eval.from_a.origin.z = 8
  p.eval.from_a.max_edt = 2.5
  p.eval.from_a.segment_a_consistency = 1 / 3
  p.eval.from_b.deleted_voxels = 0
  assert p.eval.iou == float(np.float32(0.1))  # proto `float` holds f32
  assert p.eval.from_a.segment_a_consistency == float(np.float32(1 / 3))
  assert p.eval.from_b.HasField('deleted_voxels')
  assert not p.eval.from_a.HasField('deleted_voxels')
  back = request_lib.parse_text(p.to_text(),
                                request_lib.PairResegmentationResult())
  assert back == p and back.eval.max_edt_a == float('inf')
  p.eval.iou = float('nan')
  p.eval.from_b.max_edt = float('-inf')
  back = request_lib.parse_text(p.to_text(),
                                request_lib.PairResegmentationResult())
  assert np.isnan(back.eval.iou) and back.eval.from_b.max_edt == float('-inf')
  assert back.to_text() == p.to_text()
  assert request_lib.PairResegmentationResult.SegmentResult is (
      request_lib.SegmentResult)


def test_existing_messages_print_as_before():
  r = request_lib.ResegmentationRequest()
  r.radius.x = 3
  r.inference.image_mean = 128
  r.inference.inference_options.move_threshold = 0.9
  r.points.add().id_a = 5
  assert r.to_text() == (
      'inference {\n  image_mean: 128.0\n  inference_options {\n'
      '    move_threshold: 0.8999999761581421\n  }\n}\n'
      'points {\n  id_a: 5\n}\nradius {\n  x: 3\n}\n')
  o = request_lib.parse_text('move_threshold: 0.5f pad_value: 1e-3',
                             request_lib.InferenceOptions())
  assert o.move_threshold == 0.5 and o.pad_value == float(np.float32(1e-3))


def test_parse_resegmentation_filename():
  parse = analysis_lib.parse_resegmentation_filename
  assert parse('/a/1b/149-135_at_38_39_40.npz') == (149, 135, 38, 39, 40)
  assert parse('135-0_at_1_2_3.npz') == (135, 0, 1, 2, 3)
  assert parse('%d-42_at_7_8_9.npz' % (2**63 + 1)) == (2**63 + 1, 42, 7, 8, 9)
  with pytest.raises(AttributeError):
    parse('seg-1_2_3.npz')


# ---- host plumbing with the numpy backend ----------------------------------------

def call_pair(case, path, **kw):
  return analysis_lib.evaluate_pair_resegmentation(
      path, seg_volume(case), case['radius_zyx'], case['analysis_radius_zyx'],
      case['voxel_size_zyx'], case['threshold'], **kw)


def call_endpoint(case, path, **kw):
  return analysis_lib.evaluate_endpoint_resegmentation(
      path, seg_volume(case), case['radius_zyx'], case['threshold'], **kw)


def check_pair_result(result, case, name):
  assert isinstance(result, request_lib.PairResegmentationResult), (name, result)
  assert (result.id_a, result.id_b) == (case['id_a'], case['id_b'])
  ra.assert_pair_fields(ra.pair_result_fields(result), case['want'], name)


def check_endpoint_result(result, case, name):
  assert isinstance(result, request_lib.EndpointResegmentationResult), (
      name, result)
  ra.assert_endpoint_fields(ra.endpoint_result_fields(result), case['want'],
                            name)


@pytest.mark.parametrize('name', PAIRS)
def test_pair_plumbing_against_the_fixture(name, tmp_path):
  case = CASES[name]
  path = ra.write_case_file(case, tmp_path)
  backend = ra.NumpyAnalyzer()
  if isinstance(case['want'], str):
    with pytest.raises(getattr(analysis_lib, case['want'])):
      call_pair(case, path, analyzer=backend)
    return
  check_pair_result(call_pair(case, path, analyzer=backend), case, name)
  assert backend.pair_batches == [1]


@pytest.mark.parametrize('name', ENDPOINTS)
def test_endpoint_plumbing_against_the_fixture(name, tmp_path):
  case = CASES[name]
  path = ra.write_case_file(case, tmp_path)
  backend = ra.NumpyAnalyzer()
  if isinstance(case['want'], str):
    with pytest.raises(getattr(analysis_lib, case['want'])):
      call_endpoint(case, path, analyzer=backend)
    return
  check_endpoint_result(call_endpoint(case, path, analyzer=backend), case, name)


def test_volume_forms(tmp_path):
  case = CASES['pair00']
  path = ra.write_case_file(case, tmp_path)
  backend = ra.NumpyAnalyzer()
  for volume in (case['seg'][np.newaxis], ra.Volume4d(case['seg'])):
    res = analysis_lib.evaluate_pair_resegmentation(
        path, volume, case['radius_zyx'], case['analysis_radius_zyx'],
        case['voxel_size_zyx'], case['threshold'], analyzer=backend)
    check_pair_result(res, case, 'pair00')
  class SliceOnly:
    """What an h5py dataset offers: a shape and basic indexing."""
    shape = (1,) + case['seg'].shape

    def __getitem__(self, index):
      assert isinstance(index, tuple) and index[0] == 0
      assert all(isinstance(s, slice) for s in index[1:])
      return case['seg'][index[1:]].copy()

  check_pair_result(analysis_lib.evaluate_pair_resegmentation(
      path, SliceOnly(), case['radius_zyx'], case['analysis_radius_zyx'],
      case['voxel_size_zyx'], case['threshold'], analyzer=backend), case,
                    'pair00')


def test_a_box_that_leaves_the_volume_raises_value_error(tmp_path):
  case = CASES['pair00']
  path = ra.write_case_file(case, tmp_path)
  backend = ra.NumpyAnalyzer()
  z, y, x = case['point_zyx']
  small = case['seg'][np.newaxis, :z + 2]
  with pytest.raises(ValueError):
    analysis_lib.evaluate_pair_resegmentation(
        path, small, case['radius_zyx'], case['analysis_radius_zyx'],
        case['voxel_size_zyx'], case['threshold'], analyzer=backend)
  shifted = case['seg'][np.newaxis, :, :, x - 1:]  # x - radius < 0
  with pytest.raises(ValueError):
    analysis_lib.evaluate_endpoint_resegmentation(
        path, shifted, case['radius_zyx'], analyzer=backend)
  bigger = [r + 1 for r in case['radius_zyx']]
  with pytest.raises(ValueError):  # analysis box larger than the object maps
    analysis_lib.evaluate_pair_resegmentation(
        path, np.zeros((1, 99, 99, 99), np.uint64), case['radius_zyx'], bigger,
        (1, 1, 1), analyzer=backend)
  assert not backend.pair_batches and not backend.endpoint_batches


def test_reference_surface_on_masks():
  """compute_iou and evaluate_segmentation_result take the reference's
  arguments (boolean masks)."""
  rng = np.random.default_rng(5)
  backend = ra.NumpyAnalyzer()
  reseg = rng.random((2, 9, 10, 11)) < 0.4
  want = (reseg[0] & reseg[1]).sum() / float(reseg.max(axis=0).sum())
  assert analysis_lib.compute_iou(reseg, analyzer=backend) == want
  assert np.isnan(analysis_lib.compute_iou(np.zeros((2, 3, 3, 3), bool),
                                           analyzer=backend))
  seg1 = rng.random((9, 10, 11)) < 0.3
  seg2 = seg1 ^ (rng.random((9, 10, 11)) < 0.2)  # overlaps seg1
  moves = np.array([[2, 2, 2], [0, 5, 5], [8, 8, 8], [9, 8, 8]])
  dels = np.array([1, 10, 100, 1000])
  from scipy import ndimage
  for sampling in ((1, 1, 1), (33, 8, 8)):
    res = request_lib.SegmentResult()
    analysis_lib.evaluate_segmentation_result(
        reseg[0], dels, moves, (2, 2, 2), (3, 3, 3), seg1, seg2, sampling, res,
        analyzer=backend)
    assert res.num_voxels == reseg[0].sum()
    assert res.deleted_voxels == 101  # [2, 8] on every axis, ends included
    assert res.max_edt == np.float32(ndimage.distance_transform_edt(
        reseg[0], sampling=sampling).max())
    assert res.segment_a_consistency == np.float32(
        reseg[0][seg1].sum() / seg1.sum())
    assert res.segment_b_consistency == np.float32(
        reseg[0][seg2].sum() / seg2.sum())
  res = request_lib.SegmentResult()
  analysis_lib.evaluate_segmentation_result(
      reseg[0], np.zeros(0), np.zeros((0, 3)), (2, 2, 2), (3, 3, 3), seg1, seg2,
      (1, 1, 1), res, analyzer=backend)
  assert not res.HasField('deleted_voxels')


def shared_volume_cases(tmp_path):
  """The two ref_reseg.npz points (one volume) and their files, plus a pair
  file that is incomplete and one whose segments are absent."""
  pair, end = CASES['reseg_pair'], CASES['reseg_endpoint']
  names = [ra.write_case_file(pair, tmp_path), ra.write_case_file(end, tmp_path)]
  incomplete = dict(pair, id_a=7, id_b=8, probs=pair['probs'][:1])
  absent = dict(pair, id_a=5, id_b=6)
  names.append(ra.write_case_file(incomplete, tmp_path))
  names.append(ra.write_case_file(absent, tmp_path))
  return pair, end, names


def test_evaluate_pairs_returns_exceptions_in_place(tmp_path):
  pair, _, names = shared_volume_cases(tmp_path)
  files = [names[2], names[0], str(tmp_path / '1-2_at_3_4_5.npz'), names[3],
           names[0]]
  for batch, want_batches in ((None, [3]), (2, [1, 1, 1]), (1, [1, 1, 1])):
    backend = ra.NumpyAnalyzer()
    got = analysis_lib.evaluate_pairs(
        files, seg_volume(pair), pair['radius_zyx'],
        pair['analysis_radius_zyx'], pair['voxel_size_zyx'], pair['threshold'],
        batch=batch, analyzer=backend)
    assert len(got) == 5
    assert isinstance(got[0], analysis_lib.IncompleteResegmentationError)
    assert isinstance(got[2], FileNotFoundError)
    assert isinstance(got[3], analysis_lib.InvalidBaseSegmentatonError)
    check_pair_result(got[1], pair, 'reseg_pair')
    check_pair_result(got[4], pair, 'reseg_pair')
    # files that fail before the device call are not part of a batch
    assert backend.pair_batches == want_batches, batch


def test_evaluate_request_keeps_point_order(tmp_path):
  pair, end, _ = shared_volume_cases(tmp_path)
  request = request_lib.ResegmentationRequest()
  request.output_directory = str(tmp_path)
  request.radius.x = request.radius.y = request.radius.z = 24
  request.analysis_radius.x = request.analysis_radius.y = 8
  request.analysis_radius.z = 8
  z, y, x = pair['point_zyx']

  def add(id_a, id_b=None, dx=0):
    p = request.points.add()
    p.id_a = id_a
    if id_b is not None:
      p.id_b = id_b
    p.point.z, p.point.y, p.point.x = z, y, x + dx
  add(end['id_a'])                       # endpoint
  add(pair['id_a'], pair['id_b'])        # pair
  add(pair['id_a'], pair['id_b'], dx=1)  # never written
  add(7, 8)                              # incomplete
  add(end['id_a'])                       # endpoint again
  before = sorted(os.listdir(str(tmp_path)))
  backend = ra.NumpyAnalyzer()
  got = analysis_lib.evaluate_request(request, seg_volume(pair),
                                      pair['voxel_size_zyx'],
                                      threshold=pair['threshold'],
                                      analyzer=backend)
  assert sorted(os.listdir(str(tmp_path))) == before  # nothing created
  assert len(got) == 5
  check_pair_result(got[1], pair, 'reseg_pair')
  assert isinstance(got[2], FileNotFoundError)
  assert isinstance(got[3], analysis_lib.IncompleteResegmentationError)
  assert backend.pair_batches == [1] and backend.endpoint_batches == [2]
  # the endpoint fixture was minted at threshold 0.5: the default
  got = analysis_lib.evaluate_request(request, seg_volume(pair), (1, 1, 1),
                                      analyzer=backend)
  for k in (0, 4):
    check_endpoint_result(got[k], end, 'reseg_endpoint')
  # without analysis_radius the whole box is analysed
  request.ClearField('analysis_radius')
  whole = analysis_lib.evaluate_request(request, seg_volume(pair), (1, 1, 1),
                                        threshold=0.6, analyzer=backend)[1]
  assert [whole.eval.radius.x, whole.eval.radius.y, whole.eval.radius.z] == [24] * 3
  # subdirectories as resegmentation.get_target_path names them
  import hashlib
  request.subdir_digits = 2
  sub = hashlib.md5(b'%d%d' % (pair['id_a'], pair['id_b'])).hexdigest()[:2]
  assert analysis_lib.result_path(request, 1) == os.path.join(
      str(tmp_path), sub, ra.file_name(pair))
  assert not os.path.exists(os.path.join(str(tmp_path), sub))
