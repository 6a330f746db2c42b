"""Decision points without a GPU: the numpy restatement (tests/decision_ref.py)
against the reference's own find_decision_points
(tests/golden/ref_decision_points.npz, minted by
tools/make_golden_decision_points.py), against brute force and scipy, and the
host half of the product (select_points, to_resegmentation_points)."""
import os

import numpy as np
import pytest

from tests import decision_ref

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden',
                      'ref_decision_points.npz')


def load_cases():
  g = np.load(GOLDEN)
  cases = {}
  for name in g['cases']:
    name = str(name)
    maxd = float(g[name + '_max_distance'])
    subvol = g[name + '_subvol']
    cases[name] = dict(
        seg=g[name + '_seg'], voxel_size=tuple(g[name + '_voxel_size']),
        max_distance=None if np.isnan(maxd) else maxd,
        subvol=None if not len(subvol) else (tuple(subvol[0]), tuple(subvol[1])),
        sparse=bool(g[name + '_sparse'][0]), noise=int(g[name + '_sparse'][1]),
        pairs=g[name + '_pairs'], dist=g[name + '_dist'],
        points=g[name + '_points'],
        cands={k: g['%s_cand_%s' % (name, k)]
               for k in ('a', 'b', 'dist', 'off', 'z', 'y', 'x')})
  return cases


CASES = load_cases() if os.path.exists(GOLDEN) else {}


def subvol_slices(subvol):
  if subvol is None:
    return None
  start, size = subvol
  return tuple(slice(int(s), int(s) + int(n))
               for s, n in zip(start[::-1], size[::-1]))


def assert_matches_fixture(got, case):
  """`got` is exactly the reference's dict: keys, distance bits, points."""
  keys = [tuple(int(v) for v in p) for p in case['pairs']]
  assert sorted(got) == keys
  for k, d, p in zip(keys, case['dist'], case['points']):
    assert np.float64(got[k][0]).tobytes() == np.float64(d).tobytes(), k
    assert np.array_equal(got[k][1], p), k


def small_volume():
  """<= 30^3, blocky with gaps, non-contiguous ids."""
  return decision_ref.synthetic_segmentation((11, 14, 16), seed=21, gap=2,
                                             drop=0.3)


def test_fixture_has_the_cases_the_specification_names():
  assert set(CASES) >= {'iso', 'iso_max', 'aniso', 'aniso_max', 'subvol',
                        'big_ids', 'sparse_one', 'sparse_dust'}
  assert CASES['big_ids']['seg'].max() > 2**32
  assert any(n % 64 for n in CASES['iso']['seg'].shape)
  assert len(CASES['sparse_one']['pairs']) == 0
  assert all(len(CASES[c]['pairs']) > 10 for c in CASES if c != 'sparse_one')


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_the_reference(name):
  case = CASES[name]
  seg = case['seg'].copy()
  if case['sparse']:
    ids, counts = np.unique(seg, return_counts=True)
    if case['noise']:
      seg[np.isin(seg, ids[counts < case['noise']])] = 0
    if len(np.unique(seg[seg > 0])) <= 1:
      assert len(case['pairs']) == 0
      return
  got = decision_ref.decision_points_spec(
      seg, case['voxel_size'], case['max_distance'],
      subvol_slices(case['subvol']))
  assert_matches_fixture(got, case)


@pytest.mark.parametrize('voxel_size', [(1, 1, 1), (8, 8, 33), (3, 2, 5)])
def test_expand_spec_against_brute_force(voxel_size):
  seg = small_volume()
  expanded, edt = decision_ref.expand_spec(seg, voxel_size)
  want_edt, _, tied = decision_ref.brute_force_expand(seg, voxel_size)
  assert edt.tobytes() == want_edt.tobytes()
  assert np.any(seg == 0) and np.any(seg > 0)
  n_tied = 0
  for v in np.ndindex(*seg.shape):
    assert expanded[v] == tied[v][0], v
    n_tied += len(tied[v]) > 1
  assert n_tied > 0  # the tie rule was exercised
  assert np.array_equal(expanded[seg > 0], seg[seg > 0])


@pytest.mark.parametrize('axis', [1, 0])
def test_expand_spec_keeps_a_parabola_that_only_touches(axis):
  seg, centre = decision_ref.touching_parabola_volume(axis)
  expanded, edt = decision_ref.expand_spec(seg, (1, 1, 1))
  _, _, tied = decision_ref.brute_force_expand(seg, (1, 1, 1))
  assert tied[centre] == [3, 5, 7, 9]
  assert expanded[centre] == 3 and edt[centre] == 2.0
  for v in np.ndindex(*seg.shape):
    assert expanded[v] == tied[v][0], v


def test_expand_spec_float_path_equals_packed_path():
  seg = small_volume()
  a = decision_ref.expand_spec(seg, (8, 8, 33), 40.0)
  d2 = np.where(seg > 0, 0.0, np.inf)
  values, inverse = np.unique(seg, return_inverse=True)
  ids = inverse.reshape(seg.shape).astype(np.int64)
  for axis, w in ((2, 8.0), (1, 8.0), (0, 33.0)):
    d2, ids = decision_ref._pass_float(d2, ids, axis, w)  # pylint:disable=protected-access
  edt = np.sqrt(d2)
  expanded = values[ids]
  expanded[edt > 40.0] = 0
  assert np.array_equal(a[0], expanded) and a[1].tobytes() == edt.tobytes()


def test_expand_spec_degenerate_volumes():
  full = np.full((3, 4, 5), 9, np.uint64)
  expanded, edt = decision_ref.expand_spec(full, (8, 8, 33))
  assert np.array_equal(expanded, full) and not edt.any()
  empty = np.zeros((3, 4, 5), np.uint32)
  expanded, edt = decision_ref.expand_spec(empty, (1, 1, 1), 40.0)
  assert not expanded.any() and np.all(np.isinf(edt))


def test_edt_equals_scipy_and_scipy_label_is_among_the_tied():
  ndimage = pytest.importorskip('scipy.ndimage')
  for name, sampling in (('iso', (1, 1, 1)), ('aniso', (33, 8, 8))):
    seg = CASES[name]['seg']
    _, edt = decision_ref.expand_spec(seg, sampling[::-1])
    want = ndimage.distance_transform_edt(seg == 0, sampling=sampling)
    assert edt.tobytes() == want.tobytes()
  seg = small_volume()
  for sampling in ((1, 1, 1), (33, 8, 8)):
    _, idx = ndimage.distance_transform_edt(seg == 0, sampling=sampling,
                                            return_indices=True)
    label = seg[tuple(idx)]
    _, _, tied = decision_ref.brute_force_expand(seg, sampling[::-1])
    for v in np.ndindex(*seg.shape):
      assert int(label[v]) in tied[v], v


@pytest.mark.parametrize('name', sorted(CASES))
def test_select_points_on_fixture_candidates(name):
  from ffn_amd.utils import decision_point
  case = CASES[name]
  rng = np.random.RandomState(5)
  perm = rng.permutation(len(case['cands']['a']))  # a device returns any order
  shuffled = {k: v[perm] for k, v in case['cands'].items()}
  assert_matches_fixture(decision_point.select_points(shuffled), case)


def test_select_points_takes_the_first_of_equally_central_candidates():
  from ffn_amd.utils import decision_point
  c = {'a': np.array([4, 4, 4, 4], np.uint64), 'b': np.array([9] * 4, np.uint64),
       'dist': np.full(4, 1.5), 'off': np.array([1, 0, 0, 1], np.int32),
       'z': np.zeros(4, np.int32), 'y': np.array([0, 2, 0, 2], np.int32),
       'x': np.array([2, 0, 0, 2], np.int32)}
  # mean (1, 1, 0); all four are equally far; row order puts (off 0, y 0) first
  got = decision_point.select_points(c)
  assert list(got) == [(4, 9)]
  assert got[(4, 9)][0] == 1.5 and got[(4, 9)][1].tolist() == [0, 0, 0]
  assert decision_point.select_points({k: v[:0] for k, v in c.items()}) == {}


def test_to_resegmentation_points_round_trips_through_text():
  from ffn_amd.inference import request as request_lib
  from ffn_amd.utils import decision_point
  case = CASES['subvol']
  points = decision_point.select_points(case['cands'])
  request = request_lib.ResegmentationRequest()
  request.radius.x = request.radius.y = request.radius.z = 24
  request.output_directory = '/tmp/out'
  decision_point.to_resegmentation_points(points, request, case['subvol'])
  assert len(request.points) == len(points) > 10
  origin = np.array(case['subvol'][0])
  for p, key in zip(request.points, sorted(points)):
    assert (p.id_a, p.id_b) == key and p.id_a < p.id_b
    assert [p.point.x, p.point.y, p.point.z] == (points[key][1] + origin).tolist()
    # the point lies in the volume, next to both segments' expansions
    assert all(0 <= v < n for v, n in zip(
        (p.point.z, p.point.y, p.point.x), case['seg'].shape))
  parsed = request_lib.parse_text(request.to_text(),
                                  request_lib.ResegmentationRequest())
  assert parsed == request
  assert [(p.id_a, p.id_b) for p in parsed.points] == sorted(points)


def test_crop_accepts_boxes_and_tuples():
  from ffn_amd.inference import request as request_lib  # noqa: F401
  from ffn_amd.utils import decision_point

  class Box:
    def to_slice3d(self):
      return np.index_exp[3:34, 7:36, 5:42]

  crop = decision_point._crop  # pylint:disable=protected-access
  assert crop(Box(), (40, 48, 56)) == ([3, 7, 5], [34, 36, 42])
  assert crop(((5, 7, 3), (37, 29, 31)), (40, 48, 56)) == ([3, 7, 5],
                                                            [34, 36, 42])
  assert crop(((5, 7, 3), (37, 29, 100)), (40, 48, 56)) == ([3, 7, 5],
                                                             [40, 36, 42])
  assert crop(None, (1, 2, 3)) is None


class EmulatedDecisionOps:
  """DecisionOps whose two stages are the specification (no GPU): what the
  host side of find_decision_points sees of a device."""

  def __init__(self):
    import threading
    self.lock = threading.Lock()
    self.shape = None

  def expand(self, seg, voxel_size, max_distance=None):
    self._state = decision_ref.expand_spec(seg, voxel_size, max_distance)
    self.shape = tuple(seg.shape)

  def contact_minima(self, sub_box=None):
    expanded, edt = self._state
    if sub_box is not None:
      sl = tuple(slice(l, h) for l, h in zip(*sub_box))
      expanded, edt = expanded[sl], edt[sl]
    c = decision_ref.minimising_spec(decision_ref.candidates_spec(expanded, edt))
    perm = np.random.RandomState(9).permutation(len(c['a']))
    return {k: v[perm] for k, v in c.items()}


@pytest.mark.parametrize('name', ['iso', 'aniso_max', 'subvol', 'big_ids'])
def test_find_decision_points_over_an_emulated_device(name, monkeypatch):
  from ffn_amd import decision
  from ffn_amd.utils import decision_point
  monkeypatch.setattr(decision, 'default_ops',
                      lambda device_id=0: EmulatedDecisionOps())
  case = CASES[name]
  got = decision_point.find_decision_points(
      case['seg'], case['voxel_size'], max_distance=case['max_distance'],
      subvol_box=case['subvol'])
  assert_matches_fixture(got, case)
