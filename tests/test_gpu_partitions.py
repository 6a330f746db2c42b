"""Partition maps on the GPU (include/ffn_partitions.h, ffn_amd/partitions.py,
compute_partitions.py) against the reference's own results
(tests/golden/ref_partitions.npz) and the numpy specification
(tests/partitions_ref.py): partitions and raw counts, byte for byte."""
import numpy as np
import pytest

from tests import partitions_ref
from tests.test_partitions import CASES, SAMPLE12, case_args

pytestmark = pytest.mark.gpu

#: output tile of lom_count_kernel (z, y, x) while its LDS stays below 78 KiB;
#: beyond that (e.g. rz = ry = 20) the tile is (8, 4, 64)
TILE = (8, 8, 64)


@pytest.fixture(scope='module')
def ops():
  from ffn_amd import partitions
  return partitions.default_ops(0)


def random_volume(out_shape, radius_zyx, seed, n_labels=9, hole_fraction=0.08):
  """Voronoi cells with holes whose valid region has `out_shape`."""
  shape = tuple(o + 2 * r for o, r in zip(out_shape, radius_zyx))
  seg = partitions_ref.voronoi_labels(shape, n_labels, seed, dtype=np.uint32,
                                      id_base=3, id_step=5)
  seg[np.random.RandomState(seed + 50).rand(*shape) < hole_fraction] = 0
  return seg


def check_against_spec(ops, seg, thresholds, lom_radius, counts_fn=None, **kw):
  got, counts = ops.compute(seg, thresholds, lom_radius, return_counts=True,
                            **kw)
  if counts_fn is None:
    want, want_counts = partitions_ref.partitions_spec(seg, thresholds,
                                                       lom_radius, **kw)
  else:  # boxes too large to enumerate
    assert set(kw) <= {'min_size'}
    radius = tuple(lom_radius)[::-1]
    work = partitions_ref.background_cleared(seg, None,
                                             kw.get('min_size', 10000))
    want_counts = counts_fn(work, radius)
    fov = int(np.prod([2 * r + 1 for r in radius]))
    want = partitions_ref.class_table_fast(thresholds, fov)[want_counts]
    want[want_counts == 0] = 0
  assert got.dtype == np.uint8 and counts.dtype == np.uint32
  assert got.shape == want.shape and counts.shape == want.shape
  assert counts.tobytes() == want_counts.tobytes()
  assert got.tobytes() == want.tobytes()
  assert np.array_equal(ops.partition_counts(),
                        np.array(np.unique(got, return_counts=True)))
  return got, counts


@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture_cases(ops, name):
  case = CASES[name]
  before = case['seg'].copy()
  got, counts = ops.compute(case['seg'], mask=case['mask'], return_counts=True,
                            **case_args(case))
  assert got.dtype == np.uint8 and counts.dtype == np.uint32
  assert got.shape == case['partitions'].shape
  assert counts.tobytes() == case['counts'].tobytes()
  assert got.tobytes() == case['partitions'].tobytes()
  assert np.array_equal(case['seg'], before)
  assert np.array_equal(ops.partition_counts(),
                        np.array(np.unique(got, return_counts=True)))


@pytest.mark.parametrize('out_shape', [
    tuple(t - 1 for t in TILE), TILE, tuple(t + 1 for t in TILE),
    (TILE[0] + 1, TILE[1] - 1, TILE[2]), (2 * TILE[0] + 3, 1, 2 * TILE[2] + 5),
    (1, 2 * TILE[1] + 1, TILE[2] - 1),
])
def test_random_volumes_around_the_tile(ops, out_shape):
  radius = (1, 2, 3)  # zyx
  seg = random_volume(out_shape, radius, seed=sum(out_shape))
  check_against_spec(ops, seg, SAMPLE12, radius[::-1], min_size=1)


@pytest.mark.parametrize('out_shape,radius', [
    # rz = ry = 20: the (8, 4, 64) tile, one below / at / above it
    ((7, 3, 63), (20, 20, 1)), ((8, 4, 64), (20, 20, 1)),
    ((9, 5, 65), (20, 20, 1)),
    # more than 64 KiB of dynamic LDS; the radius limit on every axis
    ((9, 5, 3), (32, 32, 2)), ((2, 3, 66), (32, 32, 32)),
])
def test_large_radii_take_the_smaller_tile(ops, out_shape, radius):
  seg = random_volume(out_shape, radius, seed=sum(out_shape) + radius[2],
                      n_labels=12, hole_fraction=0.02)
  check_against_spec(ops, seg, SAMPLE12, radius[::-1],
                     counts_fn=partitions_ref.table_counts, min_size=1)


def test_input_dtypes_give_the_same_result(ops):
  seg = random_volume((9, 9, 70), (1, 1, 2), seed=11, n_labels=20)
  ranks = np.unique(seg, return_inverse=True)[1].reshape(seg.shape)
  assert 8 < ranks.max() < 128
  results = []
  for dtype in (np.uint8, np.uint32, np.int32, np.uint64, np.int64):
    got = ops.compute(ranks.astype(dtype), SAMPLE12, (2, 1, 1), min_size=50,
                      return_counts=True)
    results.append(got)
  want = partitions_ref.partitions_spec(ranks, SAMPLE12, (2, 1, 1),
                                        min_size=50)
  for got in results:
    assert got[0].tobytes() == want[0].tobytes()
    assert got[1].tobytes() == want[1].tobytes()


def test_whitelist_spheres_and_mask_together(ops):
  radius = (2, 1, 2)
  seg = random_volume((10, 9, 66), radius, seed=23, n_labels=14)
  ids = np.unique(seg[seg > 0])
  mask = np.zeros(seg.shape, bool)
  mask[0, 0, 0] = mask[7, 5, 40] = mask[-1, -1, -1] = True
  got, _ = check_against_spec(
      ops, seg, [0.5, 0.2, 0.9], radius[::-1], min_size=30,
      id_whitelist=[int(i) for i in ids[1::2]] + [12345],
      exclusion_regions=[(20, 5, 6, 3.5), (69, 10, 13, 4), (-3.0, 2.0, 2.0, 6)],
      mask=mask)
  assert (got == 255).any() and (got == 0).any() and ((got > 0) &
                                                      (got < 255)).any()


@pytest.mark.parametrize('min_size', [0, -5])
def test_min_size_not_positive_removes_nothing(ops, min_size):
  seg = np.zeros((6, 7, 8), np.uint32)
  seg[2, 3, 4] = 9  # a single voxel
  seg[3:, :, :] = 4
  got, counts = check_against_spec(ops, seg, [0.5], (1, 1, 1),
                                   min_size=min_size)
  assert counts[1, 2, 3] == 1 and got[1, 2, 3] == 1
  dusted = ops.compute(seg, [0.5], (1, 1, 1), min_size=2)
  assert dusted[1, 2, 3] == 0


def test_axis_shorter_than_the_diameter_gives_an_empty_output():
  from ffn_amd import partitions

  class NoDevice:
    def __getattr__(self, name):
      raise AssertionError('device call: ' + name)

  fresh = partitions.PartitionOps(0)
  lib, fresh._lib = fresh._lib, NoDevice()
  try:
    seg = np.ones((4, 9, 9), np.uint32)
    got, counts = fresh.compute(seg, [0.5], (1, 1, 2), return_counts=True)
    assert got.shape == counts.shape == (0, 7, 7)
    assert got.dtype == np.uint8 and counts.dtype == np.uint32
    assert fresh.compute(seg, [0.5], (5, 1, 2)).shape == (0, 7, 0)
    assert fresh.partition_counts().shape == (2, 0)
  finally:
    fresh._lib = lib
    fresh.close()


def test_handle_closes_twice_and_the_default_is_one_object():
  from ffn_amd import _lib
  from ffn_amd import partitions
  assert partitions.default_ops(0) is partitions.default_ops(0)
  obj = partitions.PartitionOps(0)
  assert obj.device_id == 0 and obj._h
  obj.close()
  assert not obj._h
  obj.close()
  with pytest.raises(_lib.FFNHipError):
    obj.compute(np.ones((4, 4, 4), np.uint32), [0.5], (1, 1, 1))


def test_two_handles_on_one_device_share_the_kernel(ops):
  """The dynamic LDS limit is the kernel's, per device, not a handle's: a
  second handle at a small radius must not take the first one's large-radius
  launch away, nor the other way round."""
  from ffn_amd import partitions
  small = random_volume((5, 5, 5), (1, 1, 1), seed=31)
  wide = random_volume((3, 2, 5), (32, 32, 2), seed=32, n_labels=12,
                       hole_fraction=0.02)
  other = partitions.PartitionOps(0)
  try:
    for handle in (ops, other, ops):
      check_against_spec(handle, wide, SAMPLE12, (2, 32, 32),
                         counts_fn=partitions_ref.table_counts, min_size=1)
      check_against_spec(other, small, SAMPLE12, (1, 1, 1), min_size=1)
  finally:
    other.close()


def test_results_do_not_depend_on_what_ran_before(ops):
  """Buffers grow and are reused: a small volume after a large one."""
  small = random_volume((5, 5, 5), (1, 1, 1), seed=3)
  first = ops.compute(small, SAMPLE12, (1, 1, 1), min_size=1)
  large = random_volume((9, 9, 130), (1, 1, 1), seed=4, n_labels=30)
  check_against_spec(ops, large, SAMPLE12, (1, 1, 1), min_size=1)
  again = ops.compute(small, SAMPLE12, (1, 1, 1), min_size=1)
  assert first.tobytes() == again.tobytes()
  (_, _), (ms, nbytes) = ops.last_timing()
  assert ms > 0 and nbytes == small.size * 4 + again.size


@pytest.mark.parametrize('dtype', [np.uint64, np.uint32])
def test_more_ids_than_the_first_table(dtype):
  """label_sizes with more distinct ids than the 2^18 slots the id table starts
  with (it has to grow), long runs and one large count; then a small volume on
  the same handle, which finds the grown table."""
  from ffn_amd import partitions
  rng = np.random.default_rng(70)
  ids = rng.permutation(70**3).astype(np.uint64)
  ids = ids * 2**33 + 5 if dtype == np.uint64 else ids + 1
  seg = ids.astype(dtype).reshape(70, 70, 70)
  seg[:4] = 9
  want_ids, want_sizes = np.unique(seg, return_counts=True)
  assert want_ids.size > 1 << 18
  case = CASES[sorted(CASES)[0]]
  fresh = partitions.PartitionOps(0)  # a table no earlier test has grown
  try:
    got_ids, got_sizes = fresh.label_sizes(seg)
    order = np.argsort(got_ids)
    assert np.array_equal(got_ids[order], want_ids.astype(np.uint64))
    assert np.array_equal(got_sizes[order], want_sizes.astype(np.uint64))
    got_ids, got_sizes = fresh.label_sizes(case['seg'])
    order = np.argsort(got_ids)
    want_ids, want_sizes = np.unique(case['seg'], return_counts=True)
    assert np.array_equal(got_ids[order], want_ids.astype(np.uint64))
    assert np.array_equal(got_sizes[order], want_sizes.astype(np.uint64))
    got = fresh.compute(case['seg'], mask=case['mask'], **case_args(case))
    assert got.tobytes() == case['partitions'].tobytes()
  finally:
    fresh.close()


def test_cli_end_to_end(tmp_path):
  import compute_partitions as root
  case = CASES['excl']
  src, dst = str(tmp_path / 'seg.npy'), str(tmp_path / 'af.npz')
  np.save(src, case['seg'])
  root.main(['--input_volume', src, '--output_volume', dst,
             '--thresholds', ','.join(repr(t) for t in case['thresholds']),
             '--lom_radius', ','.join(str(r) for r in case['lom_radius']),
             '--exclusion_regions',
             ','.join(repr(v) for r in case['exclusion_regions'] for v in r),
             '--min_size', str(case['min_size'])])
  rx, ry, rz = case['lom_radius']
  with np.load(dst) as out:
    full, counts = out['partitions'], out['partition_counts']
  assert full.shape == case['seg'].shape
  assert np.array_equal(full[rz:-rz, ry:-ry, rx:-rx], case['partitions'])
  assert np.array_equal(counts, np.array(np.unique(case['partitions'],
                                                   return_counts=True)))
