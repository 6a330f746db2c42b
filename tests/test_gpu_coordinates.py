"""Balanced training coordinates on the GPU (include/ffn_coordinates.h,
ffn_amd/coordinates.py, build_coordinates.py) against the reference's recorded
sequences (tests/golden/ref_coordinates.npz) and the numpy restatement with its
Python TFRecord encoder (tests/coordinates_ref.py)."""
import gzip

import numpy as np
import pytest

from tests import coordinates_ref
from tests import partitions_ref
from tests.test_coordinates import CASES

pytestmark = pytest.mark.gpu

#: voxels per wave segment and per workgroup chunk of the counting sort while a
#: crop has at most 4096 segments (csrc/ffn_coordinates.hip)
SEGMENT = 1024
CHUNK = 4 * SEGMENT


@pytest.fixture(scope='module')
def ops():
  from ffn_amd import coordinates
  return coordinates.default_ops(0)


def runs(shape, seed, values, mean_run=40):
  """Long runs of the given values in C order, as a partition map has them."""
  rng = np.random.RandomState(seed)
  n = int(np.prod(shape))
  lengths = rng.randint(1, 2 * mean_run, size=3 * (n // mean_run) + 64)
  picks = rng.choice(np.asarray(values, np.uint8), size=len(lengths))
  flat = np.repeat(picks, lengths)
  assert len(flat) >= n
  return flat[:n].reshape(shape)


def flat_crop(n, seed):
  return runs((1, 1, n), seed, [0, 1, 2, 7, 255], mean_run=90)


SORT_CASES = {
    'smaller_than_a_wave': lambda: runs((3, 5, 7), 1, [0, 3, 255], mean_run=9),
    'one_wave_exactly': lambda: runs((1, 1, 64), 2, [1, 2], mean_run=5),
    'segment_minus_1': lambda: flat_crop(SEGMENT - 1, 3),
    'segment': lambda: flat_crop(SEGMENT, 4),
    'segment_plus_1': lambda: flat_crop(SEGMENT + 1, 5),
    'chunk_minus_1': lambda: flat_crop(CHUNK - 1, 6),
    'chunk': lambda: flat_crop(CHUNK, 7),
    'chunk_plus_1': lambda: flat_crop(CHUNK + 1, 8),
    'rows_end_mid_chunk': lambda: runs((20, 33, 70), 9, [0, 1, 2, 3, 4, 255]),
    'several_blocks': lambda: runs((70, 69, 71), 10, [0, 1, 2, 5, 9, 12, 255],
                                   mean_run=300),
    # more than 4096 segments of 1024: the segments grow, and end mid-wave
    'longer_segments': lambda: runs((164, 161, 163), 11, [0, 1, 4, 255],
                                    mean_run=2000),
    'every_value': lambda: np.random.RandomState(12).permutation(
        np.arange(256 * 41, dtype=np.int64) % 256).astype(np.uint8).reshape(
            8, 41, 32),
    'single_class': lambda: np.full((9, 10, 77), 6, np.uint8),
    'all_ignored': lambda: np.full((5, 6, 70), 255, np.uint8),
    'changes_every_voxel': lambda: (np.arange(11 * 13 * 67) % 2 * 3).astype(
        np.uint8).reshape(11, 13, 67),
    'changes_every_voxel_3': lambda: (np.arange(5000) % 3 * 100).astype(
        np.uint8).reshape(1, 1, 5000),
}


@pytest.mark.parametrize('name', sorted(SORT_CASES))
def test_sort_gives_flatnonzero_per_class(ops, name):
  crop = SORT_CASES[name]()
  assert crop.dtype == np.uint8 and crop.ndim == 3
  values, want_counts = np.unique(crop, return_counts=True)
  want = {int(c): np.flatnonzero(crop == c).astype(np.uint32) for c in values}
  before = crop.copy()
  results = []
  for _ in range(2):  # run-to-run identity
    ops.reset()
    # (another volume first: the lists are per volume)
    ops.add_volume(np.full((2, 3, 4), 1, np.uint8))
    counts = ops.add_volume(crop)
    assert counts.dtype == np.uint64 and counts.shape == (256,)
    assert np.array_equal(np.flatnonzero(counts), values)
    assert np.array_equal(counts[values], want_counts)
    got = {c: ops.class_list(1, c) for c in range(255)}
    for c in range(255):
      assert got[c].dtype == np.uint32
      assert got[c].tobytes() == want.get(c, np.zeros(0, np.uint32)).tobytes()
    results.append(b''.join(got[c].tobytes() for c in range(255)))
    assert ops.class_list(0, 1).tolist() == list(range(24))
  assert results[0] == results[1]
  assert np.array_equal(crop, before)
  (ms, nbytes), _, _ = ops.last_timing()
  assert ms > 0 and nbytes == 2 * crop.size + 4 * int((crop != 255).sum())


@pytest.mark.parametrize('name', sorted(CASES))
def test_fixture_cases(ops, name):
  case = CASES[name]
  before = [v.copy() for _, v in case['volumes']]
  centers, volume, totals = ops.build(case['volumes'], case['margin'],
                                      np.random.RandomState(case['seed']))
  assert centers.dtype == np.int32 and volume.dtype == np.int32
  assert centers.shape == case['centers'].shape
  assert np.array_equal(centers, case['centers'])
  assert np.array_equal(volume, case['volume'])
  assert list(totals.items()) == list(case['totals'].items())
  assert all(np.array_equal(v, b)
             for (_, v), b in zip(case['volumes'], before))


def test_build_draws_from_the_global_generator_by_default(ops):
  case = CASES['three']
  np.random.seed(case['seed'])
  centers, volume, _ = ops.build(case['volumes'], case['margin'])
  assert np.array_equal(centers, case['centers'])
  assert np.array_equal(volume, case['volume'])


def test_margin_zero_means_no_crop(ops):
  vol = runs((6, 9, 35), 21, [0, 2, 255], mean_run=12)
  got = ops.build([('v', vol)], (0, 1, 0), np.random.RandomState(3))
  want = coordinates_ref.coordinates_spec([('v', vol)], (0, 1, 0),
                                          np.random.RandomState(3))
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
  assert got[2] == want[2]
  assert got[0][:, 2].min() == 0 and got[0][:, 2].max() == 5


def test_gather_refuses_entries_out_of_range(ops):
  from ffn_amd import _lib
  ops.reset()
  counts = ops.add_volume(np.array([[[0, 0, 1, 255]]], np.uint8))
  assert counts[0] == 2 and counts[1] == 1
  good = dict(classes=[0, 1], max_count=2,
              perms=[np.array([1, 0]), np.array([0])],
              order=np.array([3, 0, 2, 1]), margin=(0, 0, 0))
  ops.gather(**good)
  assert ops.read()[0][:, 0].tolist() == [2, 1, 2, 0]
  for change in (dict(order=np.array([4, 0, 2, 1])),
                 dict(perms=[np.array([2, 0]), np.array([0])]),
                 dict(perms=[np.array([1, 0]), np.array([1])]),
                 dict(classes=[0, 2]), dict(classes=[0, 0]),
                 dict(order=np.array([3, 0, 2]))):
    with pytest.raises(_lib.FFNHipError):
      ops.gather(**dict(good, **change))
    with pytest.raises(_lib.FFNHipError):  # nothing half-made stays readable
      ops.read()
    ops.gather(**good)


def varint_volume():
  """Centres on both sides of the 1-, 2- and 3-byte varint boundaries, in two
  volumes whose names have length 1 and 40."""
  wide = np.full((3, 130, 16390), 255, np.uint8)
  for z, y, x, c in ((1, 127, 127, 0), (1, 128, 128, 0), (1, 127, 16383, 1),
                     (1, 128, 16384, 1)):
    wide[z, y, x] = c
  small = runs((4, 5, 9), 31, [0, 1, 3], mean_run=4)
  return [('w', wide), ('n' * 40, small)]


def test_serialize_equals_the_python_encoder(ops):
  volumes = varint_volume()
  names = [n for n, _ in volumes]
  centers, volume, _ = ops.build(volumes, (1, 1, 1), np.random.RandomState(8))
  for value in (127, 128, 16383, 16384):
    assert (centers[:, 0] == value).any()
  assert (centers[:, 1] == 127).any() and (centers[:, 1] == 128).any()
  assert set(volume.tolist()) == {0, 1}
  want = coordinates_ref.tfrecord_bytes(centers, volume, names)
  n = len(centers)
  assert ops.serialize(0, n) == want
  # windows whose boundaries fall inside the row range
  for window in (1, 5, 64, 257):
    assert b''.join(ops.serialize(r, min(window, n - r))
                    for r in range(0, n, window)) == want
  one = coordinates_ref.tfrecord_bytes(centers[7:8], volume[7:8], names)
  assert ops.serialize(7, 1) == one
  _, _, (ms, nbytes) = ops.last_timing()
  assert ms > 0 and nbytes == 16 + len(one)
  # other names for the same rows
  ops.set_names(['x' * 130, 'y'])
  assert ops.serialize(0, n) == coordinates_ref.tfrecord_bytes(
      centers, volume, ['x' * 130, 'y'])


def test_write_tfrecord_streams_windows(ops, tmp_path):
  from ffn_amd import coordinates
  case = CASES['three']
  names = [n for n, _ in case['volumes']]
  ops.build(case['volumes'], case['margin'],
            np.random.RandomState(case['seed']))
  path = str(tmp_path / 'coords')
  total = ops.write_tfrecord(path, window=1000)
  with gzip.open(path, 'rb') as f:
    data = f.read()
  assert len(data) == total
  assert data == coordinates_ref.tfrecord_bytes(case['centers'],
                                                case['volume'], names)
  centers, got_names = coordinates.read_tfrecord(path)
  assert np.array_equal(centers, case['centers'])
  assert got_names == [names[i] for i in case['volume']]


def test_cli_end_to_end(tmp_path):
  import build_coordinates as root
  from ffn_amd import coordinates
  from ffn_amd import partitions
  seg = partitions_ref.voronoi_labels((48, 48, 48), 9, 5, dtype=np.uint32)
  radius = (4, 4, 4)
  part = partitions.default_ops(0).compute(
      seg, [0.1, 0.3, 0.5, 0.7, 0.9], radius, min_size=100)
  full = np.full(seg.shape, 255, np.uint8)  # what compute_partitions.py writes
  full[4:-4, 4:-4, 4:-4] = part
  src, dst = str(tmp_path / 'af.npz'), str(tmp_path / 'coords.gz')
  np.savez_compressed(src, partitions=full)
  margin = (16, 15, 17)
  root.main(['--partition_volumes', 'validation1:' + src,
             '--coordinate_output', dst, '--margin', '16,15,17', '--seed', '77'])
  with gzip.open(dst, 'rb') as f:  # decompresses
    data = f.read()
  centers, names = coordinates.read_tfrecord(dst)  # passes every CRC
  want = coordinates_ref.coordinates_spec([('validation1', full)], margin,
                                          np.random.RandomState(77))
  assert np.array_equal(centers, want[0])
  assert set(names) == {'validation1'} and len(names) == len(want[0])
  assert data == coordinates_ref.tfrecord_bytes(
      want[0], want[1], ['validation1'])
  classes = full[centers[:, 2], centers[:, 1], centers[:, 0]]
  values, counts = np.unique(classes, return_counts=True)
  assert values.tolist() == sorted(want[2]) and len(values) >= 2
  assert set(counts.tolist()) == {max(want[2].values())}
  # the .npz form of the same run
  alt = str(tmp_path / 'coords.npz')
  root.main(['--partition_volumes', 'validation1:%s:partitions' % src,
             '--coordinate_output', alt, '--margin', '16,15,17', '--seed', '77'])
  with np.load(alt) as out:
    assert np.array_equal(out['centers'], want[0])
    assert np.array_equal(out['volume_index'], want[1])
    assert out['volume_names'].tolist() == ['validation1']


def test_handle_closes_twice_and_the_default_is_one_object():
  from ffn_amd import _lib
  from ffn_amd import coordinates
  assert coordinates.default_ops(0) is coordinates.default_ops(0)
  obj = coordinates.CoordinateOps(0)
  assert obj.device_id == 0 and obj._h
  obj.close()
  assert not obj._h
  obj.close()
  with pytest.raises(_lib.FFNHipError):
    obj.add_volume(np.zeros((2, 2, 2), np.uint8))
