"""Balanced training coordinates without a GPU: the numpy restatement
(tests/coordinates_ref.py) against the reference's own build_coordinates.py
(tests/golden/ref_coordinates.npz, minted by tools/make_golden_coordinates.py),
the two np.random equalities the host / device split rests on, the TFRecord
bytes (CRC32C, the Python encoder through read_tfrecord and through
google.protobuf), the limits, and the script's path grammar."""
import gzip
import os

import numpy as np
import pytest

from tests import coordinates_ref

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden',
                      'ref_coordinates.npz')


def load_cases():
  g = np.load(GOLDEN)
  cases = {}
  for name in g['cases']:
    name = str(name)
    names = [str(n) for n in g[name + '_names']]
    cases[name] = dict(
        volumes=[(n, g['%s_vol%d' % (name, i)]) for i, n in enumerate(names)],
        margin=tuple(int(m) for m in g[name + '_margin']),
        seed=int(g[name + '_seed']),
        centers=g[name + '_centers'].astype(np.int64),
        volume=g[name + '_volume'].astype(np.int64),
        totals=dict(zip(g[name + '_classes'].tolist(),
                        g[name + '_totals'].tolist())))
  return cases


CASES = load_cases() if os.path.exists(GOLDEN) else {}


def test_fixture_has_the_cases_the_specification_names():
  assert set(CASES) == {
      'one', 'new_class_in_second', 'second_first', 'three', 'lone_voxel',
      'all_ignored_beside', 'only_zero', 'unequal_margins', 'wide_x', 'speckle',
      'partition_like'}
  assert os.path.getsize(GOLDEN) < 300 * 1000
  assert sorted(len(c['volumes']) for c in CASES.values())[-1] == 3
  assert list(CASES['new_class_in_second']['totals']) == [2, 5, 1, 6]
  assert list(CASES['second_first']['totals']) == [1, 2, 5, 6]
  lone = CASES['lone_voxel']['totals']
  assert min(lone.values()) == 1 and max(lone.values()) > 2000
  assert (CASES['all_ignored_beside']['volumes'][0][1] == 255).all()
  assert list(CASES['only_zero']['totals']) == [0]
  assert len(set(CASES['unequal_margins']['margin'])) == 3
  for case in CASES.values():
    assert min(case['margin']) >= 1
    assert len(case['centers']) == len(case['totals']) * max(
        case['totals'].values())
  assert any((v.shape[2] - 2 * c['margin'][2]) % 64
             for c in CASES.values() for _, v in c['volumes'])


@pytest.mark.parametrize('name', sorted(CASES))
def test_restatement_reproduces_the_reference(name):
  case = CASES[name]
  before = [v.copy() for _, v in case['volumes']]
  centers, volume, totals = coordinates_ref.coordinates_spec(
      case['volumes'], case['margin'], np.random.RandomState(case['seed']))
  assert np.array_equal(centers, case['centers'])
  assert np.array_equal(volume, case['volume'])
  assert list(totals.items()) == list(case['totals'].items())
  assert all(np.array_equal(v, b)
             for (_, v), b in zip(case['volumes'], before))
  # every class exactly max_count times
  flat = [v[tuple(slice(m, n - m) for m, n in zip(case['margin'], v.shape))]
          for _, v in case['volumes']]
  mz, my, mx = case['margin']
  classes = np.array([flat[i][z - mz, y - my, x - mx]
                      for (x, y, z), i in zip(centers, volume)])
  values, counts = np.unique(classes, return_counts=True)
  assert sorted(values.tolist()) == sorted(totals)
  assert set(counts.tolist()) == {max(totals.values())}


def test_restatement_uses_the_global_generator_like_the_reference():
  case = CASES['three']
  np.random.seed(case['seed'])
  centers, volume, _ = coordinates_ref.coordinates_spec(case['volumes'],
                                                       case['margin'])
  assert np.array_equal(centers, case['centers'])
  assert np.array_equal(volume, case['volume'])


@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 65, 1000, 4097, 50000])
def test_permutation_of_rows_is_rows_of_a_permutation(n):
  rows = np.stack([np.arange(n) % 3, np.arange(n)[::-1] * 7], 1)
  a = np.random.RandomState(n)
  b = np.random.RandomState(n)
  assert np.array_equal(a.permutation(rows), rows[b.permutation(n)])
  # and on a list of tuples, which is what the reference hands over
  c = np.random.RandomState(n)
  assert np.array_equal(c.permutation([tuple(r) for r in rows.tolist()]),
                        rows[np.random.RandomState(n).permutation(n)])
  # the generators are left in the same state
  assert a.randint(1 << 30) == b.randint(1 << 30)


@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 65, 1000, 4097, 50000])
def test_shuffle_of_rows_is_rows_of_a_shuffled_index(n):
  rows = np.stack([np.arange(n) % 5, np.arange(n) * 3 + 1], 1)
  a = np.random.RandomState(n + 7)
  b = np.random.RandomState(n + 7)
  shuffled = rows.copy()
  a.shuffle(shuffled)
  order = np.arange(n, dtype=np.uint32)
  b.shuffle(order)
  assert np.array_equal(shuffled, rows[order])
  assert a.randint(1 << 30) == b.randint(1 << 30)


def test_crc32c_known_answers():
  from ffn_amd import coordinates
  for crc in (coordinates.crc32c, coordinates_ref.crc32c):
    assert crc(b'123456789') == 0xE3069283
    assert crc(bytes(32)) == 0x8A9136AA
  data = bytes(range(256)) * 3
  assert coordinates.crc32c(data) == coordinates_ref.crc32c(data)
  assert coordinates.masked_crc32c(data) == coordinates_ref.masked_crc(data)


ROWS = np.array([[0, 0, 0], [127, 128, 16383], [16384, 2097151, 2097152],
                 [2**31 - 1, 1, 5], [-1, 3, -2**31]], np.int64)
ROW_VOLUMES = np.array([0, 1, 2, 1, 0])
ROW_NAMES = ['v', 'validation1', 'n' * 200]


def test_encoder_round_trips_through_read_tfrecord(tmp_path):
  from ffn_amd import coordinates
  data = coordinates_ref.tfrecord_bytes(ROWS, ROW_VOLUMES, ROW_NAMES)
  for name, opener in (('plain', open), ('packed.gz', gzip.open)):
    path = str(tmp_path / name)
    with opener(path, 'wb') as f:
      f.write(data)
    centers, names = coordinates.read_tfrecord(path)
    assert centers.dtype == np.int64 and np.array_equal(centers, ROWS)
    assert names == [ROW_NAMES[i] for i in ROW_VOLUMES]


@pytest.mark.parametrize('where', ['length', 'length_crc', 'payload',
                                   'payload_crc', 'truncated'])
def test_read_tfrecord_verifies_both_crcs(tmp_path, where):
  from ffn_amd import coordinates
  data = bytearray(coordinates_ref.tfrecord_bytes(ROWS[:2], ROW_VOLUMES[:2],
                                                  ROW_NAMES))
  first = len(coordinates_ref.record_bytes(
      coordinates_ref.example_bytes(ROWS[0], b'v')))
  at = {'length': first, 'length_crc': first + 9, 'payload': first + 20,
        'payload_crc': len(data) - 2}.get(where)
  if at is None:
    data = data[:-3]
  else:
    data[at] ^= 0x10
  path = str(tmp_path / 'bad')
  with open(path, 'wb') as f:
    f.write(bytes(data))
  with pytest.raises(ValueError):
    coordinates.read_tfrecord(path)


def example_class():
  """tf.train.Example declared at run time, its map as the wire-equivalent
  repeated entry message: a decoder that owes nothing to this repository."""
  from google.protobuf import descriptor_pb2
  from google.protobuf import descriptor_pool
  from google.protobuf import message_factory
  fd = descriptor_pb2.FileDescriptorProto(
      name='coordinates_test_example.proto', package='coordinates_test',
      syntax='proto3')
  T = descriptor_pb2.FieldDescriptorProto

  def message(name, *fields):
    m = fd.message_type.add(name=name)
    for fname, number, ftype, label, type_name in fields:
      f = m.field.add(name=fname, number=number, type=ftype, label=label)
      if type_name:
        f.type_name = '.coordinates_test.' + type_name
  one, many = T.LABEL_OPTIONAL, T.LABEL_REPEATED
  message('BytesList', ('value', 1, T.TYPE_BYTES, many, None))
  message('Int64List', ('value', 1, T.TYPE_INT64, many, None))
  message('Feature', ('bytes_list', 1, T.TYPE_MESSAGE, one, 'BytesList'),
          ('int64_list', 3, T.TYPE_MESSAGE, one, 'Int64List'))
  message('Entry', ('key', 1, T.TYPE_STRING, one, None),
          ('value', 2, T.TYPE_MESSAGE, one, 'Feature'))
  message('Features', ('feature', 1, T.TYPE_MESSAGE, many, 'Entry'))
  message('Example', ('features', 1, T.TYPE_MESSAGE, one, 'Features'))
  pool = descriptor_pool.DescriptorPool()
  pool.Add(fd)
  return message_factory.GetMessageClass(
      pool.FindMessageTypeByName('coordinates_test.Example'))


def test_encoder_parses_through_protobuf():
  from ffn_amd import coordinates
  Example = example_class()
  data = coordinates_ref.tfrecord_bytes(ROWS, ROW_VOLUMES, ROW_NAMES)
  payloads = list(coordinates.iter_records(data))
  assert len(payloads) == len(ROWS)
  for payload, row, vol in zip(payloads, ROWS, ROW_VOLUMES):
    ex = Example.FromString(payload)
    entries = {e.key: e.value for e in ex.features.feature}
    assert [e.key for e in ex.features.feature] == ['center',
                                                    'label_volume_name']
    assert list(entries['center'].int64_list.value) == row.tolist()
    assert list(entries['label_volume_name'].bytes_list.value) == [
        ROW_NAMES[vol].encode()]
    # protobuf's own serialisation of the same message is the same bytes
    assert ex.SerializeToString() == payload
    assert coordinates.parse_example(payload) == (row.tolist(),
                                                  ROW_NAMES[vol].encode())


class NoDevice:
  def __getattr__(self, name):
    raise AssertionError('device call: ' + name)


@pytest.fixture
def ops_without_device():
  import threading
  from ffn_amd import coordinates
  ops = coordinates.CoordinateOps.__new__(coordinates.CoordinateOps)
  ops._lib, ops._h, ops._destroy = NoDevice(), None, lambda h: None
  ops.lock = threading.RLock()
  ops.num_rows = ops.num_volumes = 0
  ops.split = {}
  return ops


GOOD = np.zeros((6, 7, 8), np.uint8)


@pytest.mark.parametrize('volumes,margin,error', [
    ([('v', GOOD.astype(np.int32))], (1, 1, 1), TypeError),
    ([('v', GOOD.astype(np.float32))], (1, 1, 1), TypeError),
    ([('v', GOOD[0])], (1, 1, 1), ValueError),
    ([('v', GOOD)], (3, 1, 1), ValueError),          # 2 m = axis length
    ([('v', GOOD)], (1, 1, 4), ValueError),
    ([('v', GOOD)], (1, -1, 1), ValueError),
    ([('v', GOOD)], (1, 1.5, 1), ValueError),
    ([('v', GOOD)], (1, 1), ValueError),
    ([('', GOOD)], (1, 1, 1), ValueError),
    ([('a:b', GOOD)], (1, 1, 1), ValueError),
    ([(b'v', GOOD)], (1, 1, 1), ValueError),
    ([], (1, 1, 1), ValueError),
    ([('v', np.full((6, 7, 8), 255, np.uint8))], (1, 1, 1), ValueError),
    # everything but the margin is a class
    ([('v', np.pad(np.full((2, 2, 2), 255, np.uint8), 2))], (2, 2, 2),
     ValueError),
])
def test_limits_raise_before_any_device_call(ops_without_device, volumes,
                                             margin, error):
  with pytest.raises(error):
    ops_without_device.build(volumes, margin, np.random.RandomState(0))


def test_row_limit_raises_before_any_device_call(ops_without_device,
                                                 monkeypatch):
  from ffn_amd import coordinates
  with pytest.raises(ValueError, match='2\\^31'):
    coordinates.check_rows({0: 2**30, 1: 5})
  assert coordinates.check_rows({0: 2**30}) == 2**30
  with pytest.raises(ValueError, match='255'):
    coordinates.check_rows({})
  # the same path inside build(), with the limit brought down to the volume
  vol = np.zeros((6, 7, 8), np.uint8)
  vol[3:] = 1
  monkeypatch.setattr(coordinates, '_MAX_ROWS', 2 * 3 * 7 * 8)
  with pytest.raises(ValueError, match='2\\^31'):
    ops_without_device.build([('v', vol)], (0, 0, 0))
  vol[0, 0, 0] = vol[5, 0, 0] = 255  # below the limit: the device is asked
  with pytest.raises(AssertionError, match='device call'):
    ops_without_device.build([('v', vol)], (0, 0, 0))


def test_voxel_limit_raises_before_any_device_call(ops_without_device):
  # 2^31 voxels over one byte of memory: the size is looked at before the data
  big = np.lib.stride_tricks.as_strided(
      np.zeros(1, np.uint8), (2048, 1024, 1024), (0, 0, 0))
  with pytest.raises(ValueError, match='2\\^31'):
    ops_without_device.build([('v', big)], (0, 0, 0))
  with pytest.raises(ValueError, match='2\\^31'):
    ops_without_device.build([('small', GOOD), ('v', big)], (0, 0, 0))
  # the limit is on the crop: exactly 2^31 voxels are left of a larger volume
  padded = np.lib.stride_tricks.as_strided(
      np.zeros(1, np.uint8), (2050, 1026, 1026), (0, 0, 0))
  with pytest.raises(ValueError, match='2\\^31'):
    ops_without_device.build([('v', padded)], (1, 1, 1))


def test_margin_zero_means_no_crop_and_reaches_the_device(ops_without_device):
  from ffn_amd import coordinates
  names, crops, margin = coordinates.check_volumes([('v', GOOD)], (0, 2, 0))
  assert names == ['v'] and margin == (0, 2, 0)
  assert crops[0].shape == (6, 3, 8) and np.shares_memory(crops[0], GOOD)
  with pytest.raises(AssertionError, match='device call'):
    ops_without_device.build([('v', GOOD)], (0, 0, 0))


def test_script_path_grammar(tmp_path):
  import build_coordinates as root
  split = root.split_volume_spec
  assert split('a:dir/x.npy') == ('a', 'dir/x.npy', None)
  assert split('a:x.npz') == ('a', 'x.npz', 'partitions')
  assert split('a:x.npz:af') == ('a', 'x.npz', 'af')
  assert split('validation1:vol.h5:af') == ('validation1', 'vol.h5', 'af')
  for bad in ('x.npy', ':x.npy', 'a:', 'a:x.npy:b', 'a:x.npz:b:c', 'a:x.npz:',
              'a:vol.h5', 'a:vol.h5:', 'a:vol.h5:b:c', ''):
    with pytest.raises(ValueError):
      split(bad)
  vol = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
  np.save(str(tmp_path / 'p.npy'), vol)
  np.savez(str(tmp_path / 'p.npz'), partitions=vol, other=vol + 1)
  name, got = root.load_volume('n:%s' % (tmp_path / 'p.npy'))
  assert name == 'n' and np.array_equal(got, vol)
  assert np.array_equal(root.load_volume('n:%s' % (tmp_path / 'p.npz'))[1], vol)
  assert np.array_equal(
      root.load_volume('n:%s:other' % (tmp_path / 'p.npz'))[1], vol + 1)
  try:
    import h5py  # noqa: F401
  except ImportError:
    with pytest.raises(NotImplementedError, match='h5py is not available'):
      root.load_volume('n:%s:af' % (tmp_path / 'p.h5'))


def test_script_flags():
  import build_coordinates as root
  with pytest.raises(SystemExit):
    root.main(['--partition_volumes', 'a:x.npy', '--coordinate_output', 'o',
               '--margin', '1,2'])
  with pytest.raises(SystemExit):
    root.main(['--coordinate_output', 'o', '--margin', '1,2,3'])


@pytest.mark.parametrize('name_len', [1, 40, 127, 128, 200, 20000])
def test_record_bound_is_the_longest_record_of_a_name(name_len):
  from ffn_amd import coordinates
  name = b'n' * name_len
  longest = coordinates_ref.record_bytes(
      coordinates_ref.example_bytes(np.array([-1, -1, -2**31]), name))
  assert coordinates.record_bound(name_len) == len(longest)
  usual = coordinates_ref.record_bytes(
      coordinates_ref.example_bytes(np.array([2**31 - 1, 16384, 0]), name))
  assert len(usual) < len(longest)


def test_serialize_makes_room_for_the_longest_name_at_once(ops_without_device):
  """One library call per window: the first buffer already holds the records
  of the longest name, so the size pass is not run twice."""
  rows = np.array([[2**31 - 1, 2**31 - 1, 2**31 - 1]] * 3, np.int64)
  names = ['v', 'n' * 40]
  want = len(coordinates_ref.tfrecord_bytes(rows, np.array([1, 1, 1]), names))
  caps = []

  class Lib:
    def ffn_coordinates_set_names(self, h, blob, offsets, n):
      return 0

    def ffn_coordinates_serialize(self, h, row0, n_rows, cap, out, found):
      caps.append(cap)
      found._obj.value = want
      assert want <= cap, 'the library would refuse and be called again'
      return 0

  ops_without_device._lib = Lib()
  ops_without_device.set_names(names)
  assert len(ops_without_device.serialize(0, 3)) == want
  assert len(caps) == 1 and want <= caps[0] <= 2 * want
