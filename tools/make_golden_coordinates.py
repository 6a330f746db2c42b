#!/usr/bin/env python3
"""Mints tests/golden/ref_coordinates.npz with the reference's own
build_coordinates.py (at the root of the google/ffn checkout).

Runs in the build container only (needs the reference checkout).  The
reference module is imported through tools/ref_shims and its main() runs
unmodified.  Three things stand in for its surroundings, all defined here:

  * `h5py.File` opens an in-memory table {path: {dataset: array}};
  * `tf.train` / `tf.python_io` are plain recorders: the message classes keep
    their keyword arguments, SerializeToString() hands the message itself on,
    and the writer appends whatever it is given to a list;
  * the module's FLAGS is a namespace with the three flags (the absl shim
    leaves FLAGS as None), and its `logging` keeps the partition counts.

np.random.seed(seed) is called before each run.  Per case the file holds the
input volumes, names, margin and seed, the (centre, volume) sequence the
reference handed to its writer, and the classes and totals it logged, in its
dict order.  The minter asserts what each case is there for, and that the numpy
restatement (tests/coordinates_ref.py) gives the same sequence.
"""
import importlib.util
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('FFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402

import coordinates_ref  # noqa: E402

# (by path: this repository's root has a build_coordinates.py of its own)
_spec = importlib.util.spec_from_file_location(
    'ref_build_coordinates', os.path.join(REF, 'build_coordinates.py'))
ref_bc = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_bc)

GOLD = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 300 * 1000

# ---- stand-ins ---------------------------------------------------------------------

STORE = {}  # path -> {dataset: array}


class MemoryFile:
  """h5py.File over STORE, read-only."""

  def __init__(self, path, mode='r'):
    assert mode == 'r'
    self._datasets = STORE[path]

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    return False

  def __getitem__(self, dataset):
    return self._datasets[dataset]


class Message:
  """A protobuf message class that only keeps its keyword arguments."""

  def __init__(self, **fields):
    self.__dict__.update(fields)

  def SerializeToString(self):  # pylint:disable=invalid-name
    return self


class RecordingWriter:
  written = []
  opened = []

  def __init__(self, path, options=None):
    RecordingWriter.opened.append((path, options))

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    return False

  def write(self, record):
    RecordingWriter.written.append(record)


class CompressionType:
  NONE, ZLIB, GZIP = 0, 1, 2


class RecordingLog:
  lines = []

  @classmethod
  def info(cls, fmt, *args):
    cls.lines.append((fmt, args))


def install():
  ref_bc.h5py = types.SimpleNamespace(File=MemoryFile)
  ref_bc.tf = types.SimpleNamespace(
      train=types.SimpleNamespace(
          Feature=Message, Features=Message, Example=Message,
          Int64List=Message, BytesList=Message),
      python_io=types.SimpleNamespace(
          TFRecordOptions=lambda compression: ('options', compression),
          TFRecordCompressionType=CompressionType,
          TFRecordWriter=RecordingWriter))
  ref_bc.logging = RecordingLog


def run_reference(case):
  """The reference's main() on a case -> (centres (N, 3), volume indices (N,),
  classes, totals)."""
  STORE.clear()
  specs = []
  for i, (name, vol) in enumerate(case['volumes']):
    path = '/memory/%d.h5' % i
    STORE[path] = {'af': vol.copy()}
    specs.append('%s:%s:af' % (name, path))
  ref_bc.FLAGS = types.SimpleNamespace(
      partition_volumes=specs, coordinate_output='/memory/out',
      margin=[str(m) for m in case['margin']])
  RecordingWriter.written, RecordingWriter.opened = [], []
  RecordingLog.lines = []
  np.random.seed(case['seed'])
  ref_bc.main([])
  assert RecordingWriter.opened == [
      ('/memory/out', ('options', CompressionType.GZIP))]
  names = [name for name, _ in case['volumes']]
  centers, volume = [], []
  for example in RecordingWriter.written:
    feature = example.features.feature
    assert sorted(feature) == ['center', 'label_volume_name']
    centers.append([int(v) for v in feature['center'].int64_list.value])
    (name,) = feature['label_volume_name'].bytes_list.value
    volume.append(names.index(name.decode('utf-8')))
  counts = [args for fmt, args in RecordingLog.lines if fmt == ' %d: %d']
  return (np.array(centers, np.int64), np.array(volume, np.int64),
          [int(k) for k, _ in counts], [int(v) for _, v in counts])


# ---- cases -------------------------------------------------------------------------


def blocks(shape, values, seed, cell=(3, 4, 9), border=0):
  """A map of box-shaped runs of the given values, as a partition map has them,
  with `border` voxels of 255 around it."""
  rng = np.random.RandomState(seed)
  grid = [-(-n // c) for n, c in zip(shape, cell)]
  coarse = rng.choice(np.asarray(values, np.uint8), size=grid)
  vol = np.kron(coarse, np.ones(cell, np.uint8))[:shape[0], :shape[1],
                                                 :shape[2]].copy()
  if border:
    inner = vol[border:-border, border:-border, border:-border].copy()
    vol[...] = 255
    vol[border:-border, border:-border, border:-border] = inner
  return vol


def make_cases():
  lone = np.full((14, 15, 23), 3, np.uint8)
  lone[6, 7, 11] = 7  # one voxel of class 7 beside thousands of class 3
  lone[0, 0, 0] = 9   # inside the margin: never seen
  speckle = np.random.RandomState(5).randint(0, 4, (9, 10, 21)).astype(np.uint8)
  first = blocks((10, 12, 30), [2, 5, 255], 11)
  second = blocks((9, 13, 27), [1, 2, 5, 6], 12)
  cases = {
      'one': dict(volumes=[('vol', blocks((12, 14, 71), [0, 1, 2, 4, 255], 1))],
                  margin=(1, 2, 3), seed=101),
      'new_class_in_second': dict(volumes=[('a', first), ('b', second)],
                                  margin=(1, 1, 1), seed=102),
      'second_first': dict(volumes=[('b', second), ('a', first)],
                           margin=(1, 1, 1), seed=102),
      'three': dict(volumes=[('x', blocks((8, 9, 33), [0, 3], 21)),
                             ('validation1', blocks((11, 8, 19), [3, 8], 22)),
                             ('z', blocks((7, 12, 40), [0, 8, 12], 23))],
                    margin=(2, 1, 2), seed=103),
      'lone_voxel': dict(volumes=[('lone', lone)], margin=(1, 1, 1), seed=104),
      'all_ignored_beside': dict(
          volumes=[('empty', np.full((6, 7, 8), 255, np.uint8)),
                   ('full', blocks((8, 9, 35), [1, 2, 255], 31))],
          margin=(1, 1, 1), seed=105),
      'only_zero': dict(volumes=[('bg', blocks((6, 8, 20), [0, 255], 41))],
                        margin=(1, 1, 1), seed=106),
      'unequal_margins': dict(volumes=[('m', blocks((16, 9, 29), [1, 2, 3], 51))],
                              margin=(5, 1, 3), seed=107),
      'wide_x': dict(volumes=[('w', blocks((4, 5, 131), [0, 6, 255], 61,
                                           cell=(2, 2, 50)))],
                     margin=(1, 1, 1), seed=108),
      'speckle': dict(volumes=[('s', speckle)], margin=(1, 2, 1), seed=109),
      'partition_like': dict(
          volumes=[('p', blocks((20, 33, 70), [0, 1, 2, 3, 4], 71,
                                cell=(5, 8, 30), border=4))],
          margin=(2, 2, 2), seed=110),
  }
  return cases


def check_purpose(name, case, centers, volume, classes, totals):
  crops = [coordinates_ref.crop_of(v, case['margin']) for _, v in
           case['volumes']]
  assert min(case['margin']) >= 1  # the reference cannot express 0
  assert len(centers) == len(classes) * max(totals)
  if name == 'one':
    assert len(crops) == 1 and crops[0].shape[2] % 64 and len(classes) == 4
    assert (crops[0] == 255).any()
  if name == 'new_class_in_second':
    # 1 is smaller than 2 and 5 but first appears in the second volume
    assert classes == [2, 5, 1, 6]
  if name == 'second_first':
    assert classes == [1, 2, 5, 6]
  if name == 'three':
    assert len(crops) == 3 and set(volume.tolist()) == {0, 1, 2}
    assert classes == [0, 3, 8, 12]
  if name == 'lone_voxel':
    assert classes == [3, 7] and min(totals) == 1 and max(totals) > 2000
    lone = (centers == (11, 7, 6)).all(axis=1)  # xyz of seg[6, 7, 11]
    assert lone.sum() == max(totals)
  if name == 'all_ignored_beside':
    assert (crops[0] == 255).all() and set(volume.tolist()) == {1}
  if name == 'only_zero':
    assert classes == [0] and (crops[0] == 255).any()
  if name == 'unequal_margins':
    assert len(set(case['margin'])) == 3
  if name == 'wide_x':
    assert crops[0].shape[2] > 128 and crops[0].shape[2] % 64
  if name == 'speckle':
    assert (np.diff(crops[0].ravel().astype(int)) != 0).mean() > 0.6
  if name == 'partition_like':
    assert (case['volumes'][0][1][3] == 255).all() and len(classes) == 5


def main():
  install()
  cases = make_cases()
  out = {'cases': np.array(sorted(cases))}
  for name in sorted(cases):
    case = cases[name]
    centers, volume, classes, totals = run_reference(case)
    spec = coordinates_ref.coordinates_spec(
        case['volumes'], case['margin'], np.random.RandomState(case['seed']))
    assert np.array_equal(spec[0], centers), name
    assert np.array_equal(spec[1], volume), name
    assert list(spec[2].items()) == list(zip(classes, totals)), name
    check_purpose(name, case, centers, volume, classes, totals)
    out[name + '_names'] = np.array([n for n, _ in case['volumes']])
    for i, (_, vol) in enumerate(case['volumes']):
      out['%s_vol%d' % (name, i)] = vol
    out[name + '_margin'] = np.array(case['margin'], np.int64)
    out[name + '_seed'] = np.array(case['seed'], np.int64)
    # (in the narrowest types that hold them)
    out[name + '_centers'] = centers.astype(
        np.min_scalar_type(int(centers.max())))
    out[name + '_volume'] = volume.astype(np.uint8)
    out[name + '_classes'] = np.array(classes, np.uint8)
    out[name + '_totals'] = np.array(totals, np.int64)
    print('%-20s %d volume(s) margin %s -> %6d rows, classes %s totals %s' % (
        name, len(case['volumes']), case['margin'], len(centers), classes,
        totals))
  dst = os.path.join(GOLD, 'ref_coordinates.npz')
  np.savez_compressed(dst, **out)
  size = os.path.getsize(dst)
  print('wrote', dst, size, 'bytes')
  assert size < MAX_BYTES, size


if __name__ == '__main__':
  main()
