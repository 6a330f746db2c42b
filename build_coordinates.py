#!/usr/bin/env python3
r"""Balanced training coordinates from partition maps on one MI355X.

Drop-in for the reference's build_coordinates.py: the same three flags and,
for a seed, the same sequence of examples.  Every partition class other than
255 is resampled to the size of the largest class and all coordinates are
shuffled; the result is a GZIP-compressed TFRecord file of tf.train.Example
records {center: [x, y, z], label_volume_name}, written and read back without
TensorFlow.  The voxel work is done by the HIP kernels behind
ffn_amd/coordinates.py (there is no CPU fallback).

  python build_coordinates.py --margin 24,24,24 \
      --partition_volumes validation1:proofread_partitions.npz \
      --coordinate_output tf_record_file

A volume is `<name>:<file>.npz` (optionally `:<array>`; the default array is
`partitions`, which is what this repository's compute_partitions.py writes:
input-shaped, 255 outside the valid region), `<name>:<file>.npy`, or
`<name>:<file>:<dataset>` of an HDF5 file where h5py is installed.  An output
path ending in `.npz` gets the arrays `centers`, `volume_index` and
`volume_names` instead of a TFRecord file.

Two things are read differently from the reference.  A margin of 0 means "no
crop" on that axis (the reference slices [m:-m], which is empty for 0, and then
stops in max() of nothing).  `--seed` seeds numpy's global generator before the
draws; the reference always runs unseeded, which is the default here too.
"""

import argparse
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from ffn_amd import coordinates as coordinate_ops  # noqa: E402

_NO_H5PY = ('h5py is not available in this environment; convert the volume to '
            '.npy and use `image { npy: "..." }`')


def split_volume_spec(spec):
  """'<name>:<file>.npy' -> (name, file, None); '<name>:<file>.npz[:<array>]'
  -> (name, file, array or 'partitions'); '<name>:<file>:<dataset>' -> (name,
  file, dataset) of an HDF5 file."""
  parts = spec.split(':')
  if len(parts) < 2 or not parts[0] or not parts[1]:
    raise ValueError('partition volume should be <name>:<file>.npz[:<array>], '
                     '<name>:<file>.npy or <name>:<hdf5 file>:<dataset>.  '
                     'Got: %s' % spec)
  name, filename, rest = parts[0], parts[1], parts[2:]
  if filename.endswith('.npy') and not rest:
    return name, filename, None
  if filename.endswith('.npz') and len(rest) <= 1 and all(rest):
    return name, filename, rest[0] if rest else 'partitions'
  if len(rest) == 1 and rest[0] and not filename.endswith(('.npy', '.npz')):
    return name, filename, rest[0]
  raise ValueError('partition volume should be <name>:<file>.npz[:<array>], '
                   '<name>:<file>.npy or <name>:<hdf5 file>:<dataset>.  '
                   'Got: %s' % spec)


def _h5py():
  try:
    import h5py  # pylint:disable=g-import-not-at-top
  except ImportError as e:
    raise NotImplementedError(_NO_H5PY) from e
  return h5py


def load_volume(spec):
  """Returns (name, uint8 partition map zyx)."""
  name, filename, key = split_volume_spec(spec)
  if filename.endswith('.npy'):
    return name, np.load(filename)
  if filename.endswith('.npz'):
    with np.load(filename) as f:
      return name, f[key]
  with _h5py().File(filename, 'r') as f:
    return name, f[key][...]


def build_coordinates(volumes, margin, coordinate_output, seed=None,
                      device_id=0):
  """Writes the coordinates of `volumes`, a list of (name, partition map), to
  `coordinate_output`; the definition is in
  ffn_amd.coordinates.CoordinateOps.build.  Returns the {class: total} dict."""
  ops = coordinate_ops.default_ops(device_id)
  if seed is not None:
    np.random.seed(seed)
  centers, volume_index, totals = ops.build(volumes, margin)
  logging.info('Partition counts:')
  for k, v in totals.items():
    logging.info(' %d: %d', k, v)
  logging.info('Saving %d coordinates.', len(centers))
  if coordinate_output.endswith('.npz'):
    np.savez_compressed(coordinate_output, centers=centers,
                        volume_index=volume_index,
                        volume_names=np.array([n for n, _ in volumes]))
  else:
    ops.write_tfrecord(coordinate_output)
  return totals


def _csv(convert):
  return lambda text: [convert(v) for v in text.split(',') if v.strip()]


def main(argv=None):
  ap = argparse.ArgumentParser(
      description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--partition_volumes', required=True, type=_csv(str),
                  help='comma-separated <name>:<file>.npz[:<array>], '
                  '<name>:<file>.npy or <name>:<hdf5 file>:<dataset>; <name> '
                  'is the label the training script knows the volume by')
  ap.add_argument('--coordinate_output', required=True,
                  help='TFRecord file to write (GZIP), or <file>.npz')
  ap.add_argument('--margin', required=True, type=_csv(int),
                  help='z,y,x voxels next to the border of a volume to leave '
                  'out: normally the radius of the training FoV plus deltas')
  ap.add_argument('--seed', type=int, default=None,
                  help='seed of numpy\'s global generator (default: unseeded, '
                  'as the reference runs)')
  ap.add_argument('--device', type=int, default=0)
  args = ap.parse_args(argv)
  logging.basicConfig(level=logging.INFO)
  if len(args.margin) != 3:
    ap.error('--margin takes three integers z,y,x')
  if not args.partition_volumes:
    ap.error('--partition_volumes is empty')
  volumes = [load_volume(spec) for spec in args.partition_volumes]
  build_coordinates(volumes, args.margin, args.coordinate_output,
                    seed=args.seed, device_id=args.device)


if __name__ == '__main__':
  main()
