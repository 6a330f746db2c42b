#!/usr/bin/env python3
r"""Partition map of a label volume on one MI355X (classes of local label share).

Drop-in for the reference's compute_partitions.py: the same flags and the same
result.  Each labelled voxel is the centre of a box of `lom_radius` voxels to
every side (the local object mask, LOM); the share of that box that carries
the centre's own label is sorted into the classes that `thresholds` bound, and
the class is what the map stores.  The counting is done by the HIP kernels
behind ffn_amd/partitions.py (there is no CPU fallback).

  python compute_partitions.py --min_size 10000 --lom_radius 16,16,16 \
      --thresholds 0.025,0.05,0.075,0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9 \
      --input_volume proofread.npy --output_volume proofread_partitions.npz

Volumes are `<file>.npy`, or `<file>.h5:<dataset>` where h5py is installed.
An HDF5 output is written as the reference writes it (a uint8 dataset of the
input's shape, 255 outside the valid region, with the attributes
`bounding_boxes` and `partition_counts`); an `.npz` output holds the arrays
`partitions`, `bounding_boxes` and `partition_counts` instead.

Two flags are read differently from the reference, whose flag plumbing hands
`compute_partitions` lists of strings that can never match anything:
`--id_whitelist` is parsed as integers (the reference intersects a set of
strings with integer labels, which is always empty), and
`--exclusion_regions` as groups of four numbers x,y,z,r (the reference unpacks
each single string as a 4-tuple, which raises).
"""

import argparse
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from ffn_amd import partitions as partition_ops  # noqa: E402
from ffn_amd.inference import request as req_lib  # noqa: E402
from ffn_amd.inference import storage  # noqa: E402

_NO_H5PY = ('h5py is not available in this environment; convert the volume to '
            '.npy and use `image { npy: "..." }`')


def load_mask(mask_configs, shape_zyx):
  """Boolean exclusion mask of the whole input volume (None without configs);
  the reference's load_mask up to the box query, which the device does."""
  if mask_configs is None:
    return None
  return storage.build_mask(mask_configs.masks, (0, 0, 0), tuple(shape_zyx))


def compute_partitions(seg_array,
                       thresholds,
                       lom_radius,
                       id_whitelist=None,
                       exclusion_regions=None,
                       mask_configs=None,
                       min_size=10000,
                       device_id=0):
  """Partition map of `seg_array` with the reference's argument order and
  return value; the definition is in ffn_amd.partitions.PartitionOps.compute.

  seg_array is a 3-d integer volume (zyx) and is not modified.  thresholds are
  the class bounds on the own-label share of the LOM box, lom_radius its half
  widths as (x, y, z).  With id_whitelist only the listed ids get classes.
  Output voxels inside a sphere (x, y, z, r) of exclusion_regions (input
  coordinates, voxels), and those whose box touches a voxel that the
  MaskConfigs message mask_configs masks, hold 255.  Labels smaller than
  min_size voxels count as background.

  Returns (lom_radius as an array, i.e. the xyz corner of the output inside
  the input; the uint8 map of the valid region).
  """
  seg_array = np.asarray(seg_array)
  mask = None
  if mask_configs is not None and seg_array.ndim == 3:
    mask = load_mask(mask_configs, seg_array.shape)
  ops = partition_ops.default_ops(device_id)
  output = ops.compute(seg_array, thresholds, lom_radius,
                       id_whitelist=id_whitelist,
                       exclusion_regions=exclusion_regions, mask=mask,
                       min_size=min_size)
  logging.info('%d of %d output voxels carry a class or 255',
               np.count_nonzero(output), output.size)
  return np.array(lom_radius), output


def adjust_bboxes(bboxes, lom_radius):
  """Shrinks (start, size) xyz boxes by the LOM radius on every side and drops
  the ones that vanish."""
  margin = np.asarray(lom_radius)
  shrunk = [(np.asarray(start) + margin, np.asarray(size) - 2 * margin)
            for start, size in bboxes]
  return [(start, size) for start, size in shrunk if size.min() > 0]


def _split_volume_path(path, plain_suffix):
  """'<file><plain_suffix>' -> (file, None); '<file>:<dataset>' -> (file,
  dataset).  The suffix is '.npy' for the input and '.npz' for the output."""
  if path.endswith(plain_suffix):
    return path, None
  parts = path.split(':')
  if len(parts) != 2 or path.endswith(('.npy', '.npz')):
    raise ValueError('volume should be <file>%s or <hdf5 file>:<dataset>.  '
                     'Got: %s' % (plain_suffix, path))
  return parts[0], parts[1]


def _h5py():
  try:
    import h5py  # pylint:disable=g-import-not-at-top
  except ImportError as e:
    raise NotImplementedError(_NO_H5PY) from e
  return h5py


def load_volume(path):
  """Returns (label array, list of (start, size) xyz bounding boxes)."""
  filename, dataset = _split_volume_path(path, '.npy')
  bboxes = []
  if dataset is None:
    seg = np.load(filename)
  else:
    with _h5py().File(filename, 'r') as f:
      volume = f[dataset]
      # every attribute named bounding_boxes* is a list of (start, size) pairs
      keys = sorted(k for k in volume.attrs if k.startswith('bounding_boxes'))
      for key in keys:
        pairs = np.asarray(volume.attrs[key]).reshape(-1, 2, 3)
        bboxes.extend((pair[0], pair[1]) for pair in pairs)
      seg = volume[...]
  whole = (np.zeros(3, np.int64), np.array(seg.shape[::-1]))
  return seg, bboxes or [whole]


def save_volume(path, shape, corner, partitions, bboxes, partition_counts):
  filename, dataset = _split_volume_path(path, '.npz')
  # corner is xyz, the arrays are zyx
  sel = tuple(slice(int(c), int(c) + n)
              for c, n in zip(tuple(corner)[::-1], partitions.shape))
  boxes = np.array([(b[0], b[1]) for b in bboxes],
                   np.int64).reshape(-1, 2, 3)
  if dataset is None:
    full = np.full(shape, 255, np.uint8)
    full[sel] = partitions
    np.savez_compressed(filename, partitions=full, bounding_boxes=boxes,
                        partition_counts=partition_counts)
    return
  with _h5py().File(filename, 'w') as f:
    # unwritten chunks read back as 255: only the valid region is stored
    layout = dict(shape=tuple(shape), dtype='u1', fillvalue=255, chunks=True,
                  compression='gzip')
    out = f.create_dataset(dataset, **layout)
    out[sel] = partitions
    out.attrs.create('bounding_boxes', data=boxes)
    out.attrs.create('partition_counts', data=partition_counts)


def _csv(convert):
  return lambda text: [convert(v) for v in text.split(',') if v.strip()]


def main(argv=None):
  ap = argparse.ArgumentParser(
      description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--input_volume', required=True,
                  help='labels to partition: <file>.npy, or <file>:<dataset> '
                  'of an HDF5 file')
  ap.add_argument('--output_volume', required=True,
                  help='destination of the map: <file>.npz, or '
                  '<file>:<dataset> of an HDF5 file (overwritten)')
  ap.add_argument('--thresholds', required=True, type=_csv(float),
                  help='comma-separated class bounds on the own-label share '
                  'of the LOM box')
  ap.add_argument('--lom_radius', required=True, type=_csv(int),
                  help='x,y,z half widths of the LOM box in voxels')
  ap.add_argument('--id_whitelist', default=None, type=_csv(int),
                  help='comma-separated ids; all other labels are treated as '
                  'background')
  ap.add_argument('--exclusion_regions', default=None, type=_csv(float),
                  help='x,y,z,r[,x,y,z,r...]: spheres in input coordinates '
                  'whose voxels get 255')
  ap.add_argument('--mask_configs', default=None,
                  help='text-format MaskConfigs message; a voxel whose LOM '
                  'box touches the mask gets 255')
  ap.add_argument('--min_size', type=int, default=10000,
                  help='labels of fewer voxels are background (default '
                  '%(default)s)')
  ap.add_argument('--device', type=int, default=0)
  args = ap.parse_args(argv)
  logging.basicConfig(level=logging.INFO)

  exclusion_regions = None
  if args.exclusion_regions is not None:
    if len(args.exclusion_regions) % 4:
      ap.error('--exclusion_regions takes groups of four numbers x,y,z,r')
    exclusion_regions = [tuple(args.exclusion_regions[i:i + 4])
                         for i in range(0, len(args.exclusion_regions), 4)]
  mask_configs = None
  if args.mask_configs:
    mask_configs = req_lib.parse_text(args.mask_configs, req_lib.MaskConfigs())
  if len(args.lom_radius) != 3:
    ap.error('--lom_radius takes three integers x,y,z')

  seg, bboxes = load_volume(args.input_volume)
  corner, partitions = compute_partitions(
      seg, args.thresholds, args.lom_radius, args.id_whitelist,
      exclusion_regions, mask_configs, args.min_size, device_id=args.device)
  counts = partition_ops.default_ops(args.device).partition_counts()
  bboxes = adjust_bboxes(bboxes, np.array(args.lom_radius))
  save_volume(args.output_volume, seg.shape, corner, partitions, bboxes, counts)


if __name__ == '__main__':
  main()
