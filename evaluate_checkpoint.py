#!/usr/bin/env python3
r"""Scores a checkpoint on training examples on one MI355X.

The reference reports how good a network is only while it trains: the `eval/*`
and `moves/*` summaries of ffn/training/tracker.py.  This runs the same FoV
loop forward-only: for every coordinate of a TFRecord file written by
build_coordinates.py it loads the example as train.py does (without
augmentation), moves the FoV by the chosen policy, and accumulates the
tracker's numbers.  The voxel work and the network are HIP kernels (there is
no CPU fallback); the flags it shares with train.py mean what they mean there.

  python evaluate_checkpoint.py --train_coords tf_record_file \
      --data_volumes validation1:grayscale.npy \
      --label_volumes validation1:groundtruth.npy \
      --model_name convstack_3d.ConvStack3DFFNModel \
      --model_args '{"depth": 12, "fov_size": [33, 33, 33], "deltas": [8, 8, 8]}' \
      --checkpoint model.ckpt-27465036 --image_mean 128 --image_stddev 33 \
      --output scores.json

A volume is `<name>:<file>.npy`, `<name>:<file>.npz:<array>`, or
`<name>:<file>:<dataset>` of an HDF5 file where h5py is installed.  Images are
uint8 or float32, labels 4- or 8-byte integers.  Coordinates whose patches
leave their volume are skipped and counted.  `--output` gets a JSON object
with `summaries` (the reference's tags), the raw `accumulators`, and the
numbers of examples run and skipped.

train.py shuffles the moves of the 'fixed' policy with Python's unseeded
`random` when --shuffle_moves is set; here they are tried in model.shifts order
unless --shuffle_seed is given, which shuffles them with random.Random(seed).
"""

import argparse
import json
import logging
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

from ffn_amd import coordinates as coordinate_ops  # noqa: E402
from ffn_amd.training import evaluation  # noqa: E402
from ffn_amd.training.import_util import import_symbol  # noqa: E402

_NO_H5PY = ('h5py is not available in this environment; convert the volume to '
            '.npy and pass `<name>:<file>.npy`')
_SPEC = ('a volume is <name>:<file>.npy, <name>:<file>.npz:<array> or '
         '<name>:<hdf5 file>:<dataset>.  Got: %s')


def split_volume_spec(spec):
  """-> (name, file, array / dataset or None for .npy)."""
  parts = spec.split(':')
  if len(parts) < 2 or not parts[0] or not parts[1]:
    raise ValueError(_SPEC % spec)
  name, filename, rest = parts[0], parts[1], parts[2:]
  if filename.endswith('.npy'):
    if rest:
      raise ValueError(_SPEC % spec)
    return name, filename, None
  if len(rest) == 1 and rest[0]:
    return name, filename, rest[0]
  raise ValueError(_SPEC % spec)


def _h5py():
  try:
    import h5py  # pylint:disable=g-import-not-at-top
  except ImportError as e:
    raise NotImplementedError(_NO_H5PY) from e
  return h5py


def load_volume(spec):
  """Returns (name, array zyx)."""
  name, filename, key = split_volume_spec(spec)
  if filename.endswith('.npy'):
    return name, np.load(filename)
  if filename.endswith('.npz'):
    with np.load(filename) as f:
      return name, f[key]
  with _h5py().File(filename, 'r') as f:
    return name, f[key][...]


def offset_scale_map(entries):
  """train.py:182-191: '<name>:<offset>:<scale>' entries -> {name: (offset,
  scale)}."""
  out = {}
  for entry in entries or ():
    parts = entry.split(':')
    if len(parts) != 3:
      raise ValueError('expected <volume>:<offset>:<scale>, got %s' % entry)
    out[parts[0]] = (float(parts[1]), float(parts[2]))
  return out


def _csv(text):
  return [v for v in text.split(',') if v.strip()]


def parse_args(argv=None):
  ap = argparse.ArgumentParser(
      description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--train_coords', required=True,
                  help='TFRecord file of coordinates (GZIP or plain), as '
                  'build_coordinates.py writes it')
  ap.add_argument('--data_volumes', required=True, type=_csv,
                  help='comma-separated image volumes, <name>:<file>...')
  ap.add_argument('--label_volumes', required=True, type=_csv,
                  help='comma-separated label volumes under the same names')
  ap.add_argument('--model_name', default='convstack_3d.ConvStack3DFFNModel')
  ap.add_argument('--model_args', required=True, type=json.loads,
                  help='JSON arguments of the model class')
  ap.add_argument('--checkpoint', required=True,
                  help='TF checkpoint prefix, or an .npz keyed by variable name')
  ap.add_argument('--batch_size', type=int, default=4)
  ap.add_argument('--fov_policy', default='fixed', choices=evaluation.POLICIES)
  ap.add_argument('--fov_moves', type=int, default=1)
  ap.add_argument('--threshold', type=float, default=0.9)
  ap.add_argument('--seed_pad', type=float, default=0.05)
  ap.add_argument('--image_mean', type=float, default=None)
  ap.add_argument('--image_stddev', type=float, default=None)
  ap.add_argument('--image_offset_scale_map', type=_csv, default=None,
                  help='comma-separated <volume>:<offset>:<scale>; volumes not '
                  'named use --image_mean / --image_stddev')
  ap.add_argument('--max_examples', type=int, default=None)
  ap.add_argument('--shuffle_seed', type=int, default=None,
                  help="shuffles the 'fixed' policy's moves (default: "
                  'model.shifts order)')
  ap.add_argument('--device', type=int, default=0)
  ap.add_argument('--output', default=None, help='JSON file to write')
  args = ap.parse_args(argv)
  if ((args.image_stddev is None or args.image_mean is None) and
      not args.image_offset_scale_map):
    ap.error('--image_mean, --image_stddev or --image_offset_scale_map need to '
             'be defined')
  if not 1 <= args.batch_size <= evaluation.MAX_SLOTS:
    ap.error('--batch_size must be in [1, %d]' % evaluation.MAX_SLOTS)
  return args


def make_backend(args, model):
  """-> (model, engine, ops) on the device."""
  from ffn_amd import engine as hip_engine  # pylint:disable=g-import-not-at-top
  model.load_checkpoint(args.checkpoint)
  eng = hip_engine.HipEngine.from_model(model, max_batch=args.batch_size,
                                        device_id=args.device)
  return model, eng, evaluation.default_ops(args.device)


def main(argv=None):
  args = parse_args(argv)
  logging.basicConfig(level=logging.INFO)
  images = dict(load_volume(spec) for spec in args.data_volumes)
  labels = dict(load_volume(spec) for spec in args.label_volumes)
  if set(images) != set(labels):
    raise ValueError('image volumes %r and label volumes %r differ' %
                     (sorted(images), sorted(labels)))
  scales = offset_scale_map(args.image_offset_scale_map)
  model = import_symbol(args.model_name)(**args.model_args)
  model, engine, ops = make_backend(args, model)
  ev = evaluation.CheckpointEvaluator(
      model, engine, ops, args.fov_policy, args.fov_moves,
      threshold=args.threshold, seed_pad=args.seed_pad,
      batch_size=args.batch_size, shuffle_seed=args.shuffle_seed)
  for name in sorted(images):
    offset, scale = scales.get(name, (args.image_mean, args.image_stddev))
    if offset is None or scale is None:
      raise ValueError('no offset and scale for volume %r' % name)
    ev.add_volume(name, images[name], labels[name], offset, scale)
  centres, names = coordinate_ops.read_tfrecord(args.train_coords)
  result = ev.evaluate(zip(centres.tolist(), names),
                       max_examples=args.max_examples)
  logging.info('%d examples, %d skipped (patch leaves the volume)',
               result.num_patches, result.skipped)
  summaries = result.summaries()
  for tag in sorted(summaries):
    logging.info(' %s: %s', tag, summaries[tag])
  if args.output:
    with open(args.output, 'w') as f:
      json.dump({'summaries': summaries,
                 'accumulators': result.accumulators(),
                 'examples': result.num_patches, 'skipped': result.skipped},
                f, indent=1, sort_keys=True)
  return result


if __name__ == '__main__':
  main()
