#!/usr/bin/env python3
r"""Scores segmentations against ground truth on one MI355X.

The reference's manual ends with "evaluate the resulting segmentations using
metrics of interest ... we recommend skeleton metrics" and leaves the code to
the user.  This is that step: every named segmentation of one volume (the
outputs of run_inference.py for several checkpoints, say) is scored against
the same ground truth, and optionally against ground-truth skeletons, into one
JSON file -- the numbers a checkpoint is picked by.  The per-voxel and per-node
work are HIP kernels (ffn_amd/metrics.py; there is no CPU fallback).

  python evaluate_segmentation.py --groundtruth gt.npy \
      --segmentation ckpt_a:results/a --segmentation ckpt_b:results/b \
      --corner 0,0,0 --skeletons skel.npz --core 16,16,16:234,234,234 \
      --output scores.json

A segmentation is `<name>:<file>.npy` or `<name>:<segmentation_output_dir>`,
the latter read at --corner (z,y,x) as inference wrote it.  --skeletons is an
.npz with `nodes_zyx` (n, 3), `node_skeleton` (n,), `edges` (e, 2) and
`voxel_size_zyx`.  --core z0,y0,x0:z1,y1,x1 scores that half-open box only and
leaves a margin out.  Ground-truth voxels with id 0 are unlabelled and count
nowhere.  --output gets one JSON object per name: `voxels` (Rand precision /
recall, adapted Rand error, variation of information, split / missed / merging
counts, mean best IoU) and, with skeletons, `skeletons` (edge classes, expected
run length); the per-object tables only with --per_object.
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

from ffn_amd import metrics  # noqa: E402

_SPEC = 'a segmentation is <name>:<file>.npy or <name>:<output dir>.  Got: %s'


def split_segmentation_spec(spec):
  """-> (name, path)."""
  name, sep, path = spec.partition(':')
  if not sep or not name or not path:
    raise ValueError(_SPEC % spec)
  return name, path


def _zyx(text):
  values = tuple(int(v) for v in text.split(','))
  if len(values) != 3:
    raise argparse.ArgumentTypeError('expected z,y,x, got %s' % text)
  return values


def _core(text):
  lo, sep, hi = text.partition(':')
  if not sep:
    raise argparse.ArgumentTypeError('expected z0,y0,x0:z1,y1,x1, got %s' % text)
  return _zyx(lo), _zyx(hi)


def load_segmentation(path, corner):
  """-> integer zyx array."""
  if path.endswith('.npy'):
    return np.load(path)
  if corner is None:
    raise ValueError('%s is a directory: --corner is needed' % path)
  from ffn_amd.inference import storage  # pylint:disable=g-import-not-at-top
  seg, _ = storage.load_segmentation(path, corner)
  return seg


def parse_args(argv=None):
  ap = argparse.ArgumentParser(
      description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument('--groundtruth', required=True,
                  help='.npy label volume (zyx); id 0 is unlabelled')
  ap.add_argument('--segmentation', required=True, action='append',
                  help='<name>:<file>.npy or <name>:<segmentation_output_dir>; '
                  'may be given several times')
  ap.add_argument('--corner', type=_zyx, default=None,
                  help='z,y,x corner of the subvolume in an output directory')
  ap.add_argument('--skeletons', default=None,
                  help='.npz with nodes_zyx, node_skeleton, edges, '
                  'voxel_size_zyx')
  ap.add_argument('--core', type=_core, default=None,
                  help='z0,y0,x0:z1,y1,x1: score this half-open box only')
  ap.add_argument('--background', default='segment',
                  choices=('segment', 'singletons'),
                  help="segment id 0 as one segment, or every voxel of it as a "
                  'segment of its own')
  ap.add_argument('--min_overlap', type=int, default=1,
                  help='voxels an object and a segment share to count as a '
                  'piece')
  ap.add_argument('--merge_min_nodes', type=int, default=2,
                  help='nodes each of two skeletons needs in a segment for it '
                  'to be a merger')
  ap.add_argument('--per_object', action='store_true',
                  help='also write the per-object and per-segment tables')
  ap.add_argument('--device', type=int, default=0)
  ap.add_argument('--output', default=None, help='JSON file to write')
  args = ap.parse_args(argv)
  names = [split_segmentation_spec(s)[0] for s in args.segmentation]
  if len(set(names)) != len(names):
    ap.error('--segmentation names must differ: %s' % names)
  return args


def score(ops, gt, seg, skeletons, args):
  """One segmentation -> JSON-ready dict."""
  table = ops.contingency(gt, seg, core=args.core)
  out = {'voxels': metrics.to_json(
      metrics.segmentation_scores(table, args.background, args.min_overlap),
      args.per_object)}
  if skeletons is not None:
    edges = ops.skeleton_edges(seg, skeletons, args.merge_min_nodes,
                               core=args.core)
    out['skeletons'] = metrics.to_json(metrics.skeleton_scores(edges))
    out['skeletons']['mergers'] = [int(v) for v in edges.mergers]
  return out


def main(argv=None):
  args = parse_args(argv)
  logging.basicConfig(level=logging.INFO)
  gt = np.load(args.groundtruth)
  skeletons = None
  if args.skeletons:
    with np.load(args.skeletons) as f:
      skeletons = metrics.Skeletons(f['nodes_zyx'], f['node_skeleton'],
                                    f['edges'], f['voxel_size_zyx'])
  ops = metrics.default_ops(args.device)
  result = {}
  for spec in args.segmentation:
    name, path = split_segmentation_spec(spec)
    seg = load_segmentation(path, args.corner)
    if seg.shape != gt.shape:
      raise ValueError('segmentation %s has shape %r, the ground truth %r' %
                       (name, seg.shape, gt.shape))
    result[name] = score(ops, gt, seg, skeletons, args)
    v = result[name]['voxels']
    logging.info('%s: adapted Rand error %.6f, VI split %.6f merge %.6f, '
                 'mean best IoU %.6f', name, v['adapted_rand_error'],
                 v['vi_split'], v['vi_merge'], v['mean_best_iou'])
    if skeletons is not None:
      logging.info('%s: expected run length %.3f', name,
                   result[name]['skeletons']['expected_run_length'])
  if args.output:
    with open(args.output, 'w') as f:
      json.dump(result, f, indent=1, sort_keys=True)
  return result


if __name__ == '__main__':
  main()
