#!/usr/bin/env python3
"""Kernel-only rates of the metric kernels (HIP events inside the library)
beside the host numpy specification and ffn_labels_pair_counts.

  python tools/gpu_metrics_bench.py [--size 250 512] [--nodes 1000000]

Volumes: two Voronoi label volumes (cells of a grid 8 times coarser, repeated,
the segmentation shifted off that grid; 8 % of the ground truth unlabelled).
Per size: ffn_metrics_contingency on uint64 ground truth x int32 segmentation
(whole and with a core 16 voxels in), the same two volumes as uint32 with no
box and nothing ignored beside ffn_labels_pair_counts (the same memory
traffic), the wall time of tests/metrics_ref.py's np.unique on this host, and
ffn_metrics_skeleton for --nodes random-walk nodes.  The HBM fraction is
algorithmic bytes / kernel time over the 8 TB/s of an MI355X.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd import labels, metrics  # noqa: E402
from tests import metrics_ref  # noqa: E402
from tests.partitions_ref import voronoi_labels  # noqa: E402

HBM_GBS = 8000.0


def volumes(n, seed=1):
  c = -(-n // 8)
  up = lambda v: v.repeat(8, 0).repeat(8, 1).repeat(8, 2)[:n, :n, :n]
  gt = np.ascontiguousarray(up(voronoi_labels((c, c, c), 200, seed)))
  seg = np.roll(up(voronoi_labels((c, c, c), 300, seed + 1, dtype=np.int32)),
                (1, 2, 3), (0, 1, 2))
  rng = np.random.RandomState(seed)
  gt.reshape(-1)[rng.randint(0, gt.size, gt.size // 12)] = 0
  return gt, np.ascontiguousarray(seg)


def best(fn, timing, repeats=5):
  """min kernel ms over `repeats` calls (the first one also sizes tables)."""
  out = []
  for _ in range(repeats + 1):
    fn()
    out.append(timing())
  return min(ms for ms, _ in out[1:]), out[-1][1]


def report(what, ms, nbytes, extra=''):
  gbs = nbytes / ms / 1e6
  print('%s: %.3f ms, %.0f GB/s algorithmic = %.0f %% of HBM%s' %
        (what, ms, gbs, 100 * gbs / HBM_GBS, extra))


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, nargs='+', default=[250, 512])
  ap.add_argument('--nodes', type=int, default=1000000)
  ap.add_argument('--no-host', action='store_true',
                  help='skip the numpy specification timings')
  args = ap.parse_args()
  ops = metrics.default_ops(0)
  lops = labels.default_ops(0)
  for n in args.size:
    gt, seg = volumes(n)
    core = ((16,) * 3, (n - 16,) * 3)
    table = ops.contingency(gt, seg)
    print('%d^3: %d pairs' % (n, len(table.counts)))
    ms, nb = best(lambda: ops.contingency(gt, seg), ops.last_timing)
    report('%d^3 u64 x i32 contingency, gt 0 ignored' % n, ms, nb)
    ms, nb = best(lambda: ops.contingency(gt, seg, core=core), ops.last_timing)
    report('%d^3 u64 x i32 contingency, core 16 in' % n, ms, nb)
    a, b = gt.astype(np.uint32), seg.astype(np.uint32)
    ms, nb = best(lambda: ops.contingency(a, b, ignore_gt_zero=False),
                  ops.last_timing)
    report('%d^3 u32 x u32 contingency, nothing ignored' % n, ms, nb)
    ms2, nb2 = best(lambda: lops.pair_counts(a, b), lops.last_timing)
    report('%d^3 u32 x u32 ffn_labels_pair_counts' % n, ms2, nb2,
           ' (contingency / pair_counts = %.3f)' % (ms / ms2))
    if not args.no_host:
      t0 = time.time()
      want = metrics_ref.contingency(gt, seg)
      print('%d^3 numpy specification (np.unique): %.2f s wall; tables equal: %s'
            % (n, time.time() - t0,
               all(np.array_equal(x, y) for x, y in zip(table, want))))
    if n == args.size[-1] and args.nodes:
      per = 1000
      nodes, skel, edges = metrics_ref.random_walk_skeletons(
          gt.shape, args.nodes // per, per, 3)
      sk = metrics.Skeletons(nodes, skel, edges, (4.0, 1.0, 1.0))
      got = ops.skeleton_edges(seg, sk)
      ms, nb = best(lambda: ops.skeleton_edges(seg, sk), ops.last_timing, 3)
      report('%d nodes, %d edges on %d^3 skeleton (%d runs, %d mergers)' %
             (len(nodes), len(edges), n, len(got.run_lengths),
              len(got.mergers)), ms, nb)
      if not args.no_host:
        length = metrics_ref.edge_lengths_q(nodes, edges, sk.voxel_size_zyx)
        t0 = time.time()
        want = metrics_ref.skeleton_edges(seg, nodes, skel, edges, length)
        print('numpy / Python specification: %.2f s wall; classes equal: %s' %
              (time.time() - t0,
               np.array_equal(got.edge_class, want['edge_class'])))


if __name__ == '__main__':
  main()
