#!/usr/bin/env python3
"""Stage times of the decision point kernels (HIP events inside the library)
against the HBM peak, and the wall time of a CPU path on the same host.

  python tools/gpu_decision_bench.py [--size 250 512] [--repeats 7]
                                     [--cpu-size 250] [--voxel-size 8 8 33]

Per size: a seeded segmentation of convex cells with oblique faces and gaps of
about four voxels between them (uint64 ids), one warm-up call, then `repeats`
calls; median and min..max of the
device-event time of each stage, its algorithmic bytes and the rate those
give.  The CPU path (sizes in --cpu-size, where scipy imports) is scipy's
feature transform plus the numpy candidate / minimum / selection steps of
tests/decision_ref.py: the work of the reference's function without pandas.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd import decision  # noqa: E402
from ffn_amd.utils import decision_point  # noqa: E402
from tests import decision_ref  # noqa: E402

HBM_SPEC = 8.0e12      # bytes / s, MI355X data sheet
HBM_MEASURED = 6.29e12  # streaming copy on this part


def stats(values):
  values = sorted(values)
  return values[len(values) // 2], values[0], values[-1]


def cells_segmentation(ops, n, seed, cell=20):
  """Voronoi cells of (n / cell)^3 random points (the expansion kernel itself
  labels them), with every voxel within two steps of another cell unlabelled."""
  rng = np.random.RandomState(seed)
  count = max(int((n / float(cell)) ** 3), 2)
  points = np.zeros((n, n, n), np.uint32)
  points[tuple(rng.randint(0, n, size=(3, count)))] = np.arange(
      1, count + 1, dtype=np.uint32)
  seg, _ = ops.watershed_expand(points, (1, 1, 1))
  for _ in range(2):
    edge = np.zeros(seg.shape, bool)
    for axis in range(3):
      a = [slice(None)] * 3
      b = [slice(None)] * 3
      a[axis], b[axis] = slice(0, -1), slice(1, None)
      diff = seg[tuple(a)] != seg[tuple(b)]
      edge[tuple(a)] |= diff
      edge[tuple(b)] |= diff
    seg[edge] = 0
  return seg.astype(np.uint64) * np.uint64(7) + np.uint64(seg.size) * (seg > 0)


def cpu_path(seg, voxel_size, max_distance):
  from scipy import ndimage  # pylint:disable=g-import-not-at-top
  t0 = time.time()
  edt, idx = ndimage.distance_transform_edt(
      seg == 0, sampling=tuple(voxel_size)[::-1], return_indices=True)
  expanded = seg[tuple(idx)]
  if max_distance is not None:
    expanded[edt > max_distance] = 0
  t1 = time.time()
  points = decision_ref.select_spec(decision_ref.minimising_spec(
      decision_ref.candidates_spec(expanded, edt)))
  return t1 - t0, time.time() - t1, len(points)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, nargs='+', default=[250, 512])
  ap.add_argument('--repeats', type=int, default=7)
  ap.add_argument('--cpu-size', type=int, nargs='*', default=[250])
  ap.add_argument('--voxel-size', type=float, nargs=3, default=[8, 8, 33])
  ap.add_argument('--max-distance', type=float, default=None)
  args = ap.parse_args()
  ops = decision.default_ops(0)
  voxel = tuple(args.voxel_size)
  for n in args.size:
    seg = cells_segmentation(ops, n, seed=n)
    print('%d^3: %d ids, %.0f %% labelled, voxel size %s, max_distance %s' % (
        n, len(np.unique(seg)) - 1, 100.0 * np.mean(seg > 0), voxel,
        args.max_distance))
    ms = [[], []]
    nbytes = [0.0, 0.0]
    for r in range(args.repeats + 1):  # the first call is the warm-up
      ops.expand(seg, voxel, args.max_distance)
      cands = ops.contact_minima()
      (m0, b0), (m1, b1) = ops.last_timing()
      if r:
        ms[0].append(m0)
        ms[1].append(m1)
      nbytes = [b0, b1]
    for k, name in enumerate(('expand (x, y, z passes)',
                              'contact scan + per-pair minimum + emit')):
      med, lo, hi = stats(ms[k])
      rate = nbytes[k] / (med * 1e-3)
      print('  %-40s median %8.3f ms (min %.3f, max %.3f, n=%d)  %6.1f MB '
            'algorithmic  %7.1f GB/s = %4.1f %% of 8.0 TB/s spec, %4.1f %% of '
            '6.29 TB/s measured' % (name, med, lo, hi, len(ms[k]),
                                    nbytes[k] / 1e6, rate / 1e9,
                                    100 * rate / HBM_SPEC,
                                    100 * rate / HBM_MEASURED))
    t0 = time.time()
    points = decision_point.find_decision_points(seg, voxel, args.max_distance)
    wall = time.time() - t0
    print('  find_decision_points wall (upload, kernels, %d candidates back, '
          'host selection): %.3f s, %d pairs' % (len(cands['a']), wall,
                                                 len(points)))
    if n in args.cpu_size:
      try:
        t_edt, t_sel, n_cpu = cpu_path(seg, voxel, args.max_distance)
        print('  CPU path on this host: scipy feature transform %.2f s + numpy '
              'candidates / minimum / selection %.2f s = %.2f s, %d pairs' % (
                  t_edt, t_sel, t_edt + t_sel, n_cpu))
      except ImportError:
        print('  CPU path: scipy not importable, skipped')
    sys.stdout.flush()


if __name__ == '__main__':
  main()
