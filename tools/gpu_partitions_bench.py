#!/usr/bin/env python3
"""Times of the partition kernels (HIP events inside the library) against the
HBM peak, the end-to-end call with its copies, and the reference's per-label
algorithm in numpy on the same host.

  python tools/gpu_partitions_bench.py [--size 250] [--radius 16 24]
                                       [--repeats 5] [--crop 128]

The volume is a seeded Voronoi label volume of about size^3 / 62500 labels
(250 at 250^3; the decision unit's nearest-segment expansion labels it), uint64
ids, with the 12 thresholds of the reference's sample invocation.  Per radius:
one warm-up call, then `repeats` calls; median and min..max of the device-event
time of the compute stage (keep flags, relabelling, counting kernel), its
algorithmic bytes (input labels + one output byte per voxel) and the share of
the HBM rate they amount to, the wall time of the whole call, and the number of
distinct labels among the centres of a tile.  Then, on a crop^3 corner of the
volume at the first radius: the device result must equal the per-label
algorithm in numpy (tests/partitions_ref.per_label_restatement: box sums over
the whole crop once per label, as the reference does it, through separable
prefix sums and the class table), and both are timed: the device call as the
median of `repeats` calls after a warm-up, the numpy run once.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd import decision  # noqa: E402
from ffn_amd import partitions  # noqa: E402
from tests import partitions_ref  # noqa: E402

HBM_SPEC = 8.0e12      # bytes / s, MI355X data sheet
HBM_MEASURED = 6.29e12  # streaming copy on this part
SAMPLE12 = [0.025, 0.05, 0.075, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]


def stats(values):
  values = sorted(values)
  return values[len(values) // 2], values[0], values[-1]


def voronoi_volume(n, seed):
  rng = np.random.RandomState(seed)
  count = max(n ** 3 // 62500, 2)
  points = np.zeros((n, n, n), np.uint32)
  points[tuple(rng.randint(0, n, size=(3, count)))] = np.arange(
      1, count + 1, dtype=np.uint32)
  seg, _ = decision.default_ops(0).watershed_expand(points, (1, 1, 1))
  return seg.astype(np.uint64) * np.uint64(7) + np.uint64(3)


def tile_of(radius):
  """(tz, ty, tx) as choose_tile of csrc/ffn_partitions.hip picks it."""
  h = 8 + 2 * radius
  return (8, 8 if h * h * 16 + h * 8 * 128 <= 78 * 1024 else 4, 64)


def labels_per_tile(seg, radius, min_size):
  """Distinct labels among a tile's centres after dust removal, background
  not counted: the rounds lom_count_kernel runs for that tile."""
  seg = partitions_ref.background_cleared(seg, None, min_size)
  r = radius
  centre = seg[r:seg.shape[0] - r, r:seg.shape[1] - r, r:seg.shape[2] - r]
  tz, ty, tx = tile_of(radius)
  found = []
  for z in range(0, centre.shape[0], tz):
    for y in range(0, centre.shape[1], ty):
      for x in range(0, centre.shape[2], tx):
        tile = centre[z:z + tz, y:y + ty, x:x + tx]
        found.append(len(np.unique(tile[tile > 0])))
  return float(np.mean(found)), int(np.max(found)), len(found)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=250)
  ap.add_argument('--radius', type=int, nargs='+', default=[16, 24])
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--crop', type=int, default=128)
  ap.add_argument('--min-size', type=int, default=10000)
  args = ap.parse_args()
  ops = partitions.default_ops(0)
  n = args.size
  seg = voronoi_volume(n, seed=n)
  print('%d^3 Voronoi volume: %d labels, uint64 ids, 12 thresholds, min_size %d'
        % (n, len(np.unique(seg)), args.min_size))
  for radius in args.radius:
    lom = (radius,) * 3
    ms, wall = [], []
    for r in range(args.repeats + 1):  # the first call is the warm-up
      t0 = time.time()
      out = ops.compute(seg, SAMPLE12, lom, min_size=args.min_size)
      t1 = time.time()
      (m0, _), (m1, nbytes) = ops.last_timing()
      if r:
        ms.append(m1)
        wall.append(t1 - t0)
    med, lo, hi = stats(ms)
    rate = nbytes / (med * 1e-3)
    mean_l, max_l, tiles = labels_per_tile(seg, radius, args.min_size)
    print('  radius %d: output %s, tile %s, %d tiles, labels per tile mean %.2f '
          'max %d' % (radius, out.shape, tile_of(radius), tiles, mean_l, max_l))
    print('    compute kernels  median %8.3f ms (min %.3f, max %.3f, n=%d)  '
          '%6.1f MB algorithmic  %7.1f GB/s = %4.1f %% of 8.0 TB/s spec, '
          '%4.1f %% of 6.29 TB/s measured' % (
              med, lo, hi, len(ms), nbytes / 1e6, rate / 1e9,
              100 * rate / HBM_SPEC, 100 * rate / HBM_MEASURED))
    print('    label sizes kernel %.3f ms; whole call (upload, sizes, kernels, '
          'partitions + histogram back) median %.3f s (min %.3f, max %.3f)' % (
              (m0,) + stats(wall)))
    sys.stdout.flush()
  radius, c = args.radius[0], args.crop
  crop = np.ascontiguousarray(seg[:c, :c, :c])
  lom = (radius,) * 3
  t_devs = []
  for r in range(args.repeats + 1):  # the first call is the warm-up
    t0 = time.time()
    got = ops.compute(crop, SAMPLE12, lom, min_size=args.min_size)
    if r:
      t_devs.append(time.time() - t0)
  t_dev, t_dev_lo, t_dev_hi = stats(t_devs)
  t0 = time.time()
  want = partitions_ref.per_label_restatement(crop, SAMPLE12, lom,
                                              args.min_size)
  t_cpu = time.time() - t0
  same = got.shape == want.shape and got.tobytes() == want.tobytes()
  print('  %d^3 crop, radius %d, %d labels: device call median %.4f s (min '
        '%.4f, max %.4f, n=%d), per-label prefix sums in numpy on this host, '
        'one run, %.2f s (%.0f x); results %s' % (
            c, radius, len(np.unique(crop)), t_dev, t_dev_lo, t_dev_hi,
            len(t_devs), t_cpu, t_cpu / t_dev,
            'identical' if same else 'DIFFER'))
  if not same or not t_dev < t_cpu:
    sys.exit(1)


if __name__ == '__main__':
  main()
