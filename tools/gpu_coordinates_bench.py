#!/usr/bin/env python3
"""Times of the coordinate kernels (HIP events inside the library), of the
whole build_coordinates.py run with its per-step split, and of the numpy
restatement on the same host.

  python tools/gpu_coordinates_bench.py [--size 250] [--radius 16]
      [--margin 24] [--repeats 5] [--script-repeats 5] [--crop 128]

The input is the partition map of the seeded Voronoi label volume of
tools/gpu_partitions_bench.py (250 labels at 250^3, the 12 thresholds of the
reference's sample invocation, min_size 10000) at the given LOM radius, written
as compute_partitions.py writes it: input-shaped, 255 outside the valid region.

Device calls, one warm-up then `repeats` rounds, medians with min..max: the
counting sort of the cropped map (add_volume), the gather of all output rows,
and the serialisation of the first window of 2^20 rows; for each the
device-event time of its kernels and the wall time of the call with its copies.
Then the whole script, in process (build_coordinates.main with --seed), one
warm-up then `script-repeats` runs: wall time and the split into loading the
.npz, sort, host RNG (MT19937 permutations and the shuffle), gather, reading
the rows back, serialisation and gzip.  Then, on a crop^3 block from the middle
of the map, margin 0: the device's rows must equal those of the numpy
restatement (tests/coordinates_ref.coordinates_spec) for the same seed; the
device build is timed as the median of `repeats` calls after a warm-up, the
numpy run once.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import build_coordinates  # noqa: E402
import gpu_partitions_bench  # noqa: E402
from ffn_amd import coordinates  # noqa: E402
from ffn_amd import partitions  # noqa: E402
from tests import coordinates_ref  # noqa: E402

WINDOW = coordinates.DEFAULT_WINDOW


def stats(values):
  values = sorted(values)
  return values[len(values) // 2], values[0], values[-1]


def fmt(values, scale=1.0, unit='ms'):
  med, lo, hi = stats(values)
  return '%9.3f %s (min %.3f, max %.3f, n=%d)' % (
      med * scale, unit, lo * scale, hi * scale, len(values))


def partition_map(n, radius):
  seg = gpu_partitions_bench.voronoi_volume(n, seed=n)
  part = partitions.default_ops(0).compute(
      seg, gpu_partitions_bench.SAMPLE12, (radius,) * 3, min_size=10000)
  full = np.full(seg.shape, 255, np.uint8)
  full[radius:n - radius, radius:n - radius, radius:n - radius] = part
  return full


def device_calls(ops, crop, repeats):
  rows = {'sort': ([], []), 'gather': ([], []), 'serialize': ([], [])}
  for r in range(repeats + 1):  # the first round is the warm-up
    ops.reset()
    t0 = time.time()
    counts = ops.add_volume(crop)
    t_sort = time.time() - t0
    totals = {int(c): int(counts[c]) for c in np.flatnonzero(counts[:255])}
    max_count = coordinates.check_rows(totals)
    rng = np.random.RandomState(1)
    perms = [rng.permutation(v).astype(np.uint32) for v in totals.values()]
    order = np.arange(len(totals) * max_count, dtype=np.uint32)
    rng.shuffle(order)
    t0 = time.time()
    ops.gather(list(totals), max_count, perms, order, (0, 0, 0))
    t_gather = time.time() - t0
    ops.set_names(['validation1'])
    window = min(WINDOW, ops.num_rows)
    t0 = time.time()
    data = ops.serialize(0, window)
    t_ser = time.time() - t0
    timing = ops.last_timing()
    if r:
      for key, wall, (ms, _) in zip(('sort', 'gather', 'serialize'),
                                    (t_sort, t_gather, t_ser), timing):
        rows[key][0].append(ms)
        rows[key][1].append(wall * 1e3)
  nbytes = [b for _, b in timing]
  return rows, nbytes, totals, ops.num_rows, window, len(data)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=250)
  ap.add_argument('--radius', type=int, default=16)
  ap.add_argument('--margin', type=int, default=24)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--script-repeats', type=int, default=5)
  ap.add_argument('--crop', type=int, default=128)
  args = ap.parse_args()
  ops = coordinates.default_ops(0)
  n, m = args.size, args.margin
  full = partition_map(n, args.radius)
  crop = np.ascontiguousarray(full[m:n - m, m:n - m, m:n - m])
  print('%d^3 partition map (radius %d), margin %d: crop %s, %d voxels' % (
      n, args.radius, m, crop.shape, crop.size))
  rows, nbytes, totals, n_rows, window, window_bytes = device_calls(
      ops, crop, args.repeats)
  print('  classes %s' % totals)
  print('  %d classes x max_count %d = %d rows' % (
      len(totals), max(totals.values()), n_rows))
  for key, what, b in (
      ('sort', 'add_volume (upload, histogram, scan, scatter)', nbytes[0]),
      ('gather', 'gather (upload of order and perms, kernel)', nbytes[1]),
      ('serialize', 'serialize, one window of %d rows = %d bytes (sizes, scan,'
       ' write, copy back)' % (window, window_bytes), nbytes[2])):
    ms, wall = rows[key]
    print('  %s' % what)
    print('    kernels %s  %7.1f MB algorithmic = %6.1f GB/s' % (
        fmt(ms), b / 1e6, b / (stats(ms)[0] * 1e-3) / 1e9))
    print('    call    %s' % fmt(wall))
  sys.stdout.flush()

  with tempfile.TemporaryDirectory() as tmp:
    src = os.path.join(tmp, 'partitions.npz')
    dst = os.path.join(tmp, 'coordinates')
    np.savez_compressed(src, partitions=full)
    argv = ['--partition_volumes', 'validation1:' + src, '--coordinate_output',
            dst, '--margin', '%d,%d,%d' % (m, m, m), '--seed', '1']
    walls, splits = [], []
    for r in range(args.script_repeats + 1):  # the first run is the warm-up
      t0 = time.time()
      build_coordinates.main(argv)
      wall = time.time() - t0
      if r:
        walls.append(wall)
        splits.append(dict(ops.split))
    size = os.path.getsize(dst)
  print('  whole script (build_coordinates.py --seed 1, %d rows, TFRecord of %d '
        'bytes compressed): %s' % (n_rows, size, fmt(walls, unit='s')))
  named = 0.0
  for key, what in (
      ('sort', 'sort call (crop upload + kernels)'),
      ('sort_kernels', '  of which kernels'),
      ('host_rng', 'host RNG (permutations + shuffle, MT19937)'),
      ('gather', 'gather call (order / perms upload + kernel)'),
      ('gather_kernels', '  of which kernel'),
      ('read', 'rows back to the host'),
      ('serialize', 'serialize calls (kernels + copy back), all windows'),
      ('serialize_kernels', '  of which kernels'),
      ('gzip', 'gzip (level %d) and file write' % coordinates.GZIP_LEVEL)):
    med = stats([s[key] for s in splits])[0]
    if not key.endswith('_kernels'):
      named += med
    print('    %-52s %8.3f s' % (what, med))
  print('    %-52s %8.3f s' % ('everything else (loading the .npz, logging)',
                               stats(walls)[0] - named))
  sys.stdout.flush()

  c = args.crop
  lo = (n - c) // 2
  block = np.ascontiguousarray(full[lo:lo + c, lo:lo + c, lo:lo + c])
  volumes = [('validation1', block)]
  t_devs = []
  for r in range(args.repeats + 1):  # the first call is the warm-up
    t0 = time.time()
    got = ops.build(volumes, (0, 0, 0), np.random.RandomState(2))
    if r:
      t_devs.append(time.time() - t0)
  split = dict(ops.split)
  t0 = time.time()
  want = coordinates_ref.coordinates_spec(volumes, (0, 0, 0),
                                          np.random.RandomState(2))
  t_cpu = time.time() - t0
  same = (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
          and list(got[2].items()) == list(want[2].items()))
  t_dev = stats(t_devs)[0]
  print('  %d^3 block, margin 0, %d rows: device build (rows on the host) %s, '
        'of which host RNG %.3f s; numpy restatement on this host, one run, '
        '%.2f s (%.1f x); rows %s' % (
            c, len(want[0]), fmt(t_devs, unit='s'), split['host_rng'], t_cpu,
            t_cpu / t_dev, 'identical' if same else 'DIFFER'))
  if not same:
    sys.exit(1)


if __name__ == '__main__':
  main()
