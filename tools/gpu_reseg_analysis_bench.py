#!/usr/bin/env python3
"""Per-point cost of evaluating pair resegmentation results on the GPU, next
to the numpy / scipy restatement on the same host.

  python tools/gpu_reseg_analysis_bench.py [--points 256] [--radius 48]
      [--analysis-radius 32] [--distinct 8] [--repeats 5] [--files 32]
      [--voxel-size 33 8 8] [--out profiles/reseg_analysis.txt]

`--distinct` seeded synthetic pair points (blob objects grown from the two
base segments, quantised maps with never-visited zeros) are generated at the
given box and repeated to `--points`; one Analyzer.pair_stats call evaluates
them all.  Reported per point:
  kernels   HIP-event time of the mask / EDT launches (uploads excluded),
  batch     host wall time of the pair_stats call: staging copy, upload,
            kernels, read-back,
  files     wall time of evaluate_pairs over `--files` result files: np.load,
            the crop of the base segmentation, then the same batch call,
  cpu       tests/reseg_analysis_ref.py (four scipy distance transforms plus
            the reductions) on the distinct points, one thread.
Medians over `--repeats` calls after one warm-up call; min..max beside them.
The GPU rows are checked against the restatement before anything is timed.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd import analysis  # noqa: E402
from ffn_amd.inference import resegmentation_analysis  # noqa: E402
from ffn_amd.inference import storage  # noqa: E402
from tests import reseg_analysis_ref as ra  # noqa: E402


def stats(values):
  values = sorted(values)
  return values[len(values) // 2], values[0], values[-1]


def synthetic_point(seed, radius, analysis_radius):
  """(probs u8 [2, box], base segmentation u64 [box], ids) of one point."""
  rng = np.random.default_rng(seed)
  box = tuple(2 * r + 1 for r in radius)
  # blocky base segmentation: smooth noise cut into a dozen ids
  field = ndimage.gaussian_filter(rng.random(box), 6.0)
  ranks = np.digitize(field, np.quantile(field, np.linspace(0, 1, 13)[1:-1]))
  seg = (ranks.astype(np.uint64) * np.uint64(2**33 + 7)) * (ranks > 0)
  id_a = int(seg[tuple(radius)]) or int(seg.max())
  others = np.unique(seg[tuple(slice(r - a, r + a + 1)
                               for r, a in zip(radius, analysis_radius))])
  id_b = int([v for v in others if v not in (0, id_a)][0])
  probs = []
  for target in (seg == id_a, seg == id_b):
    p = ndimage.gaussian_filter(target.astype(np.float32), 2.0) * 1.3
    p += rng.normal(0, 0.05, box).astype(np.float32)
    p = np.clip(p, 0.001, 0.999)
    p[ndimage.gaussian_filter(rng.random(box), 4.0) < 0.497] = np.nan
    probs.append(storage.quantize_probability(p))
  return np.array(probs), seg, id_a, id_b


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--points', type=int, default=256)
  ap.add_argument('--radius', type=int, default=48)
  ap.add_argument('--analysis-radius', type=int, default=32)
  ap.add_argument('--distinct', type=int, default=8)
  ap.add_argument('--repeats', type=int, default=5)
  ap.add_argument('--files', type=int, default=32)
  ap.add_argument('--threshold', type=float, default=0.5)
  ap.add_argument('--voxel-size', type=float, nargs=3, default=(33, 8, 8))
  ap.add_argument('--out', default='')
  args = ap.parse_args()
  radius = (args.radius,) * 3
  ar = (args.analysis_radius,) * 3
  delta = tuple(r - a for r, a in zip(radius, ar))
  voxel = tuple(args.voxel_size)
  crop = tuple(slice(d, d + 2 * a + 1) for d, a in zip(delta, ar))
  lines = []

  def say(text=''):
    print(text, flush=True)
    lines.append(text)

  points = [synthetic_point(100 + k, radius, ar) for k in range(args.distinct)]
  items = [analysis.PairInput(p[0], np.ascontiguousarray(p[1][crop]), delta,
                              p[2], p[3]) for p in points]
  batch = [items[k % len(items)] for k in range(args.points)]
  table = analysis.object_table(args.threshold)
  box = points[0][0].shape[1:]
  shape = items[0].seg.shape
  say('resegmentation analysis, pair points')
  say('box %dx%dx%d (radius %d), analysis box %dx%dx%d (radius %d), voxel size '
      'zyx %s, threshold %g' % (box + (args.radius,) + shape +
                                (args.analysis_radius, voxel, args.threshold)))
  say('batch: %d points in one pair_stats call (%d distinct, repeated); '
      '%.1f MB uploaded per point' % (
          args.points, len(items),
          (2 * shape[0] * box[1] * box[2] + 8 * items[0].seg.size) / 1e6))

  analyzer = analysis.default_analyzer(0)
  # correctness first, and the CPU time of the same points
  t0 = time.perf_counter()
  want = [ra.pair_stats(p.probs, p.seg, p.offset_zyx, p.id_a, p.id_b, table,
                        voxel) for p in items]
  cpu_s = (time.perf_counter() - t0) / len(items)
  counts, edt = analyzer.pair_stats(batch, table, voxel)  # warm-up
  for k in range(args.points):
    w = want[k % len(items)]
    assert np.array_equal(counts[k], w[0]) and edt[k].tobytes() == w[1].tobytes()
  say('GPU rows equal the restatement (counts exact, maxima bit for bit); '
      'object voxels per mask, first point: %s' % counts[0, [0, 1, 4, 5]].tolist())

  kernel, wall = [], []
  for _ in range(args.repeats):
    t0 = time.perf_counter()
    analyzer.pair_stats(batch, table, voxel)
    wall.append((time.perf_counter() - t0) / args.points)
    kernel.append(analyzer.last_timing()[0][0] * 1e-3 / args.points)

  files_s = None
  if args.files:
    with tempfile.TemporaryDirectory() as tmp:
      vol_shape = (1, box[0], box[1], box[2] * len(points))
      volume = np.zeros(vol_shape, np.uint64)
      names = []
      for k in range(args.files):
        p = points[k % len(points)]
        x0 = (k % len(points)) * box[2]
        volume[0, :, :, x0:x0 + box[2]] = p[1]
        # distinct names for repeated points: the ids are what tells them apart
        case = {'probs': p[0], 'id_a': p[2], 'id_b': p[3],
                'point_zyx': [radius[0], radius[1], x0 + radius[2]],
                'deletes': [np.arange(5), np.arange(7)],
                'histories': [np.full((5, 3), args.radius),
                              np.full((7, 3), args.radius)],
                'start_points': [[(1, 2, 3)], [(4, 5, 6)]]}
        sub = os.path.join(tmp, '%03d' % k)
        os.mkdir(sub)
        names.append(ra.write_case_file(case, sub))
      runs = []
      for _ in range(max(args.repeats // 2, 2) + 1):
        t0 = time.perf_counter()
        got = resegmentation_analysis.evaluate_pairs(
            names, volume, radius, ar, voxel, args.threshold)
        runs.append((time.perf_counter() - t0) / len(names))
      assert all(not isinstance(g, Exception) for g in got), got
      assert got[0].eval.num_voxels_a == int(counts[0, 4])
      files_s = stats(runs[1:])

  say()
  say('per point                      median        min .. max')
  for name, (med, lo, hi) in (('kernels (HIP events)', stats(kernel)),
                              ('batch call (host wall)', stats(wall))):
    say('%-28s %9.3f ms  %9.3f .. %.3f ms' % (name, med * 1e3, lo * 1e3,
                                               hi * 1e3))
  if files_s:
    say('%-28s %9.3f ms  %9.3f .. %.3f ms   (%d files)' % (
        'from files (host wall)', files_s[0] * 1e3, files_s[1] * 1e3,
        files_s[2] * 1e3, args.files))
  say('%-28s %9.3f ms  (%d points, one pass)' % (
      'restatement on the CPU', cpu_s * 1e3, len(items)))
  k_med, w_med = stats(kernel)[0], stats(wall)[0]
  say()
  say('CPU / kernels: %.0fx; CPU / batch call: %.1fx%s' % (
      cpu_s / k_med, cpu_s / w_med,
      '; CPU / from files: %.1fx' % (cpu_s / files_s[0]) if files_s else ''))
  stages = [('the kernels', k_med), ('staging and upload', w_med - k_med)]
  if files_s:
    stages.append(('loading the files and cropping', files_s[0] - w_med))
  say('dominant stage: %s (%s)' % (
      max(stages, key=lambda s: s[1])[0],
      ', '.join('%s %.3f ms' % (n, t * 1e3) for n, t in stages)))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
      f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
