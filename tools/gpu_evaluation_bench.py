#!/usr/bin/env python3
"""Throughput of the forward-only evaluation loop (ffn_amd/training/
evaluation.py) and where a FoV step's time goes.  Reports; asserts nothing.

  python tools/gpu_evaluation_bench.py [--size 250] [--examples 64]
      [--batches 1,8,16,32] [--policy fixed] [--cpu-examples 2]

One synthetic size^3 volume (ffn_amd/synthetic.py cells phantom and its
labels), the FIB-25 weights (33^3 FoV, depth 12), `examples` coordinates drawn
from cell interiors with a seeded generator.  Per batch size, after a warm-up
run over the first batch's worth of coordinates: examples/s and FoV-steps/s of
evaluate(), the share of its wall time spent outside engine.predict_device,
and per call kind of the unit the number of calls, the HIP-event kernel time
per call (ffn_evaluation_last_timing) and the wall time per call.  Then the
numpy restatement (tests/evaluation_ref.py) with the CPU baseline forward
(oracle/ffn_oracle.forward) on the first `cpu-examples` coordinates, for
comparison on the same host.
"""
import argparse
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd import engine as hip_engine  # noqa: E402
from ffn_amd import synthetic  # noqa: E402
from ffn_amd.training import evaluation  # noqa: E402
from ffn_amd.training.models import convstack_3d  # noqa: E402
from oracle import ffn_oracle  # noqa: E402
from tests import evaluation_ref  # noqa: E402


class TimedOps:
  """An EvaluationOps whose calls are counted and timed."""

  def __init__(self, ops):
    self._ops = ops
    self.clear()

  def clear(self):
    self.calls = collections.Counter()
    self.kernel_ms = collections.Counter()
    self.wall_ms = collections.Counter()

  def __getattr__(self, name):
    attr = getattr(self._ops, name)
    if name not in evaluation.CALL_KINDS:
      return attr

    def timed(*args, **kwargs):
      t0 = time.time()
      out = attr(*args, **kwargs)
      self.wall_ms[name] += (time.time() - t0) * 1e3
      self.kernel_ms[name] += self._ops.last_timing()[name][0]
      self.calls[name] += 1
      return out

    return timed


def coordinates_of(labels, n, margin, seed):
  from scipy import ndimage  # pylint:disable=g-import-not-at-top
  ok = ndimage.distance_transform_edt(labels > 0) >= 3
  ok[:margin] = ok[-margin:] = False
  ok[:, :margin] = ok[:, -margin:] = False
  ok[:, :, :margin] = ok[:, :, -margin:] = False
  pool = np.argwhere(ok)
  rng = np.random.RandomState(seed)
  picks = pool[rng.choice(len(pool), n, replace=False)]
  return [((int(x), int(y), int(z)), 'vol') for z, y, x in picks]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=250)
  ap.add_argument('--examples', type=int, default=64)
  ap.add_argument('--batches', default='1,8,16,32')
  ap.add_argument('--policy', default='fixed', choices=evaluation.POLICIES)
  ap.add_argument('--fov-moves', type=int, default=1)
  ap.add_argument('--cpu-examples', type=int, default=2)
  args = ap.parse_args()
  shape = (args.size,) * 3
  image = synthetic.cells_volume(shape, seed=1234)
  labels = synthetic.cells_labels(shape, seed=1234)
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'fib25_weights.npz')) as d:
    variables = {k: d[k] for k in d.files}
  model = convstack_3d.ConvStack3DFFNModel(fov_size=[33, 33, 33],
                                           deltas=[8, 8, 8], depth=12)
  model.set_variables(variables)
  coords = coordinates_of(labels, args.examples, 34, 7)
  print('%d^3 cells phantom, %d examples, policy %s, fov_moves %d' % (
      args.size, len(coords), args.policy, args.fov_moves))
  ops = TimedOps(evaluation.default_ops(0))
  for batch in [int(b) for b in args.batches.split(',')]:
    eng = hip_engine.HipEngine.from_model(model, max_batch=batch, device_id=0)
    ev = evaluation.CheckpointEvaluator(model, eng, ops, args.policy,
                                        args.fov_moves, batch_size=batch)
    ev.add_volume('vol', image, labels, 128.0, 33.0)
    ev.evaluate(coords[:batch])  # warm-up
    ops.clear()
    ev.forward_seconds = ev.total_seconds = 0.0
    ev.steps = 0
    result = ev.evaluate(coords)
    fovs = sum(len(o) for o in result.offsets)
    wall = ev.total_seconds
    print('  batch %2d: %7.1f examples/s, %8.1f FoV-steps/s (%d FoVs in %d '
          'batched steps, %.3f s); forward %.3f s = %.1f %% of the wall time, '
          '%.1f %% outside it; %.1f us per step outside the forward' % (
              batch, len(coords) / wall, fovs / wall, fovs, ev.steps, wall,
              ev.forward_seconds, 100 * ev.forward_seconds / wall,
              100 * (1 - ev.forward_seconds / wall),
              1e6 * (wall - ev.forward_seconds) / max(ev.steps, 1)))
    print('            forward per batched step %.1f us' % (
        1e6 * ev.forward_seconds / max(ev.steps, 1)))
    for kind in evaluation.CALL_KINDS:
      if ops.calls[kind]:
        print('            %-12s %5d calls, kernels %8.2f us / call, wall '
              '%8.2f us / call' % (
                  kind, ops.calls[kind],
                  1e3 * ops.kernel_ms[kind] / ops.calls[kind],
                  1e3 * ops.wall_ms[kind] / ops.calls[kind]))
    sys.stdout.flush()
    eng.close()

  if args.cpu_examples:
    blob = ffn_oracle.weights_blob(variables, 12)
    geom = evaluation_ref.geometry((33,) * 3, (33,) * 3, (33,) * 3, (8,) * 3,
                                   args.policy, args.fov_moves)
    t0 = time.time()
    _, offsets, _, _ = evaluation_ref.evaluate(
        lambda seed, im: ffn_oracle.forward(im, seed, blob, 12),
        {'vol': (image, labels, 128.0, 33.0)}, coords[:args.cpu_examples], geom,
        args.policy)
    wall = time.time() - t0
    fovs = sum(len(o) for o in offsets)
    print('  numpy restatement + CPU baseline forward, %d examples: %.2f '
          'examples/s, %.1f FoV-steps/s' % (args.cpu_examples,
                                            args.cpu_examples / wall,
                                            fovs / wall))


if __name__ == '__main__':
  main()
