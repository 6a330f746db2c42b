#!/usr/bin/env python
"""Forward plus backward of the conv stack on the GPU
(ffn_amd/training/gradients.py): FoV 33^3, depth 12, batches of 1, 8 and 16.

Per batch size it reports the kernel time of every kind of call summed over
one loss_and_gradients() (HIP events, the unit's last_timing), the wall time
per batch, and the fraction of the f32-MFMA peak that wall time stands for:
3 x 45.7 GFLOP per FoV (forward, backward to the input, backward to the
weights) against 157 TFLOP/s.  One JSON line per batch size.

  python tools/gpu_gradients_bench.py [--batches 1 8 16] [--repeats 3]
      [--weights tests/golden/fib25_weights.npz]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd.training import gradients  # pylint:disable=g-import-not-at-top
from ffn_amd.training.models import convstack_3d

GFLOP_PER_FOV = 3 * 45.7
PEAK_TFLOPS = 157.0


class TimedOps:
  """Forwards to a GradientOps and adds up last_timing() per kind of call."""

  def __init__(self, ops):
    self._ops = ops
    self.ms = {name: 0.0 for name in gradients.TIMED_CALLS}
    self.calls = {name: 0 for name in gradients.TIMED_CALLS}

  def reset(self):
    for name in self.ms:
      self.ms[name] = 0.0
      self.calls[name] = 0

  def close(self):
    self._ops.close()

  def __getattr__(self, name):
    fn = getattr(self._ops, name)
    if name not in self.ms:
      return fn

    def timed(*args, **kwargs):
      out = fn(*args, **kwargs)
      self.ms[name] += self._ops.last_timing()[name]
      self.calls[name] += 1
      return out
    return timed


def inputs(n, zyx, seed=0):
  rng = np.random.RandomState(seed)
  shape = (n,) + tuple(zyx)
  logit = lambda p: np.log(p / (1 - p))
  image = rng.normal(0, 1, shape).astype(np.float32)
  s = (logit(0.05) + rng.normal(0, 0.5, shape)).astype(np.float32)
  s[:, zyx[0] // 2, zyx[1] // 2, zyx[2] // 2] = np.float32(logit(0.95))
  labels = np.where(rng.uniform(size=shape) < 0.3, 0.95, 0.05).astype(np.float32)
  return s, image, labels, np.ones(shape, np.float32)


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
  ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 16])
  ap.add_argument('--fov', type=int, nargs=3, default=[33, 33, 33],
                  metavar=('Z', 'Y', 'X'))
  ap.add_argument('--depth', type=int, default=12)
  ap.add_argument('--repeats', type=int, default=3)
  ap.add_argument('--weights', default=None,
                  help='.npz keyed by the checkpoint\'s variable names '
                  '(default: random weights)')
  ap.add_argument('--device', type=int, default=0)
  args = ap.parse_args()

  zyx = tuple(args.fov)
  model = convstack_3d.ConvStack3DFFNModel(fov_size=list(zyx[::-1]),
                                           deltas=[8, 8, 8], depth=args.depth)
  if args.weights:
    model.load_checkpoint(args.weights)
  else:
    model.init_random(stddev=0.05)
  import torch  # pylint:disable=g-import-not-at-top
  for n in args.batches:
    csg = gradients.ConvStackGradients(model, n, args.device)
    timed = TimedOps(csg.ops)
    csg.ops = timed
    dev = [torch.from_numpy(a).to(csg.device) for a in inputs(n, zyx)]
    csg.loss_and_gradients(*dev)  # warm-up: buffers, code objects
    wall = []
    for _ in range(args.repeats):
      timed.reset()
      t0 = time.perf_counter()
      loss, _, _ = csg.loss_and_gradients(*dev)
      wall.append(time.perf_counter() - t0)
    best = min(wall)
    print(json.dumps({
        'batch': n, 'fov_zyx': list(zyx), 'depth': args.depth, 'loss': loss,
        'kernel_ms': {k: round(v, 3) for k, v in timed.ms.items()},
        'calls': timed.calls,
        'kernel_ms_total': round(sum(timed.ms.values()), 3),
        'wall_ms_per_batch': round(best * 1e3, 3),
        'wall_ms_per_fov': round(best * 1e3 / n, 3),
        'fraction_of_f32_mfma_peak': round(
            GFLOP_PER_FOV * n / best / 1e3 / PEAK_TFLOPS, 4),
        'kernel_fraction_of_peak': round(
            GFLOP_PER_FOV * n / (sum(timed.ms.values()) * 1e-3) / 1e3 /
            PEAK_TFLOPS, 4),
    }), flush=True)
    csg.close()
    del csg, timed, dev
    torch.cuda.empty_cache()


if __name__ == '__main__':
  main()
