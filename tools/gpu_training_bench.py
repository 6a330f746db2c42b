#!/usr/bin/env python
"""One training step of the conv stack on the GPU
(ffn_amd/training/trainer.py): FoV 33^3, depth 12, batches of 1, 8 and 16.

Per batch size: the wall time of ConvStackTrainer.train_step (sgd) against the
wall time of ConvStackGradients.loss_and_gradients (own buffers, gradients
copied to the host: what a user had before the trainer), taken alternately in
one process, median and range over the repeats.  Both end in a device
synchronise: every call of the units returns with its kernels complete.

Per update rule: the HIP-event kernel time of grad_stats and of apply over the
whole arena (the units' last_timing, median and least over the steps) and
apply's effective bandwidth: the bytes the rule must move -- params and
gradients read, params written, every slot read and written, 4 bytes each --
over the kernel time.  One JSON line per batch size and per rule.

Synchronous replicas: the HIP-event kernel time of aggregate over the arena
at 2, 8 and 32 replicas (and the bandwidth of n arrays read, one written), and
the wall time of a step of two local replicas (two contribute, one
apply_contributions) against two plain train steps at batch 4.  One process
on one GPU: no collective runs here.

  python tools/gpu_training_bench.py [--batches 1 8 16] [--repeats 10]
      [--weights tests/golden/fib25_weights.npz] [--only_replicas]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd.training import gradients  # pylint:disable=g-import-not-at-top
from ffn_amd.training import optimizer
from ffn_amd.training import trainer as trainer_lib
from ffn_amd.training.models import convstack_3d
from tools.gpu_gradients_bench import inputs


def bytes_per_element(rule):
  """What apply must move: p and g in, p out, each slot in and out."""
  return 4 * (3 + 2 * len(optimizer.SLOT_INIT[rule]))


def spread(ms):
  return {'median': round(statistics.median(ms), 4), 'min': round(min(ms), 4),
          'max': round(max(ms), 4)}


def main():
  ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
  ap.add_argument('--batches', type=int, nargs='+', default=[1, 8, 16])
  ap.add_argument('--fov', type=int, nargs=3, default=[33, 33, 33],
                  metavar=('Z', 'Y', 'X'))
  ap.add_argument('--depth', type=int, default=12)
  ap.add_argument('--repeats', type=int, default=10)
  ap.add_argument('--weights', default=None,
                  help='.npz keyed by the checkpoint\'s variable names '
                  '(default: random weights)')
  ap.add_argument('--device', type=int, default=0)
  ap.add_argument('--aggregate', type=int, nargs='*', default=[2, 8, 32],
                  help='replica counts of the aggregate part')
  ap.add_argument('--replica_batch', type=int, default=4)
  ap.add_argument('--only_replicas', action='store_true',
                  help='the aggregate part alone')
  args = ap.parse_args()

  zyx = tuple(args.fov)
  model = convstack_3d.ConvStack3DFFNModel(fov_size=list(zyx[::-1]),
                                           deltas=[8, 8, 8], depth=args.depth)
  if args.weights:
    model.load_checkpoint(args.weights)
  else:
    model.init_random(stddev=0.05)
  import torch  # pylint:disable=g-import-not-at-top

  if args.only_replicas:
    replicas_part(args, model, zyx)
    return

  for n in args.batches:
    csg = gradients.ConvStackGradients(model, n, args.device)
    tr = trainer_lib.ConvStackTrainer(model, optimizer.OptimizerConfig(), n,
                                      args.device)
    dev = [torch.from_numpy(a).to(csg.device) for a in inputs(n, zyx)]
    torch.cuda.synchronize()
    csg.loss_and_gradients(*dev)  # warm-up: buffers, code objects
    tr.train_step(*dev)
    step_ms, grad_ms = [], []
    for _ in range(args.repeats):
      t0 = time.perf_counter()
      csg.loss_and_gradients(*dev)
      grad_ms.append((time.perf_counter() - t0) * 1e3)
      t0 = time.perf_counter()
      loss, _, _ = tr.train_step(*dev)
      step_ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({
        'batch': n, 'fov_zyx': list(zyx), 'depth': args.depth,
        'repeats': args.repeats, 'loss': loss,
        'train_step_wall_ms': spread(step_ms),
        'loss_and_gradients_wall_ms': spread(grad_ms),
        'train_step_over_loss_and_gradients': round(
            statistics.median(step_ms) / statistics.median(grad_ms), 4),
    }), flush=True)
    csg.close()
    tr.close()
    del csg, tr, dev
    torch.cuda.empty_cache()

  n = args.batches[0]
  dev = None
  for rule in optimizer.RULES:
    tr = trainer_lib.ConvStackTrainer(
        model, optimizer.OptimizerConfig(optimizer=rule), n, args.device)
    if dev is None:
      dev = [torch.from_numpy(a).to(tr.device) for a in inputs(n, zyx)]
      torch.cuda.synchronize()
    tr.train_step(*dev)  # warm-up
    stats_ms, apply_ms = [], []
    for _ in range(args.repeats):
      tr.train_step(*dev)
      timing = tr.ops.last_timing()
      stats_ms.append(timing['grad_stats'])
      apply_ms.append(timing['apply'])
    moved = tr.layout.total * bytes_per_element(rule)
    print(json.dumps({
        'rule': rule, 'elements': tr.layout.total,
        'bytes_per_element': bytes_per_element(rule),
        'grad_stats_kernel_ms': spread(stats_ms),
        'apply_kernel_ms': spread(apply_ms),
        'apply_effective_GBps_at_median': round(
            moved / (statistics.median(apply_ms) * 1e-3) / 1e9, 1),
        'apply_effective_GBps_at_min': round(
            moved / (min(apply_ms) * 1e-3) / 1e9, 1),
    }), flush=True)
    tr.close()
    del tr
    torch.cuda.empty_cache()
  replicas_part(args, model, zyx)


def replicas_part(args, model, zyx):
  """The aggregate kernel over the arena at n replicas, and a step of two
  local replicas against two plain steps."""
  import torch  # pylint:disable=g-import-not-at-top
  ops = optimizer.OptimizerOps(args.device)
  total = optimizer.arena_layout(args.depth).total
  device = torch.device('cuda', args.device)
  for n in args.aggregate:
    src = torch.randn((n, total), dtype=torch.float32, device=device) * 0.5
    dst = torch.empty((total,), dtype=torch.float32, device=device)
    torch.cuda.synchronize()
    ops.aggregate(total, n, src, total, 0.7, dst)  # warm-up
    ms = []
    for _ in range(args.repeats):
      ops.aggregate(total, n, src, total, 0.7, dst)
      ms.append(ops.last_timing_aggregate())
    moved = 4 * total * (n + 1)
    print(json.dumps({
        'aggregate_replicas': n, 'elements': total,
        'aggregate_kernel_ms': spread(ms),
        'aggregate_effective_GBps_at_median': round(
            moved / (statistics.median(ms) * 1e-3) / 1e9, 1),
    }), flush=True)
    del src, dst
  ops.close()
  batch = args.replica_batch
  plain = trainer_lib.ConvStackTrainer(model, optimizer.OptimizerConfig(),
                                       batch, args.device)
  two = trainer_lib.ConvStackTrainer(model, optimizer.OptimizerConfig(), batch,
                                     args.device, replicas=2)
  dev = [torch.from_numpy(a).to(plain.device) for a in inputs(batch, zyx)]
  torch.cuda.synchronize()
  plain.train_step_device(*dev)  # warm-up
  two.contribute(0, *dev)
  two.contribute(1, *dev)
  two.apply_contributions()
  plain_ms, two_ms = [], []
  for _ in range(args.repeats):
    t0 = time.perf_counter()
    plain.train_step_device(*dev)
    plain.train_step_device(*dev)
    plain_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    two.contribute(0, *dev)
    two.contribute(1, *dev)
    two.apply_contributions()
    two_ms.append((time.perf_counter() - t0) * 1e3)
  print(json.dumps({
      'batch': batch, 'fov_zyx': list(zyx), 'depth': args.depth,
      'repeats': args.repeats,
      'two_plain_steps_wall_ms': spread(plain_ms),
      'two_replica_step_wall_ms': spread(two_ms),
      'two_replica_step_over_two_plain_steps': round(
          statistics.median(two_ms) / statistics.median(plain_ms), 4),
  }), flush=True)
  plain.close()
  two.close()


if __name__ == '__main__':
  main()
