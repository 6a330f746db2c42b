#!/usr/bin/env python3
"""Throughput of the training loop (ffn_amd/training/examples.py +
trainer.train_step_device) and what its two new kernels cost.  Reports;
asserts nothing.

  python tools/gpu_train_loop_bench.py [--size 250] [--steps 40]
      [--batches 1,8,16] [--kernel-batches 1,32] [--repeats 20] [--sections]

Part 1: one synthetic size^3 volume (ffn_amd/synthetic.py cells phantom and its
labels), the FIB-25 geometry and weights (33^3 FoV, depth 12, deltas 8), policy
'fixed', momentum, PermuteAndReflect over y, x / z, y, x as train.py's defaults
have it.  Per batch size, after one warm-up batch: steps/s and examples
(FoVs)/s over `steps` steps, the share of the wall time spent outside
train_step_device, and the calls of the unit per step.

Part 2: HIP-event kernel times (ffn_evaluation_last_timing /
last_timing_train; median of `repeats` calls after two warm-up calls) on 49^3
patches at batch 1 and 32: load_augmented with the identity, an x reflection,
an x-y swap and a z-x swap against load, and gather_train against gather.

--sections: part 1 runs every batch size a second time with the section
augmentations on (SECTIONS below: all four, never skipped), and part 2 adds
load_sections (ffn_evaluation_last_timing_sections: the whole call, and its
first launch alone) with an empty plan and with a full one: a translation by
(4, -4) from the middle section, two blanked sections, a blur of sigma 2
(radius 8) on every fourth section, grayscale factors on all of them.
"""
import argparse
import collections
import os
import sys
import time

import numpy as np
import torch  # before the library is loaded: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ffn_amd import synthetic  # noqa: E402
from ffn_amd.training import augmentation  # noqa: E402
from ffn_amd.training import evaluation  # noqa: E402
from ffn_amd.training import examples  # noqa: E402
from ffn_amd.training import optimizer  # noqa: E402
from ffn_amd.training import trainer as trainer_lib  # noqa: E402
from ffn_amd.training.models import convstack_3d  # noqa: E402

COUNTED = ('load_augmented', 'load_sections', 'probe_moves', 'gather_train',
           'paste', 'finish')
SECTIONS = dict(misalignment_skip_ratio=0.0, max_xy_offset=4,
                slip_vs_translate_ratio=0.5, missing_section_skip_ratio=0.0,
                max_missing_section_indices_ratio=0.05,
                outoffocus_skip_ratio=0.0, max_outoffocus_indices_ratio=0.25,
                max_filter_stdev=2.0, grayscale_skip_ratio=0.0,
                max_contrast_factor=0.3, max_brightness_factor=0.3)
TRANSFORMS = [('identity', (0, 1, 2), (0, 0, 0)),
              ('x-reflect', (0, 1, 2), (0, 0, 1)),
              ('xy-swap', (0, 2, 1), (0, 0, 0)),
              ('zx-swap', (2, 1, 0), (0, 0, 0))]


class CountedOps:
  """An EvaluationOps whose calls are counted and wall-timed."""

  def __init__(self, ops):
    self._ops = ops
    self.clear()

  def clear(self):
    self.calls = collections.Counter()
    self.wall_ms = collections.Counter()

  def __getattr__(self, name):
    attr = getattr(self._ops, name)
    if name not in COUNTED:
      return attr

    def timed(*args, **kwargs):
      t0 = time.time()
      out = attr(*args, **kwargs)
      self.wall_ms[name] += (time.time() - t0) * 1e3
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


def loop_part(model, volumes, coords, batches, steps, with_sections=False):
  ops = CountedOps(evaluation.default_ops(0))
  runs = [(b, on) for b in batches for on in ((False, True) if with_sections
                                              else (False,))]
  for batch, on in runs:
    sections = augmentation.SectionAugmentations(SECTIONS, 1) if on else None
    trainer = trainer_lib.ConvStackTrainer(
        model, optimizer.OptimizerConfig(optimizer='momentum'),
        max_batch=batch)
    geometry = evaluation.Geometry.from_info(model.info, 'fixed', 1, batch)
    it = examples.BatchExampleIter(
        model.info, ops, volumes, coords, batch_size=batch,
        transform=augmentation.PermuteAndReflect((1, 2), (0, 1, 2), 1),
        shuffle_moves=True, moves_seed=1, shuffle_seed=1, sections=sections,
        io=examples.torch_io(geometry, batch, trainer.device))

    def run(n):
      in_step = 0.0
      for _ in range(n):
        seed, image, labels, weights = it.next()
        t0 = time.time()
        _, logits, _ = trainer.train_step_device(seed, image, labels, weights)
        in_step += time.time() - t0
        it.update_seeds(logits)
      return in_step

    run(1)  # warm-up
    ops.clear()
    started = it.examples_started
    t0 = time.time()
    in_step = run(steps)
    wall = time.time() - t0
    print('  batch %2d%s: %6.2f steps/s, %7.1f FoVs/s (%d steps, %.3f s, %d '
          'examples started); train step %.2f ms; outside it %.1f %% of the '
          'wall time = %.1f us per step' % (
              batch, ' with sections' if on else '', steps / wall,
              steps * batch / wall, steps, wall,
              it.examples_started - started, 1e3 * in_step / steps,
              100 * (1 - in_step / wall), 1e6 * (wall - in_step) / steps))
    for kind in COUNTED:
      if ops.calls[kind]:
        print('            %-14s %5.2f calls / step, wall %8.2f us / call' % (
            kind, ops.calls[kind] / steps,
            1e3 * ops.wall_ms[kind] / ops.calls[kind]))
    sys.stdout.flush()
    trainer.close()


def full_plan(g):
  sections = g.image_patch[0]
  plan = augmentation.SectionPlan(sections, (4, 4))
  plan.kind, plan.z0, plan.dy, plan.dx = (augmentation.TRANSLATION,
                                          sections // 2, 4, -4)
  plan.blank_value = np.float32(200.0)
  plan.blank_mask[[3, sections - 2]] = 8
  plan.blur_sigma = np.float32(2.0)
  plan.blur_mask[::4] = 8
  plan.gray[:] = 1
  plan.factors[:] = (1.1, -0.05, 0.8)
  return plan


def kernel_part(model, image, labels, coords, batches, repeats,
                with_sections=False):
  ops = evaluation.default_ops(0)
  median = lambda values: float(np.median(values))
  for batch in batches:
    g = evaluation.Geometry.from_info(model.info, 'fixed', 1, batch)
    ops.configure(g)
    ops.reset()
    vol = ops.add_volume(image, labels)
    slots = list(range(batch))
    centres = [c for c, _ in coords[:batch]]
    args = (slots, [vol] * batch, centres, [128.0] * batch, [33.0] * batch)
    rows = []
    times = []
    for k in range(repeats + 2):
      ops.load(*args, 0.05)
      times.append(ops.last_timing()['load'])
    base = median([t[0] for t in times[2:]])
    rows.append(('load', base, times[-1][1]))
    for name, perm, reflect in TRANSFORMS:
      times = []
      for k in range(repeats + 2):
        ops.load_augmented(*args, [perm] * batch, [reflect] * batch, 0.05)
        times.append(ops.last_timing_train()['load_augmented'])
      rows.append(('load_augmented ' + name, median([t[0] for t in times[2:]]),
                   times[-1][1]))
    if with_sections:
      identity = ([(0, 1, 2)] * batch, [(0, 0, 0)] * batch)
      for name, plan in (('empty', augmentation.SectionPlan(g.image_patch[0])),
                         ('full', full_plan(g))):
        times = []
        for k in range(repeats + 2):
          ops.load_sections(*args, *identity, [plan] * batch, 0.05)
          times.append(ops.last_timing_sections())
        for kind in evaluation.SECTION_CALL_KINDS:
          rows.append(('%s %s' % (kind, name),
                       median([t[kind][0] for t in times[2:]]),
                       times[-1][kind][1]))
    new = lambda dims: torch.empty((batch,) + tuple(dims),
                                   dtype=torch.float32, device='cuda:0')
    io = [new(g.input_seed), new(g.input_image), new(g.pred_mask)]
    torch.cuda.synchronize()
    offsets = [(8, -8, 0)] * batch
    for name in ('gather', 'gather_train'):
      times = []
      for k in range(repeats + 2):
        if name == 'gather':
          ops.gather(slots, offsets, io[0], io[1])
          times.append(ops.last_timing()['gather'])
        else:
          ops.gather_train(slots, offsets, *io)
          times.append(ops.last_timing_train()['gather_train'])
      rows.append((name, median([t[0] for t in times[2:]]), times[-1][1]))
    print('  batch %2d, patches %r:' % (batch, g.image_patch))
    for name, ms, nbytes in rows:
      print('    %-26s %8.1f us  %8.2f MB  %7.1f GB/s  x%.2f of load' % (
          name, 1e3 * ms, nbytes / 1e6, nbytes / (ms * 1e-3) / 1e9 if ms else 0,
          ms / base if base else 0))
    sys.stdout.flush()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--size', type=int, default=250)
  ap.add_argument('--steps', type=int, default=40)
  ap.add_argument('--batches', default='1,8,16')
  ap.add_argument('--kernel-batches', default='1,32')
  ap.add_argument('--repeats', type=int, default=20)
  ap.add_argument('--sections', action='store_true')
  args = ap.parse_args()
  shape = (args.size,) * 3
  image = synthetic.cells_volume(shape, seed=1234)
  labels = synthetic.cells_labels(shape, seed=1234)
  with np.load(os.path.join(ROOT, 'tests', 'golden', 'fib25_weights.npz')) as d:
    variables = {k: d[k] for k in d.files}
  model = convstack_3d.ConvStack3DFFNModel(fov_size=[33, 33, 33],
                                           deltas=[8, 8, 8], depth=12)
  model.set_variables(variables)
  coords = coordinates_of(labels, 64, 34, 7)
  ints = lambda text: [int(b) for b in text.split(',') if b]
  print('%d^3 cells phantom, FIB-25 geometry, policy fixed' % args.size)
  loop_part(model, {'vol': (image, labels, 128.0, 33.0)}, coords,
            ints(args.batches), args.steps, args.sections)
  kernel_part(model, image, labels, coords, ints(args.kernel_batches),
              args.repeats, args.sections)


if __name__ == '__main__':
  main()
