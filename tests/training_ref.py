"""Numpy restatement of the training loop's data plumbing (include/
ffn_evaluation.h load_augmented / gather_train, ffn_amd/training/examples.py,
train.py) on top of tests/evaluation_ref.py, and of the whole loop with
gradients_ref.run + optimizer_ref.Optimizer as the train step.

`RefOps` stands in for EvaluationOps and `RefTrainer` for ConvStackTrainer so
that BatchExampleIter and the loop run on a CPU.  `run_loop` is written a
second time, independently of BatchExampleIter, as the reference's generators
are: one generator per slot, asked in slot order.
"""
import collections

import numpy as np
from scipy import special
import torch

from tests import evaluation_ref
from tests import gradients_ref
from tests import optimizer_ref

M = evaluation_ref.M


def transform(x, perm, reflect):
  """train.py's PermuteAndReflect on a [z, y, x] array."""
  out = np.transpose(x, tuple(int(p) for p in perm))
  axes = tuple(a for a in range(3) if int(reflect[a]))
  return np.ascontiguousarray(np.flip(out, axes) if axes else out)


def all_transforms():
  """The 6 x 8 (perm, reflect) pairs."""
  perms = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
  return [(p, ((r >> 2) & 1, (r >> 1) & 1, r & 1)) for p in perms
          for r in range(8)]


def load_augmented(image_volume, label_volume, centre_xyz, offset, scale, geom,
                   perm, reflect, seed_pad=0.05):
  """evaluation_ref.load, then the transform on image and labels; the seed is
  the fresh one.  The object mask is taken before the transform."""
  image, labels, seed = evaluation_ref.load(image_volume, label_volume,
                                            centre_xyz, offset, scale, geom,
                                            seed_pad)
  for a in range(3):
    if perm[a] != a and (image.shape[a] != image.shape[perm[a]] or
                         labels.shape[a] != labels.shape[perm[a]]):
      raise ValueError('axes of different size change places')
  return transform(image, perm, reflect), transform(labels, perm, reflect), seed


def gather_train(arrays, off_xyz, geom):
  """arrays: [image, labels, seed] of a slot -> (seed, image, labels) crops of
  get_example (examples.py:62-65)."""
  return (evaluation_ref.crop(arrays[2], off_xyz, geom['input_seed']),
          evaluation_ref.crop(arrays[0], off_xyz, geom['input_image']),
          evaluation_ref.crop(arrays[1], off_xyz, geom['pred_mask']))


class RefOps(evaluation_ref.RefOps):
  """EvaluationOps with the training calls, on numpy arrays."""

  def load_augmented(self, slots, volumes, centres_xyz, offsets, scales, perms,
                     reflects, seed_pad):
    self.calls['load_augmented'] += 1
    loaded = [load_augmented(*self.volumes[v], c, o, s, self.geom, p, r,
                             seed_pad)
              for v, c, o, s, p, r in zip(volumes, centres_xyz, offsets, scales,
                                          perms, reflects)]
    for slot, arrays in zip(slots, loaded):
      self.slots[slot] = list(arrays)

  def alloc_io_train(self, n):
    seed, image, logits = self.alloc_io(n)
    return seed, image, logits, np.zeros((n,) + self.geom['pred_mask'],
                                         np.float32)

  def gather_train(self, slots, offsets_xyz, seed_out, image_out, labels_out):
    self.calls['gather_train'] += 1
    crops = [gather_train(self.slots[s], o, self.geom)
             for s, o in zip(slots, offsets_xyz)]
    for k, (seed, image, labels) in enumerate(crops):
      seed_out[k], image_out[k], labels_out[k] = seed, image, labels


class RefTrainer:
  """ConvStackTrainer.train_step_device restated: gradients_ref.run for the
  loss and the gradients, optimizer_ref.Optimizer for the update, in float32 or
  float64.  The logits come back as float32, what the seed canvas holds."""

  def __init__(self, variables, depth, f64=False, **flags):
    self.np_dtype = np.float64 if f64 else np.float32
    self.torch_dtype = torch.float64 if f64 else torch.float32
    self.depth = depth
    self.variables = {k: np.asarray(v, self.np_dtype)
                      for k, v in variables.items()}
    self.optimizer = optimizer_ref.Optimizer(dtype=self.np_dtype, **flags)
    self.losses = []

  @property
  def global_step(self):
    return self.optimizer.global_step

  def train_step_device(self, seed, image, labels, weights):
    out = gradients_ref.run(self.variables, self.depth, np.asarray(seed),
                            np.asarray(image), np.asarray(labels),
                            np.asarray(weights), dtype=self.torch_dtype)
    grads = {k: np.asarray(g, self.np_dtype) for k, g in out['grads'].items()}
    self.variables = self.optimizer.step(self.variables, grads)
    self.losses.append(out['loss'])
    return (out['loss'], np.asarray(out['logits'], np.float32),
            self.optimizer.global_step)


# ---- the loop, restated with one generator per slot -----------------------------


def example_stream(slot, source, geom, fov_policy, threshold, shifts, seed_pad,
                   log, margins):
  """get_example with its policy generator inlined.  `source()` -> (example
  index, image volume, label volume, centre, offset, scale, perm, reflect).
  Yields (seed view, image crop, labels crop); the caller writes the seed view.
  Appends one entry per example to `log`."""
  seed_thr = special.logit(threshold)
  label_thr = special.expit(seed_thr)
  deltas_xyz = geom['deltas'][::-1]
  lo = [(a - p) // 2 for a, p in zip(geom['input_seed'], geom['pred_mask'])]
  inner = tuple(slice(l, l + p) for l, p in zip(lo, geom['pred_mask']))
  while True:
    index, image_volume, label_volume, centre, offset, scale, perm, reflect = (
        source())
    image, labels, seed = load_augmented(image_volume, label_volume, centre,
                                         offset, scale, geom, perm, reflect,
                                         seed_pad)
    entry = {'coordinate': index, 'slot': slot, 'perm': tuple(perm),
             'reflect': tuple(reflect), 'offsets': [], 'records': [],
             'seed': seed, 'finished': False}
    log.append(entry)

    def eval_move(off):
      valid, wanted = evaluation_ref.probe(seed, labels, off, seed_thr,
                                           label_thr)
      o = tuple(off)[::-1]
      margins.append(abs(float(
          seed[tuple(s // 2 + d for s, d in zip(seed.shape, o))]) - seed_thr))
      return valid, wanted

    def crops(off):
      entry['offsets'].append(tuple(int(v) for v in off))
      window = evaluation_ref.crop(seed, off, geom['input_seed'])
      return (window[inner],
              evaluation_ref.crop(image, off, geom['input_image']),
              evaluation_ref.crop(labels, off, geom['pred_mask']))

    if fov_policy == 'fixed':
      for off in [(0, 0, 0)] + list(shifts):
        valid, wanted = eval_move(off)
        entry['records'].append((bool(wanted), bool(valid), tuple(off)))
        if valid:
          yield crops(off)
    elif fov_policy == 'max_pred_moves':
      max_radius = [p // 2 - f // 2 for p, f in
                    zip(geom['image_patch'][::-1], geom['input_image'][::-1])]
      queue = collections.deque([(0, 0, 0)])
      done = set()
      while queue:
        off = queue.popleft()
        if any(abs(o) > m for o, m in zip(off, max_radius)):
          continue
        quantized = tuple((o + d / 2) // max(d, 1)
                          for o, d in zip(off, deltas_xyz))
        if quantized in done:
          continue
        valid, wanted = eval_move(off)
        entry['records'].append((bool(wanted), bool(valid), (0, 0, 0)))
        if not valid or (not wanted and quantized != (0, 0, 0)):
          continue
        done.add(quantized)
        yield crops(off)
        scores, positions = evaluation_ref.face_scores(
            evaluation_ref.crop(seed, off, geom['pred_mask']), geom['deltas'])
        found = set()
        for f in range(6):
          if geom['deltas'][f // 2] == 0:
            continue
          margins.append(abs(float(scores[f]) - seed_thr))
          if scores[f] < seed_thr:
            continue
          found.add((float(scores[f]), tuple(int(v) for v in positions[f])))
        queue.extend((p[2] + off[0], p[1] + off[1], p[0] + off[2])
                     for _, p in sorted(found, reverse=True))
    else:
      raise ValueError(fov_policy)
    entry['finished'] = True


def run_loop(trainer, volumes, coordinates, transforms, geom, fov_policy,
             batch_size, steps, threshold=0.9, seed_pad=0.05, shifts=None):
  """The loop of train.py:384-412.  volumes: {name: (image, labels, offset,
  scale)}; coordinates are cycled in order; transforms: (perm, reflect) per
  example started, in starting order (cycled).  -> dict: examples (the log, in
  starting order, each with its final or current seed), losses, margins."""
  shifts = (evaluation_ref.model_shifts(geom['deltas'][::-1])
            if shifts is None else shifts)
  log, margins = [], []

  def source():
    k = len(log)
    centre, name = coordinates[k % len(coordinates)]
    perm, reflect = transforms[k % len(transforms)]
    image_volume, label_volume, offset, scale = volumes[name]
    return (k % len(coordinates), image_volume, label_volume, centre, offset,
            scale, perm, reflect)

  streams = [example_stream(s, source, geom, fov_policy, threshold, shifts,
                            seed_pad, log, margins) for s in range(batch_size)]
  weights = np.ones((batch_size,) + tuple(geom['pred_mask']), np.float32)
  losses = []
  for _ in range(steps):
    batch = [next(g) for g in streams]  # in slot order
    seed = np.stack([b[0] for b in batch])
    # (the conv stack takes seed, image, labels of one shape)
    assert geom['input_seed'] == geom['pred_mask'] == geom['input_image']
    loss, logits, _ = trainer.train_step_device(
        seed, np.stack([b[1] for b in batch]), np.stack([b[2] for b in batch]),
        weights)
    losses.append(loss)
    for k, b in enumerate(batch):
      b[0][...] = logits[k]
  return {'examples': log, 'losses': losses, 'margins': margins}
