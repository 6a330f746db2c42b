"""Batches of training examples from the evaluation unit: the reference's
ffn/training/examples.py (get_example, _batch_gen, BatchExampleIter) with the
voxel arrays resident on the GPU.

`BatchExampleIter` keeps `batch_size` slots of an EvaluationOps busy, one
independent example stream per slot as in the reference's `_batch_gen`.  A
stream loads the next coordinate with a freshly sampled PermuteAndReflect
transform (EvaluationOps.load_augmented; with `sections`, also a freshly
sampled plan of section augmentations, EvaluationOps.load_sections), walks
the FoV offsets of its move policy (evaluation.FovWalk, the same walk
CheckpointEvaluator runs), and when they are exhausted scores the slot with
`finish` into an EvalResult, as get_example calls EvalTracker.add_patch,
before it takes the next coordinate.
`next()` hands out the seed, image, label and weight arrays of one FoV per
slot as device arrays; `update_seeds()` pastes the network's logits back.
The host sees probe results, face maxima and the finish sums only: no voxel
array crosses to the host inside a step.

What differs from the reference: the coordinates come from a list that is
cycled without end (reshuffled per epoch under `shuffle_seed`) instead of
tf.train.shuffle_batch's queue; the slots ask for their coordinates in slot
order, not from racing threads; coordinates whose patches leave their volume
are skipped and counted; the loss weights are one array of ones (a permuted
array of ones is itself).  No CPU fallback: the ops raise without a GPU.
"""

from __future__ import annotations

import random
from typing import Optional, Sequence

import numpy as np

from . import evaluation

TRAIN_POLICIES = ('fixed', 'max_pred_moves')
IDENTITY = ((0, 1, 2), (0, 0, 0))


def fits(centre_xyz, shape_zyx, geometry, margin_yx=(0, 0)) -> bool:
  """Whether the image and label patches around a centre, enlarged by
  `margin_yx` voxels on both sides of y and x (what the section augmentations
  read), stay inside a volume of `shape_zyx` (the reference would fail in a
  reshape otherwise)."""
  margins = (0, int(margin_yx[0]), int(margin_yx[1]))
  for axis in range(3):
    c = int(centre_xyz[2 - axis])
    for size in (geometry.image_patch[axis], geometry.label_patch[axis]):
      start = c - (size - 1) // 2 - margins[axis]
      if start < 0 or start + size + 2 * margins[axis] > shape_zyx[axis]:
        return False
  return True


def torch_io(geometry, batch_size: int, device):
  """(seed, image, labels, weights) torch tensors for `batch_size` FoVs on
  `device`, the weights all one."""
  import torch  # pylint:disable=g-import-not-at-top
  new = lambda dims: torch.zeros((batch_size,) + tuple(dims),
                                 dtype=torch.float32, device=device)
  weights = torch.ones((batch_size,) + tuple(geometry.pred_mask),
                       dtype=torch.float32, device=device)
  out = (new(geometry.input_seed), new(geometry.input_image),
         new(geometry.pred_mask), weights)
  if getattr(device, 'type', str(device)[:4]) == 'cuda':
    torch.cuda.synchronize(device)
  return out


class BatchExampleIter:
  """Endless batches of `batch_size` FoVs for a train step.

  info: a ModelInfo (xyz arrays).
  ops: an EvaluationOps, or an object with its methods.  The iterator
    configures it and replaces its volumes: an ops serves one user at a time.
  volumes: {name: (image zyx, labels zyx, offset, scale)}; the image is
    normalised as (float(v) - offset) / scale.
  coordinates: (centre (x, y, z), volume name) pairs, as
    coordinates.read_tfrecord returns them zipped.
  fov_policy: 'fixed' or 'max_pred_moves' (train.py:96).
  shifts: the moves of 'fixed' in the order to try them, (x, y, z); with
    `shuffle_moves` they are shuffled once with random.Random(moves_seed), as
    train.py:353-355 shuffles model.shifts.
  transform: an augmentation.PermuteAndReflect (anything with `sample()` ->
    (perm, reflect)); None trains unaugmented.
  shuffle_seed: None runs the coordinates in the given order, epoch after
    epoch; otherwise random.Random(shuffle_seed) reshuffles them per epoch.
  io: (seed, image, labels, weights) device arrays the caller made (what the
    trainer takes: torch tensors); default: the unit's own buffers and
    `weights` None.
  sections: an augmentation.SectionAugmentations (anything with `sample(image
    patch zyx, label patch zyx)` -> SectionPlan and `margin_yx`); a plan is
    sampled for every example started, after the transform, from the sections'
    own generator, and the example is loaded with EvaluationOps.load_sections.
    Coordinates whose patches enlarged by the margin leave their volume are
    skipped.  None: load_augmented, as before.
  result: an evaluation.EvalResult to score into instead of one of the
    iterator's own, so the iterators of several replicas of one process
    accumulate into one (it must have been made for the same shifts in the same
    order); `reset_result(result)` hands every one of them the next.  None: an
    EvalResult of its own, as before.
  keep_history: keep, per example started, its coordinate index, transform,
    offsets and records (and its section plan under 'plan') in `history`
    (tests; it grows without bound).
  """

  def __init__(self, info, ops, volumes, coordinates, fov_policy: str = 'fixed',
               fov_moves: int = 1, batch_size: int = 4, threshold: float = 0.9,
               seed_pad: float = 0.05, shifts: Optional[Sequence] = None,
               shuffle_moves: bool = False, moves_seed: Optional[int] = None,
               transform=None, shuffle_seed: Optional[int] = None, io=None,
               keep_history: bool = False, sections=None, result=None):
    if fov_policy not in TRAIN_POLICIES:
      raise ValueError('fov_policy is one of %r, got %r' %
                       (TRAIN_POLICIES, fov_policy))
    if not 1 <= int(batch_size) <= evaluation.MAX_SLOTS:
      raise ValueError('batch_size must be in [1, %d]' % evaluation.MAX_SLOTS)
    self.ops = ops
    self.fov_policy = fov_policy
    self.batch_size = int(batch_size)
    self.geometry = evaluation.Geometry.from_info(info, fov_policy, fov_moves,
                                                  self.batch_size)
    g = self.geometry
    for axis, p in enumerate(getattr(transform, 'permutable_axes', ())):
      for q in transform.permutable_axes[axis + 1:]:
        if (g.image_patch[p] != g.image_patch[q] or
            g.label_patch[p] != g.label_patch[q]):
          raise ValueError('axes %d and %d may change places but differ in '
                           'patch size' % (p, q))
    self.transform = transform
    self.sections = sections
    margin_yx = (0, 0) if sections is None else tuple(sections.margin_yx)
    #: per-augmentation counts of the reference's summaries, since the start
    self.section_counts = {'examples': 0, 'misalignment': 0,
                           'missing_sections': 0, 'outoffocus_sections': 0,
                           'grayscale': 0}
    self.seed_pad = float(seed_pad)
    self.threshold = evaluation.logit(threshold)
    self.label_threshold = evaluation.expit(self.threshold)
    deltas_xyz = tuple(int(v) for v in np.asarray(info.deltas))
    if shifts is None:
      d = deltas_xyz  # model.py:75-81
      shifts = [(dx, dy, dz) for dx in (-d[0], 0, d[0])
                for dy in (-d[1], 0, d[1]) for dz in (-d[2], 0, d[2])
                if (dx, dy, dz) != (0, 0, 0)]
    shifts = [tuple(int(v) for v in s) for s in shifts]
    if shuffle_moves:
      random.Random(moves_seed).shuffle(shifts)
    self.shifts = shifts
    self.walk = evaluation.FovWalk(fov_policy, g, shifts, deltas_xyz,
                                   self.threshold)
    ops.configure(g)
    ops.reset()
    self._volumes = {}
    for name in sorted(volumes):
      image, labels, offset, scale = volumes[name]
      index = ops.add_volume(image, labels)
      self._volumes[name] = (index, tuple(np.asarray(image).shape),
                             float(offset), float(scale))
    self.coordinates = []
    self.skipped = 0
    for centre, name in coordinates:
      if name not in self._volumes:
        raise KeyError('no volume named %r' % (name,))
      if fits(centre, self._volumes[name][1], g, margin_yx):
        self.coordinates.append((tuple(int(v) for v in centre), name))
      else:
        self.skipped += 1
    if not self.coordinates:
      raise ValueError('none of the %d coordinates has its patches inside its '
                       'volume' % self.skipped)
    self._shuffle = (None if shuffle_seed is None
                     else random.Random(shuffle_seed))
    self._order = []
    self.epochs = 0
    if io is None:
      seed, image, _, labels = ops.alloc_io_train(self.batch_size)
      io = (seed, image, labels, None)
    self._io = tuple(io)
    self._layout = (evaluation.EvaluationOps.LOGITS_FOV
                    if g.pred_mask != g.input_seed
                    else evaluation.EvaluationOps.LOGITS_PRED)
    self._streams = [self.walk.new_stream()
                     for _ in range(self.batch_size)]
    self._current = [None] * self.batch_size  # the history entry of a slot
    self._slots = list(range(self.batch_size))
    self._pasted = True
    self.keep_history = bool(keep_history)
    self.history = []
    self.examples_started = 0
    self.examples_finished = 0
    self.steps = 0
    self.result = (result if result is not None
                   else evaluation.EvalResult(self.shifts))

  # -- bookkeeping ---------------------------------------------------------------

  def reset_result(self, result=None):
    """EvalTracker.reset: a fresh `result` for the next summary interval (or
    the given one, shared with other iterators)."""
    self.result = (result if result is not None
                   else evaluation.EvalResult(self.shifts))

  def _count_sections(self, plan):
    summary = plan.summary()
    counts = self.section_counts
    counts['examples'] += 1
    counts['misalignment'] += summary['misalignment_z'] >= 0
    counts['missing_sections'] += len(summary['missing_z'])
    counts['outoffocus_sections'] += len(summary['outoffocus_z'])
    counts['grayscale'] += summary['grayscale']

  def _next_coordinate(self) -> int:
    if not self._order:
      self._order = list(range(len(self.coordinates)))
      if self._shuffle is not None:
        self._shuffle.shuffle(self._order)
      self._order.reverse()  # popped from the end
      self.epochs += 1
    return self._order.pop()

  def offsets(self):
    """The offset (x, y, z) of every slot's current step."""
    return [self._streams[s].offset for s in self._slots]

  # -- the iterator --------------------------------------------------------------

  def __iter__(self):
    return self

  def __next__(self):
    return self.next()

  def next(self):
    """-> (seed [n, input_seed], image [n, input_image], labels [n,
    pred_mask], weights): device arrays, n = batch_size; valid until the next
    call."""
    if not self._pasted:
      raise RuntimeError('update_seeds() has to follow every next()')
    ops, streams = self.ops, self._streams
    eval_voxels = int(np.prod(self.geometry.eval))
    need = list(self._slots)
    rounds = 0
    while need:
      rounds += 1
      if rounds > 64:
        raise RuntimeError('examples end without a step: the seed centre is '
                           'below the move threshold')
      fresh = [s for s in need if streams[s].example is None]
      if fresh:
        rows, perms, reflects, plans = [], [], [], []
        for s in fresh:
          index = self._next_coordinate()
          perm, reflect = (self.transform.sample() if self.transform is not None
                           else IDENTITY)
          self.walk.start(streams[s], index)
          rows.append(self.coordinates[index])
          perms.append(perm)
          reflects.append(reflect)
          entry = {'coordinate': index, 'slot': s,
                   'perm': tuple(int(v) for v in perm),
                   'reflect': tuple(int(v) for v in reflect),
                   'offsets': [], 'records': []}
          if self.sections is not None:
            plan = self.sections.sample(self.geometry.image_patch,
                                        self.geometry.label_patch)
            plans.append(plan)
            entry['plan'] = plan
            self._count_sections(plan)
          self._current[s] = entry
          if self.keep_history:
            self.history.append(entry)
          self.examples_started += 1
        vols = [self._volumes[name] for _, name in rows]
        if self.sections is None:
          ops.load_augmented(fresh, [v[0] for v in vols], [c for c, _ in rows],
                             [v[2] for v in vols], [v[3] for v in vols], perms,
                             reflects, self.seed_pad)
        else:
          ops.load_sections(fresh, [v[0] for v in vols], [c for c, _ in rows],
                            [v[2] for v in vols], [v[3] for v in vols], perms,
                            reflects, plans, self.seed_pad)
      pairs = [(s, o) for s in need for o in self.walk.candidates(streams[s])]
      probed = {s: {} for s in need}
      if pairs:
        valid, wanted = ops.probe_moves(
            [s for s, _ in pairs], [o for _, o in pairs], self.threshold,
            self.label_threshold)
        for (s, o), v, w in zip(pairs, valid, wanted):
          probed[s][o] = (bool(v), bool(w))
      again = []
      for s in need:
        stream = streams[s]
        entry = self._current[s]
        stream.offset = self.walk.next_offset(stream, probed[s], self.result,
                                              entry['records'])
        if stream.offset is None:
          loss_sum, counts, masked = ops.finish(s)
          self.result.add_patch(loss_sum / eval_voxels, counts, eval_voxels,
                                masked)
          self.examples_finished += 1
          stream.example = None
          again.append(s)
        else:
          entry['offsets'].append(stream.offset)
      need = again
    seed, image, labels, weights = self._io
    ops.gather_train(self._slots, self.offsets(), seed, image, labels)
    self.result.track_weights(
        self.batch_size * int(np.prod(self.geometry.pred_mask)))
    self._pasted = False
    return seed, image, labels, weights

  def update_seeds(self, logits):
    """BatchExampleIter.update_seeds from a device array: dense [n, input_seed]
    logits as the train step returns them (their centred pred_mask box is
    used), or dense [n, pred_mask] where the two sizes are equal."""
    offsets = self.offsets()
    self.ops.paste(self._slots, offsets, logits, self._layout)
    if self.fov_policy == 'max_pred_moves':
      scores, positions = self.ops.score_faces(self._slots, offsets)
      for k, s in enumerate(self._slots):
        self.walk.extend_queue(self._streams[s], scores[k], positions[k])
    self._pasted = True
    self.steps += 1
