"""Numpy restatement of the forward-only evaluation loop
(ffn_amd/training/evaluation.py, include/ffn_evaluation.h): every call of the
unit as a few lines of numpy, the loop one example at a time (examples are
independent of each other), and the accumulators of the reference's EvalTracker
with its float32 `loss` and `fov_stats` holders.  `RefOps` / `RefEngine` stand in
for the device unit and the engine so that CheckpointEvaluator runs on a CPU.

The "network" is any callable forward(seed [n, z, y, x], image [n, z, y, x]) ->
logits of the whole FoV.
"""
import collections

import numpy as np
from scipy import special

M = 1e-3  # logit units: the margin the minter keeps around every threshold


def zyx(v):
  return tuple(int(x) for x in np.asarray(v)[::-1])


def geometry(input_seed_xyz, input_image_xyz, pred_mask_xyz, deltas_xyz,
             fov_policy, fov_moves):
  """train.py:155-179 -> dict of zyx tuples."""
  moves = fov_moves + 1 if fov_policy == 'max_pred_moves' else fov_moves
  d = np.asarray(deltas_xyz)
  return dict(
      input_seed=zyx(input_seed_xyz), input_image=zyx(input_image_xyz),
      pred_mask=zyx(pred_mask_xyz), deltas=zyx(deltas_xyz),
      canvas=zyx(np.asarray(input_seed_xyz) + d * 2 * moves),
      image_patch=zyx(np.asarray(input_image_xyz) + d * 2 * moves),
      label_patch=zyx(np.asarray(pred_mask_xyz) + d * 2 * moves),
      eval=zyx(np.asarray(pred_mask_xyz) + d * 2 * fov_moves))


def model_shifts(deltas_xyz):
  """reference model.py:75-81."""
  d = [int(v) for v in deltas_xyz]
  return [(dx, dy, dz) for dx in (-d[0], 0, d[0]) for dy in (-d[1], 0, d[1])
          for dz in (-d[2], 0, d[2]) if (dx, dy, dz) != (0, 0, 0)]


# ---- the unit's calls --------------------------------------------------------------


def patch_of(volume, centre_xyz, size_zyx):
  """inputs.load_from_numpylike: the box of `size` around a centre, or
  ValueError where it leaves the volume."""
  sel = []
  for axis in range(3):
    start = int(centre_xyz[2 - axis]) - (size_zyx[axis] - 1) // 2
    if start < 0 or start + size_zyx[axis] > volume.shape[axis]:
      raise ValueError('patch leaves the volume')
    sel.append(slice(start, start + size_zyx[axis]))
  return volume[tuple(sel)]


def load(image_volume, label_volume, centre_xyz, offset, scale, geom,
         seed_pad=0.05):
  """-> (image patch, soft labels, seed canvas), all f32 (train.py:232-274,
  examples.py:59)."""
  raw = patch_of(image_volume, centre_xyz, geom['image_patch'])
  lab = patch_of(label_volume, centre_xyz, geom['label_patch'])
  image = (raw.astype(np.float32) - np.float32(offset)) / np.float32(scale)
  centre = lab[tuple(s // 2 for s in lab.shape)]
  lom = (lab > 0) & (lab == centre)
  labels = np.where(lom, np.float32(0.95), np.float32(0.05)).astype(np.float32)
  seed = np.full(geom['canvas'], seed_pad, np.float32)
  seed[tuple(s // 2 for s in seed.shape)] = 0.95
  return image, labels, special.logit(seed)


def crop(data, off_xyz, crop_zyx):
  """mask.crop_and_pad on a [z, y, x] array -> view."""
  start = [s // 2 - c // 2 + int(o)
           for s, c, o in zip(data.shape, crop_zyx, tuple(off_xyz)[::-1])]
  if min(start) < 0 or any(st + c > s for st, c, s in
                           zip(start, crop_zyx, data.shape)):
    raise ValueError('crop leaves the array')
  return data[tuple(slice(st, st + c) for st, c in zip(start, crop_zyx))]


def probe(seed, labels, off_xyz, seed_threshold, label_threshold):
  """examples._eval_move -> (valid, wanted).  The thresholds are float64, as
  special.logit / special.expit return them: numpy compares in float64."""
  seed_threshold = np.float64(seed_threshold)
  label_threshold = np.float64(label_threshold)
  o = tuple(off_xyz)[::-1]
  valid = seed[tuple(s // 2 + d for s, d in zip(seed.shape, o))] >= seed_threshold
  wanted = (labels[tuple(s // 2 + d for s, d in zip(labels.shape, o))] >=
            label_threshold)
  return bool(valid), bool(wanted)


def paste(seed, off_xyz, logits_pred, geom):
  """BatchExampleIter.update_seeds."""
  window = crop(seed, off_xyz, geom['input_seed'])
  lo = [(s - p) // 2 for s, p in zip(geom['input_seed'], geom['pred_mask'])]
  window[tuple(slice(l, l + p) for l, p in zip(lo, geom['pred_mask']))] = (
      logits_pred)


def face_scores(prob_map, deltas_zyx):
  """The six face maxima of movement.get_scored_move_offsets before its
  threshold: (scores (6,), positions (6, 3) zyx relative to the centre), faces
  in z-, z+, y-, y+, x-, x+ order; first maximum in C order."""
  centre = [s // 2 for s in prob_map.shape]
  sub = [slice(c - d, c + d + 1) for c, d in zip(centre, deltas_zyx)]
  scores = np.zeros(6, np.float32)
  positions = np.zeros((6, 3), np.int32)
  for axis in range(3):
    for k, sign in enumerate((-1, 1)):
      sel = list(sub)
      sel[axis] = centre[axis] + sign * deltas_zyx[axis]
      face = prob_map[tuple(sel)]
      pos = np.unravel_index(face.argmax(), face.shape)
      rel = [pos[0] - face.shape[0] // 2, pos[1] - face.shape[1] // 2]
      rel.insert(axis, sign * deltas_zyx[axis])
      scores[2 * axis + k] = face[pos]
      positions[2 * axis + k] = rel
  return scores, positions


def loss_terms(x, z):
  """max(x, 0) - x z + log1p(exp(-|x|)) in float64: the formula TensorFlow
  documents for sigmoid_cross_entropy_with_logits."""
  x = np.asarray(x, np.float64)
  z = np.asarray(z, np.float64)
  return np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))


def finish(seed, labels, geom):
  """EvalTracker.add_patch -> (loss sum f64, [tp, tn, fp, fn], masked)."""
  x = crop(seed, (0, 0, 0), geom['eval'])
  z = crop(labels, (0, 0, 0), geom['eval'])
  pred = x >= special.logit(0.9)
  true = z > 0.5
  counts = [int((pred & true).sum()), int((~pred & ~true).sum()),
            int((pred & ~true).sum()), int((~pred & true).sum())]
  return float(loss_terms(x, z).sum()), counts, 0


# ---- the loop, one example at a time ---------------------------------------------


class Tracker:
  """EvalTracker's accumulators with its dtypes (tracker.py:100-114)."""

  def __init__(self, shifts):
    self.moves = np.zeros(3, np.int64)
    self.moves_by_r = {r: np.zeros(3, np.int64) for r in sorted(
        {int(np.linalg.norm(s)) for s in shifts} | {0})}
    self.loss = np.zeros(1, np.float32)
    self.num_patches = np.zeros(1, np.int64)
    self.num_voxels = np.zeros(2, np.int64)
    self.prediction_counts = np.zeros(4, np.int64)
    self.fov_stats = np.zeros(3, np.float32)

  def record_move(self, wanted, executed, off_xyz):
    r = int(np.linalg.norm(off_xyz))
    kind = (0 if executed else 1) if wanted else (2 if executed else None)
    if kind is not None:
      self.moves[kind] += 1
      self.moves_by_r[r][kind] += 1


def walk(forward, image, labels, seed, geom, fov_policy, threshold, shifts,
         tracker, margins=None):
  """One example: the policy's generator and get_example's loop around it.
  Changes `seed` in place; returns (offsets taken, records).  `margins`
  collects |value - threshold| of everything compared with a move threshold."""
  seed_thr = special.logit(threshold)
  label_thr = special.expit(seed_thr)
  deltas_xyz = geom['deltas'][::-1]
  offsets, records = [], []

  def note(value, thr):
    if margins is not None:
      margins.append(abs(float(value) - float(thr)))

  def eval_move(off):
    valid, wanted = probe(seed, labels, off, seed_thr, label_thr)
    o = tuple(off)[::-1]
    note(seed[tuple(s // 2 + d for s, d in zip(seed.shape, o))], seed_thr)
    return valid, wanted

  def step(off):
    offsets.append(tuple(int(v) for v in off))
    s = crop(seed, off, geom['input_seed'])
    im = crop(image, off, geom['input_image'])
    logits = forward(s[None], im[None])[0]
    lo = [(a - p) // 2 for a, p in zip(geom['input_seed'], geom['pred_mask'])]
    paste(seed, off, logits[tuple(slice(l, l + p) for l, p in
                                  zip(lo, geom['pred_mask']))], geom)
    voxels = int(np.prod(geom['pred_mask']))
    tracker.fov_stats[0] += voxels
    tracker.fov_stats[2] += np.float32(voxels)

  def record(wanted, valid, off):
    tracker.record_move(wanted, valid, off)
    records.append((bool(wanted), bool(valid), tuple(int(v) for v in off)))

  if fov_policy == 'no_step':
    record(True, True, (0, 0, 0))
    step((0, 0, 0))
  elif fov_policy == 'fixed':
    for off in [(0, 0, 0)] + list(shifts):
      valid, wanted = eval_move(off)
      record(wanted, valid, off)
      if valid:
        step(off)
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
      record(wanted, valid, (0, 0, 0))
      if not valid or (not wanted and quantized != (0, 0, 0)):
        continue
      done.add(quantized)
      step(off)
      scores, positions = face_scores(crop(seed, off, geom['pred_mask']),
                                      geom['deltas'])
      found = set()
      for f in range(6):
        if geom['deltas'][f // 2] == 0:
          continue
        note(scores[f], seed_thr)
        if scores[f] < seed_thr:
          continue
        found.add((float(scores[f]), tuple(int(v) for v in positions[f])))
      queue.extend((p[2] + off[0], p[1] + off[1], p[0] + off[2])
                   for _, p in sorted(found, reverse=True))
  else:
    raise ValueError(fov_policy)

  _, counts, masked = finish(seed, labels, geom)
  voxels = int(np.prod(geom['eval']))
  # (the mean as np.mean takes it, then into the float32 holder)
  tracker.loss[:] += loss_terms(crop(seed, (0, 0, 0), geom['eval']),
                                crop(labels, (0, 0, 0), geom['eval'])).mean()
  tracker.num_voxels[0] += voxels
  tracker.num_voxels[1] += masked
  tracker.prediction_counts += np.asarray(counts, np.int64)
  tracker.num_patches[:] += 1
  return offsets, records


def evaluate(forward, volumes, coordinates, geom, fov_policy, threshold=0.9,
             seed_pad=0.05, shifts=None, margins=None):
  """volumes: {name: (image, labels, offset, scale)}; coordinates: (centre xyz,
  name) pairs, all inside their volumes.  -> (Tracker, per-example offsets,
  per-example records, per-example final seeds)."""
  shifts = model_shifts(geom['deltas'][::-1]) if shifts is None else shifts
  tracker = Tracker(shifts)
  all_offsets, all_records, seeds = [], [], []
  for centre, name in coordinates:
    image_volume, label_volume, offset, scale = volumes[name]
    image, labels, seed = load(image_volume, label_volume, centre, offset,
                               scale, geom, seed_pad)
    offsets, records = walk(forward, image, labels, seed, geom, fov_policy,
                            threshold, shifts, tracker, margins)
    all_offsets.append(offsets)
    all_records.append(records)
    seeds.append(seed)
  return tracker, all_offsets, all_records, seeds


def sample_seed(seed, step=3):
  """Every `step`-th voxel per axis, counted from the centre outward."""
  sel = tuple(slice((s // 2) % step, None, step) for s in seed.shape)
  return seed[sel]


# ---- stand-ins for the device unit and the engine -------------------------------


class RefOps:
  """EvaluationOps on numpy arrays; "device arrays" are numpy arrays."""

  LOGITS_PRED = 0
  LOGITS_FOV = 1

  def __init__(self):
    self.volumes = []
    self.geometry = None
    self.calls = collections.Counter()

  def configure(self, geometry):
    self.geometry = geometry
    self.geom = {k: tuple(getattr(geometry, k)) for k in (
        'input_seed', 'input_image', 'pred_mask', 'deltas', 'canvas',
        'image_patch', 'label_patch', 'eval')}
    self.slots = [None] * geometry.slots

  def reset(self):
    self.volumes = []

  def add_volume(self, image, labels):
    self.volumes.append((np.asarray(image), np.asarray(labels)))
    return len(self.volumes) - 1

  def load(self, slots, volumes, centres_xyz, offsets, scales, seed_pad):
    self.calls['load'] += 1
    loaded = [load(*self.volumes[v], c, o, s, self.geom, seed_pad)
              for v, c, o, s in zip(volumes, centres_xyz, offsets, scales)]
    for slot, arrays in zip(slots, loaded):
      self.slots[slot] = list(arrays)

  def probe_moves(self, slots, offsets_xyz, seed_threshold, label_threshold):
    self.calls['probe_moves'] += 1
    out = [probe(self.slots[s][2], self.slots[s][1], o, seed_threshold,
                 label_threshold) for s, o in zip(slots, offsets_xyz)]
    return (np.array([v for v, _ in out], bool),
            np.array([w for _, w in out], bool))

  def alloc_io(self, n):
    g = self.geom
    return (np.zeros((n,) + g['input_seed'], np.float32),
            np.zeros((n,) + g['input_image'], np.float32),
            np.zeros((n,) + g['input_seed'], np.float32))

  def gather(self, slots, offsets_xyz, seed_out, image_out):
    self.calls['gather'] += 1
    for k, (s, o) in enumerate(zip(slots, offsets_xyz)):
      seed_out[k] = crop(self.slots[s][2], o, self.geom['input_seed'])
      image_out[k] = crop(self.slots[s][0], o, self.geom['input_image'])

  def paste(self, slots, offsets_xyz, logits, layout=0):
    self.calls['paste'] += 1
    g = self.geom
    lo = [(a - p) // 2 for a, p in zip(g['input_seed'], g['pred_mask'])]
    for k, (s, o) in enumerate(zip(slots, offsets_xyz)):
      box = logits[k]
      if layout == self.LOGITS_FOV:
        box = box[tuple(slice(l, l + p) for l, p in zip(lo, g['pred_mask']))]
      paste(self.slots[s][2], o, box, g)

  def score_faces(self, slots, offsets_xyz):
    self.calls['score_faces'] += 1
    out = [face_scores(crop(self.slots[s][2], o, self.geom['pred_mask']),
                       self.geom['deltas']) for s, o in zip(slots, offsets_xyz)]
    return np.stack([a for a, _ in out]), np.stack([b for _, b in out])

  def finish(self, slot, pred_threshold=None):
    self.calls['finish'] += 1
    return finish(self.slots[slot][2], self.slots[slot][1], self.geom)

  def read_seed(self, slot):
    return self.slots[slot][2].copy()

  def read_labels(self, slot):
    return self.slots[slot][1].copy()

  def read_image(self, slot):
    return self.slots[slot][0].copy()


class RefEngine:
  """predict_device over a forward callable."""

  def __init__(self, forward):
    self.forward = forward
    self.batches = []

  def predict_device(self, n, seed, image, logits):
    self.batches.append(int(n))
    logits[:n] = self.forward(seed[:n], image[:n])


def toy_forward(seed, image):
  """A cheap stand-in network for tests of the loop's bookkeeping: grows the
  object along bright voxels.  logits = seed + update, as the real one."""
  seed = np.asarray(seed, np.float32)
  image = np.asarray(image, np.float32)
  from scipy import ndimage  # pylint:disable=g-import-not-at-top
  grown = ndimage.maximum_filter(seed, size=(1, 7, 7, 7), mode='constant',
                                 cval=-10.0)
  bright = np.maximum(seed, grown - np.float32(0.2)) + np.float32(0.01) * image
  return np.where(image > 0, bright, seed - np.float32(0.4)).astype(np.float32)
