"""Forward-only evaluation of a checkpoint on training examples: the FoV loop of
the reference's train.py (examples.py, mask.py, tracker.EvalTracker) without
the optimiser, on one MI355X.

`EvaluationOps` is the Python handle over the evaluation kernels of
libffn_hip.so (include/ffn_evaluation.h): resident volumes, and per slot a seed
canvas, an image patch and a label patch on the device.  `CheckpointEvaluator`
keeps `batch_size` such slots busy the way the reference's `_batch_gen` does
(one independent example stream per slot) and composes the unit with
`HipEngine.predict_device`: gather -> forward -> paste, all device-resident.
The host keeps only what the move policies keep: the remaining shifts, or the
queue and the `done` set.  `EvalResult` holds the accumulators of the
reference's EvalTracker and `summaries()` its scalar summaries under the same
tags.  No CPU fallback: without the library / a GPU every device call raises.

Not covered: any backward pass, augmentation (evaluation runs
unaugmented; every loss weight is 1), the `fixed_offsets_window` policy, image
and mesh summaries, weighted or sampled coordinate sources.

For training the unit also has `load_augmented` (load with
train.py's PermuteAndReflect) and `gather_train` (gather plus the labels of the
FoV) and `load_sections` (load_augmented with the section augmentations of
augmentation.SectionPlan carried out on the device); `FovWalk`
holds the host halves of the move policies for this module's
CheckpointEvaluator and for examples.BatchExampleIter.
"""

from __future__ import annotations

import collections
import ctypes
import dataclasses
import math
import random
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .. import _lib
from .. import _unit
from .._lib import check

POLICIES = ('fixed', 'max_pred_moves', 'no_step')
MAX_SLOTS = 32
#: EvalTracker.eval_threshold (tracker.py:87)
EVAL_PROBABILITY = 0.9
CALL_KINDS = ('load', 'probe_moves', 'gather', 'paste', 'score_faces', 'finish')
TRAIN_CALL_KINDS = ('load_augmented', 'gather_train')
SECTION_CALL_KINDS = ('load_sections', 'sections_kernel')
#: numpy views of the ctypes mirrors of ffn_evaluation_section_plan / _section
PLAN_DTYPE = np.dtype(_lib.EvaluationSectionPlan)
SECTION_DTYPE = np.dtype(_lib.EvaluationSection)


def logit(p) -> float:
  """log(p / (1 - p)) in float64, as scipy.special.logit evaluates a Python
  float."""
  p = float(p)
  if p <= 0.0 or p >= 1.0:
    raise ValueError('a probability strictly between 0 and 1, got %r' % p)
  return math.log(p / (1.0 - p))


def f32_logit(p) -> np.float32:
  """The value mask.make_seed + special.logit put into the f32 seed: the logit
  of the float32 nearest to p, evaluated in f32 precision."""
  p32 = np.float32(p)
  with np.errstate(all='ignore'):
    from scipy import special  # pylint:disable=g-import-not-at-top
    return np.float32(special.logit(p32))


def ceil_f32(value: float) -> np.float32:
  """The smallest float32 that is >= value: for a float32 v, v >= ceil_f32(t)
  exactly when v >= t in float64, which is how numpy compares an f32 array with
  a float64 threshold."""
  out = np.float32(value)
  if float(out) < float(value):
    out = np.nextafter(out, np.float32(np.inf))
  return out


def expit(x: float) -> float:
  return 1.0 / (1.0 + math.exp(-float(x)))


@dataclasses.dataclass(frozen=True)
class Geometry:
  """Sizes of the loop, all (z, y, x) (train.py:155-179)."""
  input_seed: Tuple[int, int, int]
  input_image: Tuple[int, int, int]
  pred_mask: Tuple[int, int, int]
  deltas: Tuple[int, int, int]
  canvas: Tuple[int, int, int]
  image_patch: Tuple[int, int, int]
  label_patch: Tuple[int, int, int]
  eval: Tuple[int, int, int]
  slots: int

  @classmethod
  def from_info(cls, info, fov_policy: str, fov_moves: int, slots: int):
    """`info`: a ModelInfo (xyz arrays).  For 'max_pred_moves' the arrays hold
    one more move than the eval box, as train.py:155-159 has it."""
    if fov_policy not in POLICIES:
      raise ValueError('fov_policy is one of %r, got %r' %
                       (POLICIES, fov_policy))
    fov_moves = int(fov_moves)
    if fov_moves < 0:
      raise ValueError('fov_moves must not be negative')
    moves = fov_moves + 1 if fov_policy == 'max_pred_moves' else fov_moves
    zyx = lambda v: tuple(int(x) for x in np.asarray(v)[::-1])
    deltas = zyx(info.deltas)
    grow = lambda size, m: tuple(s + 2 * m * d for s, d in zip(zyx(size), deltas))
    return cls(input_seed=zyx(info.input_seed_size),
               input_image=zyx(info.input_image_size),
               pred_mask=zyx(info.pred_mask_size), deltas=deltas,
               canvas=grow(info.input_seed_size, moves),
               image_patch=grow(info.input_image_size, moves),
               label_patch=grow(info.pred_mask_size, moves),
               eval=grow(info.pred_mask_size, fov_moves), slots=int(slots))

  def max_radius_xyz(self):
    """train.py:357-368: how far an offset may go, (x, y, z)."""
    return tuple(p // 2 - f // 2
                 for p, f in zip(self.image_patch[::-1], self.input_image[::-1]))


class DeviceArray:
  """Address and shape of an f32 device array somebody else owns."""

  def __init__(self, address: int, shape):
    self._address = int(address)
    self.shape = tuple(shape)

  def data_ptr(self) -> int:
    return self._address


def _i32(values, shape=None) -> np.ndarray:
  out = np.ascontiguousarray(values, dtype=np.int32)
  return out if shape is None else out.reshape(shape)


def section_plan_arrays(plans, sections: int):
  """augmentation.SectionPlans -> (ffn_evaluation_section_plan [n],
  ffn_evaluation_section [n, sections]) as numpy arrays of the C layout."""
  c_plans = np.zeros(len(plans), PLAN_DTYPE)
  c_sections = np.zeros((len(plans), sections), SECTION_DTYPE)
  for k, p in enumerate(plans):
    if p.sections != sections:
      raise ValueError('a plan for %d sections, the image patch has %d' %
                       (p.sections, sections))
    c_plans['margin_yx'][k] = p.margin_yx
    for name in ('kind', 'z0', 'dy', 'dx', 'blank_value', 'blur_sigma'):
      c_plans[name][k] = getattr(p, name)
    for name in ('blank_mask', 'blur_mask', 'gray', 'blank_yx', 'blur_yx'):
      c_sections[name][k] = getattr(p, name)
    c_sections['contrast'][k] = p.factors[:, 0]
    c_sections['brightness'][k] = p.factors[:, 1]
    c_sections['gamma'][k] = p.factors[:, 2]
  return c_plans, c_sections


class EvaluationOps(_unit.Handle):
  """One stream + device storage for the evaluation kernels."""

  LOGITS_PRED = 0
  LOGITS_FOV = 1

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_evaluation_create', 'ffn_evaluation_destroy',
                     device_id)
    self.lock = threading.RLock()
    self.geometry = None
    self.num_volumes = 0

  def configure(self, geometry: Geometry):
    g = _lib.EvaluationGeometry()
    g.input_seed_zyx[:] = geometry.input_seed
    g.input_image_zyx[:] = geometry.input_image
    g.pred_mask_zyx[:] = geometry.pred_mask
    g.deltas_zyx[:] = geometry.deltas
    g.canvas_zyx[:] = geometry.canvas
    g.image_patch_zyx[:] = geometry.image_patch
    g.label_patch_zyx[:] = geometry.label_patch
    g.eval_zyx[:] = geometry.eval
    g.slots = geometry.slots
    with self.lock:
      check(self._lib.ffn_evaluation_configure(self._h, ctypes.byref(g)))
      self.geometry = geometry

  def reset(self):
    """Forgets every volume."""
    with self.lock:
      check(self._lib.ffn_evaluation_reset(self._h))
      self.num_volumes = 0

  def add_volume(self, image: np.ndarray, labels: np.ndarray) -> int:
    """image: uint8 or float32 zyx; labels: 4- or 8-byte integers of the same
    shape, none negative.  Both stay on the device; returns the volume index."""
    image = np.asarray(image)
    labels = np.asarray(labels)
    if image.ndim != 3 or image.shape != labels.shape:
      raise ValueError('image %r and labels %r must be 3d and of one shape' %
                       (image.shape, labels.shape))
    if image.dtype not in (np.uint8, np.float32):
      raise TypeError('images are uint8 or float32, got %s' % image.dtype)
    if labels.dtype.kind not in 'iu' or labels.dtype.itemsize not in (4, 8):
      raise TypeError('labels are 4- or 8-byte integers, got %s' % labels.dtype)
    if labels.dtype.kind == 'i' and labels.size and labels.min() < 0:
      raise ValueError('negative label ids are not supported')
    image = np.ascontiguousarray(image)
    labels = np.ascontiguousarray(labels)
    index = ctypes.c_int32(-1)
    with self.lock:
      check(self._lib.ffn_evaluation_add_volume(
          self._h, image.ctypes.data, image.dtype.itemsize, labels.ctypes.data,
          labels.dtype.itemsize, (ctypes.c_int64 * 3)(*image.shape),
          ctypes.byref(index)))
      self.num_volumes += 1
    return int(index.value)

  def load(self, slots, volumes, centres_xyz, offsets, scales, seed_pad: float):
    """Fills `slots` with the examples around `centres_xyz` (n, 3) of
    `volumes`; raises (and touches no slot) if a patch leaves its volume.  The
    seed is logit(seed_pad) with logit(0.95) at the centre."""
    slots = _i32(slots)
    volumes = _i32(volumes)
    centres = _i32(centres_xyz, (-1, 3))
    offsets = np.ascontiguousarray(offsets, dtype=np.float32)
    scales = np.ascontiguousarray(scales, dtype=np.float32)
    if not (len(slots) == len(volumes) == len(centres) == len(offsets) ==
            len(scales)):
      raise ValueError('one volume, centre, offset and scale per slot')
    with self.lock:
      check(self._lib.ffn_evaluation_load(
          self._h, len(slots), slots.ctypes.data, volumes.ctypes.data,
          centres.ctypes.data, offsets.ctypes.data, scales.ctypes.data,
          float(f32_logit(seed_pad)), float(f32_logit(0.95))))

  def load_augmented(self, slots, volumes, centres_xyz, offsets, scales,
                     perms, reflects, seed_pad: float):
    """load() followed by train.py's PermuteAndReflect on the image and label
    patches: `perms` (n, 3) holds the source axis of each output axis in zyx
    numbering (np.transpose), `reflects` (n, 3) 0 / 1 per output axis.  The
    seed canvas is not transformed.  Raises, touching no slot, on what load()
    refuses, on a perm that is no permutation, and on axes of different patch
    sizes changing places."""
    slots = _i32(slots)
    volumes = _i32(volumes)
    centres = _i32(centres_xyz, (-1, 3))
    offsets = np.ascontiguousarray(offsets, dtype=np.float32)
    scales = np.ascontiguousarray(scales, dtype=np.float32)
    perms = _i32(perms, (-1, 3))
    reflects_in = np.asarray(reflects).reshape(-1, 3)
    if ((reflects_in < 0) | (reflects_in > 255)).any():  # the library sees u8
      raise ValueError('a reflect value is 0 or 1')
    reflects = np.ascontiguousarray(reflects_in, dtype=np.uint8)
    if not (len(slots) == len(volumes) == len(centres) == len(offsets) ==
            len(scales) == len(perms) == len(reflects)):
      raise ValueError('one volume, centre, offset, scale, perm and reflect '
                       'per slot')
    with self.lock:
      check(self._lib.ffn_evaluation_load_augmented(
          self._h, len(slots), slots.ctypes.data, volumes.ctypes.data,
          centres.ctypes.data, offsets.ctypes.data, scales.ctypes.data,
          perms.ctypes.data, reflects.ctypes.data,
          float(f32_logit(seed_pad)), float(f32_logit(0.95))))

  def load_sections(self, slots, volumes, centres_xyz, offsets, scales,
                    perms, reflects, plans, seed_pad: float):
    """load_augmented() with the section augmentations of `plans` (one
    augmentation.SectionPlan per slot) carried out on the device between
    reading the volume and the normalisation: misalignment of image and
    labels, then missing section, out of focus and grayscale perturbation of
    the image (include/ffn_evaluation.h).  Plans without an operation write
    what load_augmented() writes.  Raises, touching no slot, on what
    load_augmented() refuses, on a plan the header refuses, and where the
    patches enlarged by a plan's margins leave their volume."""
    slots = _i32(slots)
    volumes = _i32(volumes)
    centres = _i32(centres_xyz, (-1, 3))
    offsets = np.ascontiguousarray(offsets, dtype=np.float32)
    scales = np.ascontiguousarray(scales, dtype=np.float32)
    perms = _i32(perms, (-1, 3))
    reflects_in = np.asarray(reflects).reshape(-1, 3)
    if ((reflects_in < 0) | (reflects_in > 255)).any():  # the library sees u8
      raise ValueError('a reflect value is 0 or 1')
    reflects = np.ascontiguousarray(reflects_in, dtype=np.uint8)
    plans = list(plans)
    if not (len(slots) == len(volumes) == len(centres) == len(offsets) ==
            len(scales) == len(perms) == len(reflects) == len(plans)):
      raise ValueError('one volume, centre, offset, scale, perm, reflect and '
                       'plan per slot')
    sections = self.geometry.image_patch[0]
    c_plans, c_sections = section_plan_arrays(plans, sections)
    with self.lock:
      check(self._lib.ffn_evaluation_load_sections(
          self._h, len(slots), slots.ctypes.data, volumes.ctypes.data,
          centres.ctypes.data, offsets.ctypes.data, scales.ctypes.data,
          perms.ctypes.data, reflects.ctypes.data,
          c_plans.ctypes.data, c_sections.ctypes.data,
          float(f32_logit(seed_pad)), float(f32_logit(0.95))))

  def last_timing_sections(self) -> Dict[str, Tuple[float, float]]:
    """last_timing() of the last load_sections: the whole call and its first
    launch, the section kernel."""
    ms = (ctypes.c_double * 2)()
    nbytes = (ctypes.c_double * 2)()
    check(self._lib.ffn_evaluation_last_timing_sections(self._h, ms, nbytes))
    return {kind: (ms[k], nbytes[k])
            for k, kind in enumerate(SECTION_CALL_KINDS)}

  def probe_moves(self, slots, offsets_xyz, seed_threshold: float,
                  label_threshold: float):
    """(valid, wanted) bool arrays, one entry per (slot, offset) pair.  The
    thresholds are float64 values; the device gets ceil_f32 of them."""
    slots = _i32(slots)
    offsets = _i32(offsets_xyz, (-1, 3))
    if len(slots) != len(offsets):
      raise ValueError('one offset per slot entry')
    valid = np.zeros(len(slots), np.uint8)
    wanted = np.zeros(len(slots), np.uint8)
    with self.lock:
      check(self._lib.ffn_evaluation_probe_moves(
          self._h, len(slots), slots.ctypes.data, offsets.ctypes.data,
          float(ceil_f32(seed_threshold)), float(ceil_f32(label_threshold)),
          valid.ctypes.data, wanted.ctypes.data))
    return valid.astype(bool), wanted.astype(bool)

  def alloc_io(self, n: int):
    """Three device arrays for n <= slots FoVs, owned by the handle and valid
    until the next configure(): seed [n, input_seed], image [n, input_image],
    logits [n, input_seed] (DeviceArray: `data_ptr()` and `shape`)."""
    g = self.geometry
    if not 1 <= n <= g.slots:
      raise ValueError('%d FoVs for %d slots' % (n, g.slots))
    ptrs = [ctypes.c_void_p() for _ in range(3)]
    with self.lock:
      check(self._lib.ffn_evaluation_io_buffers(
          self._h, *[ctypes.byref(p) for p in ptrs]))
    return (DeviceArray(ptrs[0].value, (n,) + g.input_seed),
            DeviceArray(ptrs[1].value, (n,) + g.input_image),
            DeviceArray(ptrs[2].value, (n,) + g.input_seed))

  def gather(self, slots, offsets_xyz, seed_out, image_out):
    """mask.crop_and_pad of the seed canvas and the image patch of every entry
    into the device arrays `seed_out` / `image_out` (objects with data_ptr(),
    or addresses)."""
    slots = _i32(slots)
    offsets = _i32(offsets_xyz, (-1, 3))
    with self.lock:
      check(self._lib.ffn_evaluation_gather(
          self._h, len(slots), slots.ctypes.data, offsets.ctypes.data,
          _address(seed_out), _address(image_out)))

  def alloc_io_train(self, n: int):
    """alloc_io()'s three arrays and a fourth for the labels of gather_train:
    [n, pred_mask]."""
    seed, image, logits = self.alloc_io(n)
    ptr = ctypes.c_void_p()
    with self.lock:
      check(self._lib.ffn_evaluation_io_labels(self._h, ctypes.byref(ptr)))
    return seed, image, logits, DeviceArray(ptr.value,
                                            (n,) + self.geometry.pred_mask)

  def gather_train(self, slots, offsets_xyz, seed_out, image_out, labels_out):
    """gather(), and the pred_mask crop of every entry's soft labels at its
    offset (examples.py:65) into the device array `labels_out`."""
    slots = _i32(slots)
    offsets = _i32(offsets_xyz, (-1, 3))
    with self.lock:
      check(self._lib.ffn_evaluation_gather_train(
          self._h, len(slots), slots.ctypes.data, offsets.ctypes.data,
          _address(seed_out), _address(image_out), _address(labels_out)))

  def paste(self, slots, offsets_xyz, logits, layout: int = LOGITS_PRED):
    """BatchExampleIter.update_seeds from the device array `logits`: dense
    [n, pred_mask] (LOGITS_PRED) or [n, input_seed] (LOGITS_FOV)."""
    slots = _i32(slots)
    offsets = _i32(offsets_xyz, (-1, 3))
    with self.lock:
      check(self._lib.ffn_evaluation_paste(
          self._h, len(slots), slots.ctypes.data, offsets.ctypes.data,
          _address(logits), int(layout)))

  def score_faces(self, slots, offsets_xyz):
    """(scores (n, 6) f32, positions (n, 6, 3) int32 zyx relative to the centre
    of the pred_mask crop at the offset), faces in z-, z+, y-, y+, x-, x+
    order."""
    slots = _i32(slots)
    offsets = _i32(offsets_xyz, (-1, 3))
    scores = np.empty((len(slots), 6), np.float32)
    positions = np.empty((len(slots), 6, 3), np.int32)
    with self.lock:
      check(self._lib.ffn_evaluation_score_faces(
          self._h, len(slots), slots.ctypes.data, offsets.ctypes.data,
          scores.ctypes.data, positions.ctypes.data))
    return scores, positions

  def finish(self, slot: int, pred_threshold: Optional[float] = None):
    """EvalTracker.add_patch of a slot -> (loss sum f32, [tp, tn, fp, fn],
    masked voxels)."""
    if pred_threshold is None:
      pred_threshold = logit(EVAL_PROBABILITY)
    loss = ctypes.c_float(0.0)
    counts = (ctypes.c_int64 * 4)()
    masked = ctypes.c_int64(0)
    with self.lock:
      check(self._lib.ffn_evaluation_finish(
          self._h, int(slot), float(ceil_f32(pred_threshold)),
          ctypes.byref(loss), counts, ctypes.byref(masked)))
    return float(loss.value), [int(c) for c in counts], int(masked.value)

  def _read(self, name: str, slot: int, shape):
    out = np.empty(shape, np.float32)
    with self.lock:
      check(getattr(self._lib, name)(self._h, int(slot), out.ctypes.data))
    return out

  def read_seed(self, slot: int) -> np.ndarray:
    return self._read('ffn_evaluation_read_seed', slot, self.geometry.canvas)

  def read_labels(self, slot: int) -> np.ndarray:
    return self._read('ffn_evaluation_read_labels', slot,
                      self.geometry.label_patch)

  def read_image(self, slot: int) -> np.ndarray:
    return self._read('ffn_evaluation_read_image', slot,
                      self.geometry.image_patch)

  def write_seed(self, slot: int, seed: np.ndarray):
    seed = np.ascontiguousarray(seed, dtype=np.float32)
    if seed.shape != self.geometry.canvas:
      raise ValueError('a seed canvas is %r, got %r' %
                       (self.geometry.canvas, seed.shape))
    with self.lock:
      check(self._lib.ffn_evaluation_write_seed(self._h, int(slot),
                                                seed.ctypes.data))

  def last_timing(self) -> Dict[str, Tuple[float, float]]:
    """{call kind: (kernel ms, algorithmic bytes)} of the last calls."""
    ms = (ctypes.c_double * 6)()
    nbytes = (ctypes.c_double * 6)()
    check(self._lib.ffn_evaluation_last_timing(self._h, ms, nbytes))
    return {kind: (ms[k], nbytes[k]) for k, kind in enumerate(CALL_KINDS)}

  def last_timing_train(self) -> Dict[str, Tuple[float, float]]:
    """last_timing() of the last load_augmented and gather_train."""
    ms = (ctypes.c_double * 2)()
    nbytes = (ctypes.c_double * 2)()
    check(self._lib.ffn_evaluation_last_timing_train(self._h, ms, nbytes))
    return {kind: (ms[k], nbytes[k])
            for k, kind in enumerate(TRAIN_CALL_KINDS)}


def _address(array) -> int:
  return int(array.data_ptr()) if hasattr(array, 'data_ptr') else int(array)


_default = _unit.Registry(EvaluationOps)


def default_ops(device_id: int = 0) -> EvaluationOps:
  """Process-wide EvaluationOps of a device (created on first use)."""
  return _default.get(device_id)


# ---- accumulators ------------------------------------------------------------------


class EvalResult:
  """The accumulators of the reference's EvalTracker (tracker.py:100-114).

  moves / moves_by_r[r]: [correct, missed, spurious]; num_voxels: [total,
  masked]; prediction_counts: [tp, tn, fp, fn]; fov_stats: [total voxels, masked
  voxels, weight sum] of the FoVs handed to the network.  `loss` is the sum of
  the per-patch mean losses, kept in float64 (the reference keeps a float32).
  `offsets` and `records` list, per finished example in the order of the
  coordinates, the offsets taken and the (wanted, valid, offset) triples
  recorded.
  """

  def __init__(self, shifts=()):
    self.moves = [0, 0, 0]
    radii = {int(np.linalg.norm(s)) for s in shifts} | {0}
    self.moves_by_r = {r: [0, 0, 0] for r in sorted(radii)}
    self.loss = 0.0
    self.num_patches = 0
    self.num_voxels = [0, 0]
    self.prediction_counts = [0, 0, 0, 0]
    self.fov_stats = [0.0, 0.0, 0.0]
    self.skipped = 0
    self.offsets: List[List[Tuple[int, int, int]]] = []
    self.records: List[List[Tuple[bool, bool, Tuple[int, int, int]]]] = []

  def record_move(self, wanted: bool, executed: bool, offset_xyz):
    """EvalTracker.record_move."""
    r = int(np.linalg.norm(offset_xyz))
    if r not in self.moves_by_r:
      raise ValueError('%d not in %r' % (r, list(self.moves_by_r)))
    kind = (0 if executed else 1) if wanted else (2 if executed else None)
    if kind is not None:
      self.moves[kind] += 1
      self.moves_by_r[r][kind] += 1

  def track_weights(self, num_voxels: int):
    """EvalTracker.track_weights of all-one weights."""
    self.fov_stats[0] += num_voxels
    self.fov_stats[2] += num_voxels

  def add_patch(self, mean_loss: float, counts, num_voxels: int, masked: int):
    self.loss += float(mean_loss)
    self.num_voxels[0] += int(num_voxels)
    self.num_voxels[1] += int(masked)
    for k in range(4):
      self.prediction_counts[k] += int(counts[k])
    self.num_patches += 1

  def summaries(self) -> Dict[str, float]:
    """The scalar summaries of EvalTracker.get_summaries under its tags
    (tracker.py:325-440); {} before any patch, as there."""
    if not self.num_voxels[0]:
      return {}
    out = {}
    total_moves = max(sum(self.moves), 1)
    out['fov/masked_voxel_fraction'] = self.fov_stats[1] / max(
        self.fov_stats[0], 1)
    out['fov/average_weight'] = self.fov_stats[2] / max(self.fov_stats[0], 1)
    out['masked_voxel_fraction'] = self.num_voxels[1] / self.num_voxels[0]
    out['eval/patch_loss'] = self.loss / self.num_patches
    out['eval/patches'] = self.num_patches
    out['moves/total'] = total_moves
    for k, name in enumerate(('correct', 'missed', 'spurious')):
      out['moves/all/%s' % name] = self.moves[k] / total_moves
    tp, tn, fp, fn = self.prediction_counts
    precision = tp / max(tp + fp, 1)
    recall = tp / max(tp + fn, 1)
    if precision > 0 or recall > 0:
      f1 = 2.0 * precision * recall / (precision + recall)
    else:
      f1 = 0.0
    out['eval/all/accuracy'] = (tp + tn) / max(tp + tn + fp + fn, 1)
    out['eval/all/precision'] = precision
    out['eval/all/recall'] = recall
    out['eval/all/specificity'] = tn / max(tn + fp, 1)
    out['eval/all/f1'] = f1
    for r, r_moves in self.moves_by_r.items():
      total = max(sum(r_moves), 1)
      out['moves/r=%d/correct' % r] = r_moves[0] / total
      out['moves/r=%d/spurious' % r] = r_moves[2] / total
      out['moves/r=%d/missed' % r] = r_moves[1] / total
      out['moves/r=%d/total' % r] = total
    return out

  def accumulators(self) -> dict:
    """JSON-ready copy of the raw accumulators."""
    return {
        'moves': list(self.moves),
        'moves_by_r': {str(r): list(v) for r, v in self.moves_by_r.items()},
        'loss': self.loss,
        'num_patches': self.num_patches,
        'num_voxels': list(self.num_voxels),
        'prediction_counts': list(self.prediction_counts),
        'fov_stats': list(self.fov_stats),
        'skipped': self.skipped,
    }


# ---- the loop ----------------------------------------------------------------------


class _Stream:
  """Host state of one slot: the example it holds and what its move policy
  keeps between two steps."""

  def __init__(self):
    self.example = None   # index into the coordinate list, None = idle
    self.pending = None   # offsets still to try: a list (fixed) or a deque
    self.done = None      # quantised offsets taken (max_pred_moves)
    self.offset = None    # offset of the step being made


class FovWalk:
  """The host halves of the move policies of train.py:359-373
  (examples.fixed_offsets, max_pred_offsets, no_offsets): which offsets a
  stream may ask the device about, which one it takes next, and what it queues
  after a step.  Shared by CheckpointEvaluator and examples.BatchExampleIter.

  `result` arguments are anything with EvalResult.record_move."""

  def __init__(self, fov_policy: str, geometry: Geometry, shifts, deltas_xyz,
               threshold: float):
    if fov_policy not in POLICIES:
      raise ValueError('fov_policy is one of %r, got %r' %
                       (POLICIES, fov_policy))
    self.fov_policy = fov_policy
    self.shifts = [tuple(int(v) for v in s) for s in shifts]
    self.deltas_xyz = tuple(int(v) for v in deltas_xyz)
    self.deltas_zyx = tuple(geometry.deltas)
    self.max_radius = geometry.max_radius_xyz()
    self.threshold = float(threshold)  # of the seed, in logits

  @staticmethod
  def new_stream() -> _Stream:
    """The host state of one slot, idle."""
    return _Stream()

  def start(self, stream: _Stream, example: int):
    stream.example = example
    stream.offset = None
    if self.fov_policy == 'fixed':
      stream.pending = [(0, 0, 0)] + self.shifts
    elif self.fov_policy == 'max_pred_moves':
      stream.pending = collections.deque([(0, 0, 0)])
      stream.done = set()
    else:
      stream.pending = [(0, 0, 0)]

  def quantize(self, offset):
    d = self.deltas_xyz
    return tuple((o + dd / 2) // max(dd, 1) for o, dd in zip(offset, d))

  def candidates(self, stream: _Stream):
    """The pending offsets whose seed and label values the next walk may ask
    for: the seed does not change before the stream's next step."""
    if self.fov_policy == 'fixed':
      return list(stream.pending)
    if self.fov_policy == 'max_pred_moves':
      return [o for o in stream.pending
              if not any(abs(v) > m for v, m in zip(o, self.max_radius))]
    return []

  def next_offset(self, stream: _Stream, probed, result: EvalResult, records):
    """Walks the pending offsets as the policy's generator does until one is to
    be taken; returns it, or None when the example is exhausted."""
    if self.fov_policy == 'no_step':
      if not stream.pending:
        return None
      stream.pending = []
      result.record_move(True, True, (0, 0, 0))
      records.append((True, True, (0, 0, 0)))
      return (0, 0, 0)
    if self.fov_policy == 'fixed':
      while stream.pending:
        off = stream.pending.pop(0)
        valid, wanted = probed[off]
        result.record_move(wanted, valid, off)
        records.append((wanted, valid, off))
        if valid:
          return off
      return None
    while stream.pending:
      off = stream.pending.popleft()
      if any(abs(v) > m for v, m in zip(off, self.max_radius)):
        continue
      quantized = self.quantize(off)
      if quantized in stream.done:
        continue
      valid, wanted = probed[off]
      result.record_move(wanted, valid, (0, 0, 0))
      records.append((wanted, valid, (0, 0, 0)))
      if not valid or (not wanted and quantized != (0, 0, 0)):
        continue
      stream.done.add(quantized)
      return off
    return None

  def extend_queue(self, stream: _Stream, scores, positions):
    """max_pred_offsets' tail: the face maxima at or above the threshold,
    highest first, queued relative to the step's offset."""
    found = set()
    for f in range(6):
      if self.deltas_zyx[f // 2] == 0:
        continue
      score = scores[f]
      if score < ceil_f32(self.threshold):
        continue
      found.add((float(score), tuple(int(v) for v in positions[f])))
    off = stream.offset
    for _, p in sorted(found, reverse=True):
      stream.pending.append((p[2] + off[0], p[1] + off[1], p[0] + off[2]))


class CheckpointEvaluator:
  """Scores a checkpoint on a finite list of training coordinates.

  model: carries `info` (ModelInfo) and `shifts`; its weights are already in
    `engine`.
  engine: `predict_device(n, seed, image, logits)` on device arrays
    (HipEngine, max_batch >= batch_size; with pred_mask < input_seed it is
    already set with set_pred_size).
  ops: an EvaluationOps (or an object with its methods).
  fov_policy: 'fixed', 'max_pred_moves' or 'no_step' (train.py:359-373).
  shifts: the moves of 'fixed' in the order to try them, (x, y, z); default
    `model.shifts`.  train.py shuffles them with Python's `random` when
    --shuffle_moves is set; here the caller passes the list it wants, or
    `shuffle_seed`, which shuffles with random.Random(shuffle_seed).

  Volumes are added with add_volume(); evaluate() then runs the coordinates.
  Creating an evaluator configures `ops` and drops the volumes it held: an
  EvaluationOps serves one evaluator at a time.
  Every slot is an independent example stream, as in the reference's
  `_batch_gen`: it takes the next coordinate when its offsets are exhausted, so
  which examples share a batch depends on `batch_size`, but what happens to an
  example does not.  The last steps run with fewer than batch_size FoVs.
  """

  def __init__(self, model, engine, ops, fov_policy: str, fov_moves: int,
               threshold: float = 0.9, seed_pad: float = 0.05,
               batch_size: int = 1, shifts: Optional[Sequence] = None,
               shuffle_seed: Optional[int] = None):
    if not 1 <= int(batch_size) <= MAX_SLOTS:
      raise ValueError('batch_size must be in [1, %d]' % MAX_SLOTS)
    self.model = model
    self.engine = engine
    self.ops = ops
    self.fov_policy = fov_policy
    self.batch_size = int(batch_size)
    self.geometry = Geometry.from_info(model.info, fov_policy, fov_moves,
                                       self.batch_size)
    self.seed_pad = float(seed_pad)
    self.threshold = logit(threshold)            # of the seed, in logits
    self.label_threshold = expit(self.threshold)  # of the soft labels
    shifts = list(model.shifts if shifts is None else shifts)
    self.shifts = [tuple(int(v) for v in s) for s in shifts]
    if shuffle_seed is not None:
      random.Random(shuffle_seed).shuffle(self.shifts)
    self.deltas_xyz = tuple(int(v) for v in np.asarray(model.info.deltas))
    self.max_radius = self.geometry.max_radius_xyz()
    self.walk = FovWalk(fov_policy, self.geometry, self.shifts,
                        self.deltas_xyz, self.threshold)
    self._volumes = {}
    ops.configure(self.geometry)
    ops.reset()  # the unit serves one evaluator at a time
    self._io = ops.alloc_io(self.batch_size)
    self._layout = (EvaluationOps.LOGITS_FOV
                    if self.geometry.pred_mask != self.geometry.input_seed
                    else EvaluationOps.LOGITS_PRED)
    #: seconds inside engine.predict_device / in the whole of evaluate()
    self.forward_seconds = 0.0
    self.total_seconds = 0.0
    self.steps = 0

  def add_volume(self, name: str, image, labels, offset: float, scale: float):
    """A named volume pair and the normalisation of its image:
    (float(v) - offset) / scale (train.py:270-274)."""
    index = self.ops.add_volume(image, labels)
    self._volumes[name] = (index, tuple(np.asarray(image).shape), float(offset),
                           float(scale))

  def fits(self, centre_xyz, name: str) -> bool:
    """Whether the image and label patches around a centre stay inside the
    volume (the reference would fail in a reshape otherwise)."""
    shape = self._volumes[name][1]
    for axis in range(3):
      c = int(centre_xyz[2 - axis])
      for size in (self.geometry.image_patch[axis],
                   self.geometry.label_patch[axis]):
        start = c - (size - 1) // 2
        if start < 0 or start + size > shape[axis]:
          return False
    return True

  # -- the loop ----------------------------------------------------------------------

  def evaluate(self, coordinates, max_examples: Optional[int] = None
               ) -> EvalResult:
    """coordinates: (centre (x, y, z), volume name) pairs.  Those whose patches
    leave their volume are skipped and counted in `result.skipped`."""
    t_begin = time.time()
    result = EvalResult(self.shifts)
    todo = []
    for centre, name in coordinates:
      if name not in self._volumes:
        raise KeyError('no volume named %r' % (name,))
      if not self.fits(centre, name):
        result.skipped += 1
        continue
      todo.append((tuple(int(v) for v in centre), name))
      if max_examples is not None and len(todo) >= max_examples:
        break
    result.offsets = [[] for _ in todo]
    result.records = [[] for _ in todo]
    streams = [self.walk.new_stream() for _ in range(self.batch_size)]
    next_example = 0
    eval_voxels = int(np.prod(self.geometry.eval))
    pred_voxels = int(np.prod(self.geometry.pred_mask))
    seed_io, image_io, logits_io = self._io

    while True:
      # every slot gets its next offset, taking new examples as needed
      need = list(range(self.batch_size))
      while need:
        fresh = []
        for s in need:
          if streams[s].example is None and next_example < len(todo):
            self.walk.start(streams[s], next_example)
            fresh.append(s)
            next_example += 1
        if fresh:
          rows = [todo[streams[s].example] for s in fresh]
          vols = [self._volumes[name] for _, name in rows]
          self.ops.load(fresh, [v[0] for v in vols], [c for c, _ in rows],
                        [v[2] for v in vols], [v[3] for v in vols],
                        self.seed_pad)
        need = [s for s in need if streams[s].example is not None]
        pairs = [(s, o) for s in need for o in self.walk.candidates(streams[s])]
        probed = {s: {} for s in need}
        if pairs:
          valid, wanted = self.ops.probe_moves(
              [s for s, _ in pairs], [o for _, o in pairs], self.threshold,
              self.label_threshold)
          for (s, o), v, w in zip(pairs, valid, wanted):
            probed[s][o] = (bool(v), bool(w))
        again = []
        for s in need:
          stream = streams[s]
          stream.offset = self.walk.next_offset(stream, probed[s], result,
                                                result.records[stream.example])
          if stream.offset is None:
            loss_sum, counts, masked = self.ops.finish(s)
            result.add_patch(loss_sum / eval_voxels, counts, eval_voxels,
                             masked)
            stream.example = None
            again.append(s)
          else:
            result.offsets[stream.example].append(stream.offset)
        need = again if next_example < len(todo) else []

      active = [s for s in range(self.batch_size)
                if streams[s].example is not None]
      if not active:
        break
      n = len(active)
      offsets = [streams[s].offset for s in active]
      self.ops.gather(active, offsets, seed_io, image_io)
      t0 = time.time()
      self.engine.predict_device(n, seed_io, image_io, logits_io)
      self.forward_seconds += time.time() - t0
      self.ops.paste(active, offsets, logits_io, self._layout)
      result.track_weights(n * pred_voxels)
      self.steps += 1
      if self.fov_policy == 'max_pred_moves':
        scores, positions = self.ops.score_faces(active, offsets)
        for k, s in enumerate(active):
          self.walk.extend_queue(streams[s], scores[k], positions[k])
    self.total_seconds += time.time() - t_begin
    return result
