"""Numpy restatement of the section augmentations of
ffn_evaluation_load_sections (include/ffn_evaluation.h), written the way the
reference's ffn/training/augmentation.py words them -- np.pad, np.roll and a
centre crop for the misalignment, slices for the quadrants,
scipy.ndimage.correlate1d for the blur -- and so independent of the index
arithmetic of ffn_amd/training/augmentation.apply_sections.  `RefOps` adds
load_sections to tests/training_ref.RefOps, `run_loop` restates the training
loop with section plans, and `within` is the yardstick of DESIGN.md 10.5 / 10.8.

A plan is anything with the attributes of augmentation.SectionPlan.
"""
import numpy as np
from scipy import ndimage

from tests import evaluation_ref
from tests import training_ref

FACTOR = 4.0


# ---- the four operations -----------------------------------------------------------


def padded_size(image_zyx, label_zyx, margin_yx):
  loaded = [(s[0], s[1] + 2 * margin_yx[0], s[2] + 2 * margin_yx[1])
            for s in (image_zyx, label_zyx)]
  return tuple(max(a, b) for a, b in zip(*loaded))


def edge_pad(box, m):
  pad = [((t - s) // 2, t - s - (t - s) // 2) for s, t in zip(box.shape, m)]
  return np.pad(box, pad, 'edge')


def centre_crop(box, final_zyx):
  start = [(s - f) // 2 for s, f in zip(box.shape, final_zyx)]
  return box[tuple(slice(a, a + f) for a, f in zip(start, final_zyx))]


def misalign(box, final_zyx, m, plan):
  """box: what was read from the volume (the final size plus the margins)."""
  padded = edge_pad(np.asarray(box), m).copy()
  if plan.kind == 1:
    sel = slice(plan.z0, plan.z0 + 1)
  elif plan.kind == 2:
    sel = slice(plan.z0, None)
  else:
    sel = slice(0, 0)
  padded[sel] = np.roll(padded[sel], plan.dy, 1)
  padded[sel] = np.roll(padded[sel], -plan.dx, 2)
  return np.ascontiguousarray(centre_crop(padded, final_zyx))


def quadrant_slices(mask, yx):
  y, x = int(yx[0]), int(yx[1])
  regions = [(slice(0, y), slice(0, x)), (slice(y, None), slice(0, x)),
             (slice(0, y), slice(x, None)), (slice(y, None), slice(x, None))]
  return [r for k, r in enumerate(regions) if (int(mask) >> k) & 1]


def touched(plan, shape_yx, which):
  """bool [z, y, x]: the voxels `which` ('blank', 'blur' or 'gray') writes."""
  out = np.zeros((plan.sections,) + tuple(shape_yx), bool)
  for z in range(plan.sections):
    if which == 'gray':
      out[z] = bool(plan.gray[z])
      continue
    if which == 'blur' and blur_radius(plan.blur_sigma) == 0:
      continue
    mask, yx = ((plan.blank_mask, plan.blank_yx) if which == 'blank' else
                (plan.blur_mask, plan.blur_yx))
    for r in quadrant_slices(mask[z], yx[z]):
      out[z][r] = True
  return out


def blur_radius(sigma):
  return int(4.0 * float(sigma) + 0.5)


def gaussian_kernel(sigma):
  """scipy.ndimage's _gaussian_kernel1d at order 0, truncate 4."""
  sigma = float(sigma)
  radius = blur_radius(sigma)
  x = np.arange(-radius, radius + 1)
  phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
  return phi / phi.sum()


def blur(plane, sigma):
  """gaussian_filter of a [y, x] plane in its own dtype: along y, then x."""
  if blur_radius(sigma) == 0:
    return plane.copy()
  kernel = gaussian_kernel(sigma)
  tmp = ndimage.correlate1d(plane, kernel, 0, output=plane.dtype,
                            mode='reflect')
  return ndimage.correlate1d(tmp, kernel, 1, output=plane.dtype,
                             mode='reflect')


def perturb(plane, contrast, brightness, gamma):
  """grayscale_perturb's perturb_fn: float32 whatever the plane's dtype."""
  f = np.float32
  unit = plane.astype(f) / f(255)
  shifted = unit * f(contrast) + f(brightness)
  powered = np.clip(shifted, f(0), f(1)) ** f(gamma)
  return (powered * f(255)).astype(plane.dtype)


def apply(image_box, label_box, plan, image_zyx, label_zyx, dtype=np.float32):
  """-> (image of the final size in `dtype`, before the normalisation; label
  ids of the final size)."""
  m = padded_size(image_zyx, label_zyx, plan.margin_yx)
  image = misalign(np.asarray(image_box).astype(dtype), image_zyx, m, plan)
  labels = misalign(label_box, label_zyx, m, plan)
  for z in range(plan.sections):
    for r in quadrant_slices(plan.blank_mask[z], plan.blank_yx[z]):
      image[z][r] = dtype(plan.blank_value)
    if plan.blur_mask[z]:
      blurred = blur(image[z], plan.blur_sigma)
      for r in quadrant_slices(plan.blur_mask[z], plan.blur_yx[z]):
        image[z][r] = blurred[r]
    if plan.gray[z]:
      image[z] = perturb(image[z], *plan.factors[z])
  return image, labels


# ---- the yardstick -----------------------------------------------------------------


def e_ref(ref32, ref64):
  """max |f32 - f64| of a case, at least one f32 ulp of its largest
  magnitude."""
  ref64 = np.asarray(ref64, np.float64)
  spread = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
  ulp = float(np.spacing(np.float32(np.abs(ref64).max())))
  return max(spread, ulp)


def within(got, ref32, ref64, exact, e=None):
  """-> (passes, distance, bound): bit-equal to ref32 where `exact` (bool
  array) is set, and max |got - ref64| <= 4 E_ref everywhere; E_ref is `e`, or
  that of ref32 and ref64."""
  got = np.asarray(got)
  bound = FACTOR * (e_ref(ref32, ref64) if e is None else e)
  distance = float(np.abs(got.astype(np.float64) -
                          np.asarray(ref64, np.float64)).max())
  same = np.array_equal(got[exact], np.asarray(ref32)[exact])
  return bool(same and distance <= bound), distance, bound


# ---- the unit's call ---------------------------------------------------------------


def box_of(volume, centre_xyz, final_zyx, margin_yx):
  size = (final_zyx[0], final_zyx[1] + 2 * margin_yx[0],
          final_zyx[2] + 2 * margin_yx[1])
  sel = []
  for axis in range(3):
    margin = 0 if axis == 0 else margin_yx[axis - 1]
    start = int(centre_xyz[2 - axis]) - (final_zyx[axis] - 1) // 2 - margin
    if start < 0 or start + size[axis] > volume.shape[axis]:
      raise ValueError('patch leaves the volume')
    sel.append(slice(start, start + size[axis]))
  return volume[tuple(sel)]


def load_sections(image_volume, label_volume, centre_xyz, offset, scale, geom,
                  perm, reflect, plan, seed_pad=0.05, dtype=np.float32):
  """-> (image, labels, seed) as the slot holds them.  With dtype float64 the
  image is the float64 statement (the normalisation in float64 too)."""
  _, plain_labels, seed = evaluation_ref.load(
      image_volume, label_volume, centre_xyz, offset, scale, geom, seed_pad)
  del plain_labels
  ip, lp = geom['image_patch'], geom['label_patch']
  image, ids = apply(box_of(image_volume, centre_xyz, ip, plan.margin_yx),
                     box_of(label_volume, centre_xyz, lp, plan.margin_yx),
                     plan, ip, lp, dtype)
  centre = evaluation_ref.patch_of(label_volume, centre_xyz, lp)[
      tuple(s // 2 for s in lp)]
  labels = np.where((ids > 0) & (ids == centre), np.float32(0.95),
                    np.float32(0.05)).astype(np.float32)
  image = (image - dtype(offset)) / dtype(scale)
  for a in range(3):
    if perm[a] != a and (ip[a] != ip[perm[a]] or lp[a] != lp[perm[a]]):
      raise ValueError('axes of different size change places')
  return (training_ref.transform(image, perm, reflect),
          training_ref.transform(labels, perm, reflect), seed)


def untouched(plan, geom, perm, reflect):
  """bool, in slot layout: the image voxels neither blur nor gray writes."""
  shape_yx = geom['image_patch'][1:]
  keep = ~(touched(plan, shape_yx, 'blur') | touched(plan, shape_yx, 'gray'))
  return training_ref.transform(keep, perm, reflect)


class RefOps(training_ref.RefOps):
  """EvaluationOps with load_sections, on numpy arrays."""

  def load_sections(self, slots, volumes, centres_xyz, offsets, scales, perms,
                    reflects, plans, seed_pad):
    self.calls['load_sections'] += 1
    loaded = [load_sections(*self.volumes[v], c, o, s, self.geom, p, r, plan,
                            seed_pad)
              for v, c, o, s, p, r, plan in zip(volumes, centres_xyz, offsets,
                                                scales, perms, reflects, plans)]
    for slot, arrays in zip(slots, loaded):
      self.slots[slot] = list(arrays)


# ---- the loop with section plans, one generator per slot ----------------------------


def example_stream(slot, source, geom, threshold, shifts, seed_pad, log):
  """training_ref.example_stream's 'fixed' policy with a section plan per
  example.  `source()` -> (index, image volume, label volume, centre, offset,
  scale, perm, reflect, plan)."""
  from scipy import special
  seed_thr = special.logit(threshold)
  label_thr = special.expit(seed_thr)
  lo = [(a - p) // 2 for a, p in zip(geom['input_seed'], geom['pred_mask'])]
  inner = tuple(slice(l, l + p) for l, p in zip(lo, geom['pred_mask']))
  while True:
    (index, image_volume, label_volume, centre, offset, scale, perm, reflect,
     plan) = source()
    image, labels, seed = load_sections(image_volume, label_volume, centre,
                                        offset, scale, geom, perm, reflect,
                                        plan, seed_pad)
    entry = {'coordinate': index, 'slot': slot, 'perm': tuple(perm),
             'reflect': tuple(reflect), 'plan': plan, 'offsets': [],
             'records': [], 'image': image, 'labels': labels, 'seed': seed}
    log.append(entry)
    for off in [(0, 0, 0)] + list(shifts):
      valid, wanted = evaluation_ref.probe(seed, labels, off, seed_thr,
                                           label_thr)
      entry['records'].append((bool(wanted), bool(valid), tuple(off)))
      if valid:
        entry['offsets'].append(tuple(int(v) for v in off))
        window = evaluation_ref.crop(seed, off, geom['input_seed'])
        yield (window[inner],
               evaluation_ref.crop(image, off, geom['input_image']),
               evaluation_ref.crop(labels, off, geom['pred_mask']))


def run_loop(forward, volumes, coordinates, transforms, plans, geom,
             batch_size, steps, threshold=0.9, seed_pad=0.05):
  """The loop of train.py:384-412 with `forward(seed, image)` -> logits as the
  train step; coordinates, transforms and plans are taken in turn per example
  started.  -> the log of examples, in starting order."""
  shifts = evaluation_ref.model_shifts(geom['deltas'][::-1])
  log = []

  def source():
    k = len(log)
    centre, name = coordinates[k % len(coordinates)]
    perm, reflect = transforms[k % len(transforms)]
    image_volume, label_volume, offset, scale = volumes[name]
    return (k % len(coordinates), image_volume, label_volume, centre, offset,
            scale, perm, reflect, plans[k])

  streams = [example_stream(s, source, geom, threshold, shifts, seed_pad, log)
             for s in range(batch_size)]
  for _ in range(steps):
    batch = [next(g) for g in streams]  # in slot order
    logits = forward(np.stack([b[0] for b in batch]),
                     np.stack([b[1] for b in batch]))
    for k, b in enumerate(batch):
      b[0][...] = logits[k]
  return log
