"""The basic augmentation of the reference's train.py: a random permutation of
some axes and a random reflection of some (augmentation.PermuteAndReflect,
train.py:262-267), for [z, y, x] arrays.

The reference samples both inside the TensorFlow graph (tf.random.shuffle and
tf.random.uniform) and applies them to rank-5 tensors, so train.py adds 1 to its
--permutable_axes / --reflectable_axes flags for the batch axis.  Here the axes
are the flags' own zyx numbers, the decisions come from a
numpy.random.Generator, and the transform itself runs on the device
(EvaluationOps.load_augmented); `apply` is the same transform in numpy for
hosts and tests.  TensorFlow's random number stream is NOT reproduced: a seed
gives a reproducible run of this package, not the reference's sequence of
transforms.  The distribution is the same (a uniform permutation of the
permutable axes, independent fair coins for the reflectable ones).

The section augmentations of the reference's augmentation.py (after Lee et
al., SNEMI3D) -- misalignment, missing_section, out_of_focus_section and
grayscale_perturb -- are sampled by `SectionAugmentations` and carried out on
the device by EvaluationOps.load_sections, before the normalisation and the
permutation (include/ffn_evaluation.h has the exact definition;
`apply_sections` is the same in numpy).  Their decisions come from a legacy
numpy.random.RandomState in the reference's order, so that under one seed they
ARE the reference's decisions (the reference draws from the global np.random).
The arithmetic is float32 on the voxel converted to float32; the truncation
the reference's functions perform on a uint8 patch is not reproduced, and
neither is misalignment's `mask` argument (every loss weight is one).

Not implemented, for want of anything to check them against: elastic_warp and
affine_transform (skimage.transform.warp), apply_rotation
(multidim_image_augmentation) and random_contrast_brightness_adjustment
(tf.image).
"""

from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

RANK = 3
#: the keys of a SectionAugmentations config, per augmentation
SECTION_KEYS = {
    'misalignment': ('misalignment_skip_ratio', 'max_xy_offset',
                     'slip_vs_translate_ratio'),
    'missing_section': ('missing_section_skip_ratio',
                        'max_missing_section_indices_ratio'),
    'out_of_focus': ('outoffocus_skip_ratio', 'max_outoffocus_indices_ratio',
                     'max_filter_stdev'),
    'grayscale': ('grayscale_skip_ratio', 'max_contrast_factor',
                  'max_brightness_factor'),
}
#: keys of apply_section_augmentations this package cannot honour
UNSUPPORTED_SECTION_KEYS = {
    'elastic_warp_skip_ratio': 'elastic_warp', 'max_warp_indices_ratio':
    'elastic_warp', 'num_control_points_ratio': 'elastic_warp',
    'deformation_stdev_ratio': 'elastic_warp',
    'affine_transform_skip_ratio': 'affine_transform',
    'max_affine_transform_indices_ratio': 'affine_transform',
    'rotation_max': 'affine_transform', 'scale_max': 'affine_transform',
    'shear_max': 'affine_transform',
}
# the reference's defaults (augmentation.py: missing_section,
# out_of_focus_section, grayscale_perturb)
FULL_PROB = 0.5
QUADRANT_PROB = 0.5
MAX_FILL_VAL = 256
MAX_VAL = 255
MAX_BLUR_RADIUS = 31
MAX_BLUR_PLANE = 128 * 128
NONE, SLIP, TRANSLATION = 0, 1, 2


class PermuteAndReflect:
  """Samples (perm, reflect) pairs.

  perm: 3 ints, the source axis of each output axis (np.transpose); the
    identity off `permutable_axes`.
  reflect: 3 values 0 / 1, whether each output axis is reversed after the
    permutation; 0 off `reflectable_axes`.
  """

  def __init__(self, permutable_axes: Sequence[int],
               reflectable_axes: Sequence[int], rng=None):
    permutable_axes = [int(x) for x in permutable_axes]
    reflectable_axes = [int(x) for x in reflectable_axes]
    # (augmentation.py:439-447 with rank = 3)
    if len(set(permutable_axes)) != len(permutable_axes):
      raise ValueError('permutable_axes must not contain duplicates')
    if len(set(reflectable_axes)) != len(reflectable_axes):
      raise ValueError('reflectable_axes must not contain duplicates')
    if not all(0 <= x < RANK for x in permutable_axes):
      raise ValueError('permutable_axes must be a subset of [0, rank-1].')
    if not all(0 <= x < RANK for x in reflectable_axes):
      raise ValueError('reflectable_axes must be a subset of [0, rank-1].')
    self.permutable_axes = np.array(permutable_axes, dtype=np.int32)
    self.reflectable_axes = np.array(reflectable_axes, dtype=np.int32)
    if rng is None or isinstance(rng, (int, np.integer)):
      rng = np.random.default_rng(rng)
    self.rng = rng

  def sample(self) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """One transform: reflection decisions first, then the permutation, as the
    reference's constructor orders them."""
    reflect = [0] * RANK
    if self.reflectable_axes.size > 0:
      decisions = self.rng.random(len(self.reflectable_axes)) > 0.5
      for axis, decision in zip(self.reflectable_axes, decisions):
        reflect[int(axis)] = int(decision)
    full_permutation = list(range(RANK))
    if self.permutable_axes.size > 0:
      permutation = self.rng.permutation(self.permutable_axes)
      for i, d in enumerate(self.permutable_axes):
        full_permutation[int(d)] = int(permutation[i])
    return tuple(full_permutation), tuple(reflect)


def check_transform(perm, reflect):
  perm = tuple(int(p) for p in perm)
  reflect = tuple(int(r) for r in reflect)
  if sorted(perm) != list(range(RANK)):
    raise ValueError('%r is not a permutation of 0, 1, 2' % (perm,))
  if len(reflect) != RANK or any(r not in (0, 1) for r in reflect):
    raise ValueError('reflect holds three values 0 / 1, got %r' % (reflect,))
  return perm, reflect


def apply(x: np.ndarray, perm, reflect) -> np.ndarray:
  """flip(transpose(x, perm), axes with reflect = 1) of a [z, y, x] array, by
  index arithmetic: out[i] = x[k] with j_a = S_a - 1 - i_a where reflect[a]
  else i_a, and k[perm[a]] = j_a."""
  perm, reflect = check_transform(perm, reflect)
  x = np.asarray(x)
  if x.ndim != RANK:
    raise ValueError('a [z, y, x] array, got shape %r' % (x.shape,))
  out_shape = tuple(x.shape[p] for p in perm)
  index = np.indices(out_shape)
  source = [None] * RANK
  for a in range(RANK):
    j = out_shape[a] - 1 - index[a] if reflect[a] else index[a]
    source[perm[a]] = j
  return x[tuple(source)]


def keeps_shape(shape, perm) -> bool:
  """Whether every axis that changes places has the size of the axis it takes
  the place of (the reference's permute_axes cannot keep a static shape
  otherwise, and the device slots have one)."""
  return all(shape[a] == shape[int(p)] for a, p in enumerate(perm))


# ---- section augmentations ---------------------------------------------------------


class SectionPlan:
  """The decisions of the section augmentations for one example: what
  ffn_evaluation_section_plan and its ffn_evaluation_section rows hold
  (include/ffn_evaluation.h).  `sections` is the number of image sections.

  margin_yx, kind (NONE / SLIP / TRANSLATION), z0, dy, dx: misalignment.
  blank_value (float32), blank_mask [z], blank_yx [z, 2]: missing section.
  blur_sigma (float32), blur_mask [z], blur_yx [z, 2]: out of focus.
  gray [z] 0 / 1, factors [z, 3] float32 (contrast, brightness, gamma).
  """

  def __init__(self, sections: int, margin_yx=(0, 0)):
    self.sections = int(sections)
    self.margin_yx = (int(margin_yx[0]), int(margin_yx[1]))
    self.kind, self.z0, self.dy, self.dx = NONE, 0, 0, 0
    self.blank_value = np.float32(0)
    self.blur_sigma = np.float32(0)
    self.blank_mask = np.zeros(self.sections, np.uint8)
    self.blank_yx = np.zeros((self.sections, 2), np.int32)
    self.blur_mask = np.zeros(self.sections, np.uint8)
    self.blur_yx = np.zeros((self.sections, 2), np.int32)
    self.gray = np.zeros(self.sections, np.uint8)
    self.factors = np.zeros((self.sections, 3), np.float32)
    # the sections chosen, for the summaries only (one whose four quadrant
    # draws all fail is chosen and unchanged); None: whatever the masks select
    self.missing_z = None
    self.outoffocus_z = None

  def is_empty(self) -> bool:
    return (self.kind == NONE and not self.blank_mask.any() and
            not self.blur_mask.any() and not self.gray.any())

  def summary(self) -> dict:
    """What the reference's functions return for their tensorboard summaries:
    the z the misalignment starts at (-1: skipped), the blanked and the blurred
    z indices, whether the grayscale perturbation was applied."""
    chosen = lambda z, mask: sorted(int(v) for v in (
        np.flatnonzero(mask) if z is None else z))
    return {'misalignment_z': self.z0 if self.kind != NONE else -1,
            'missing_z': chosen(self.missing_z, self.blank_mask),
            'outoffocus_z': chosen(self.outoffocus_z, self.blur_mask),
            'grayscale': int(self.gray.any())}

  def key(self):
    """A hashable, exactly comparable statement of the plan."""
    return (self.sections, self.margin_yx, self.kind, self.z0, self.dy,
            self.dx, float(self.blank_value), float(self.blur_sigma),
            self.blank_mask.tobytes(), self.blank_yx.tobytes(),
            self.blur_mask.tobytes(), self.blur_yx.tobytes(),
            self.gray.tobytes(), self.factors.tobytes())

  def __eq__(self, other):
    return isinstance(other, SectionPlan) and self.key() == other.key()

  def __hash__(self):
    return hash(self.key())

  def __repr__(self):
    return 'SectionPlan(%r)' % (self.summary(),)


def blur_radius(sigma) -> int:
  """scipy.ndimage.gaussian_filter's radius at truncate = 4."""
  return int(4.0 * float(sigma) + 0.5)


def padded_size(image_zyx, label_zyx, margin_yx):
  """M of include/ffn_evaluation.h: the per-axis maximum of the two loaded
  boxes."""
  return (max(image_zyx[0], label_zyx[0]),
          max(image_zyx[1], label_zyx[1]) + 2 * margin_yx[0],
          max(image_zyx[2], label_zyx[2]) + 2 * margin_yx[1])


def check_plan(plan: SectionPlan, image_zyx, label_zyx):
  """Raises ValueError on what ffn_evaluation_load_sections refuses in a
  plan."""
  if plan.sections != image_zyx[0]:
    raise ValueError('a plan for %d sections, the image patch has %d' %
                     (plan.sections, image_zyx[0]))
  if min(plan.margin_yx) < 0:
    raise ValueError('negative margin %r' % (plan.margin_yx,))
  if plan.kind not in (NONE, SLIP, TRANSLATION):
    raise ValueError('misalignment kind %r' % (plan.kind,))
  m = padded_size(image_zyx, label_zyx, plan.margin_yx)
  if not 0 <= plan.z0 < m[0]:
    raise ValueError('z0 %d outside [0, %d)' % (plan.z0, m[0]))
  if abs(plan.dy) > m[1] or abs(plan.dx) > m[2]:
    raise ValueError('misalignment offset (%d, %d) exceeds the padded size' %
                     (plan.dy, plan.dx))
  sigma = float(plan.blur_sigma)
  if not sigma >= 0 or blur_radius(min(sigma, 1e6)) > MAX_BLUR_RADIUS:
    raise ValueError('blur_sigma %r' % (sigma,))
  for mask, yx in ((plan.blank_mask, plan.blank_yx),
                   (plan.blur_mask, plan.blur_yx)):
    if (mask > 15).any():
      raise ValueError('a quadrant mask has four bits')
    if ((yx < 0) | (yx > np.array(image_zyx[1:]))).any():
      raise ValueError('a split point outside the section')
  if (plan.gray > 1).any():
    raise ValueError('gray is 0 or 1')
  on = plan.factors[plan.gray > 0]
  if not np.isfinite(on).all() or (on[:, 2] <= 0).any():
    raise ValueError('grayscale factors are finite and gamma is positive')
  if (plan.blur_mask.any() and blur_radius(sigma) > 0 and
      image_zyx[1] * image_zyx[2] > MAX_BLUR_PLANE):
    raise ValueError('a blur on a section of more than %d voxels' %
                     MAX_BLUR_PLANE)


class SectionAugmentations:
  """Samples SectionPlans as the reference's apply_section_augmentations would
  decide them.

  config: a dict under the reference's argument names (SECTION_KEYS); an
    augmentation none of whose keys is given is off, one with some of its keys
    missing raises, and so does a key of the elastic or affine augmentations,
    which are not implemented.  `margin_yx` (optional, not the reference's):
    how much larger than the final patch the box is that is read from the
    volume; default max_xy_offset on both axes, so that no voxel wrapped
    around by np.roll reaches the final patch.
  rng: a numpy.random.RandomState (or a seed for one).  The legacy generator on
    purpose: the reference draws from the global np.random, and
    np.random.seed(s) followed by its calls gives what RandomState(s) gives
    here.
  """

  def __init__(self, config: dict, rng=None):
    config = dict(config)
    for key in config:
      if key in UNSUPPORTED_SECTION_KEYS:
        raise ValueError(
            '%s: %s is not implemented (nothing to check it against: it needs '
            'skimage.transform.warp)' % (key, UNSUPPORTED_SECTION_KEYS[key]))
    known = {k for keys in SECTION_KEYS.values() for k in keys} | {'margin_yx'}
    unknown = sorted(set(config) - known)
    if unknown:
      raise ValueError('unknown section augmentation keys %r' % (unknown,))
    self.enabled = {}
    for name, keys in SECTION_KEYS.items():
      given = [k for k in keys if k in config]
      if given and len(given) != len(keys):
        raise ValueError('%s needs all of %r' % (name, keys))
      self.enabled[name] = bool(given)
    for key, value in config.items():
      if key != 'margin_yx' and not float(value) >= 0:
        raise ValueError('%s must not be negative, got %r' % (key, value))
    self.config = config
    self.max_xy_offset = int(config.get('max_xy_offset', 0))
    if self.max_xy_offset != config.get('max_xy_offset', 0):
      raise ValueError('max_xy_offset is an integer')
    margin = config.get('margin_yx', (self.max_xy_offset,) * 2)
    self.margin_yx = (int(margin[0]), int(margin[1]))
    if min(self.margin_yx) < 0:
      raise ValueError('negative margin %r' % (margin,))
    if blur_radius(config.get('max_filter_stdev', 0)) > MAX_BLUR_RADIUS:
      raise ValueError('max_filter_stdev %r gives a blur radius above %d' %
                       (config['max_filter_stdev'], MAX_BLUR_RADIUS))
    if rng is None or isinstance(rng, (int, np.integer)):
      rng = np.random.RandomState(rng)
    self.rng = rng

  def _quadrants(self, mask, yx, z, shape_yx):
    """The draws of one chosen section after `blurred` / the fill exist: the
    whole section, or _quadrant_replace's."""
    rng = self.rng
    if rng.rand() < FULL_PROB:
      mask[z], yx[z] = 8, (0, 0)
      return
    bits = rng.rand(4) < QUADRANT_PROB
    y = rng.randint(0, shape_yx[0])
    x = rng.randint(0, shape_yx[1])
    mask[z] = sum(int(b) << k for k, b in enumerate(bits))
    yx[z] = (y, x)

  def _chosen_sections(self, ratio, sections):
    """Two draws: how many sections (1 .. at most `ratio` of them, at least
    one), then which, without repetition."""
    most = max(int(ratio * sections), 1)
    count = self.rng.randint(1, most + 1)
    return self.rng.choice(sections, count, replace=False)

  def sample(self, image_zyx, label_zyx) -> SectionPlan:
    """One plan for final patches of these sizes: the reference's draws in the
    reference's order (misalignment, missing section, out of focus,
    grayscale)."""
    rng, c = self.rng, self.config
    sections, shape_yx = int(image_zyx[0]), tuple(image_zyx[1:])
    plan = SectionPlan(sections, self.margin_yx)
    if self.enabled['misalignment']:
      if not rng.rand() < c['misalignment_skip_ratio']:
        m = padded_size(image_zyx, label_zyx, self.margin_yx)
        dy, dx = rng.randint(-self.max_xy_offset, self.max_xy_offset + 1, 2)
        plan.z0 = int(rng.randint(0, m[0]))
        plan.dy, plan.dx = int(dy), int(dx)
        plan.kind = (SLIP if rng.rand() < c['slip_vs_translate_ratio']
                     else TRANSLATION)
    if self.enabled['missing_section']:
      if not rng.rand() < c['missing_section_skip_ratio']:
        chosen = self._chosen_sections(
            c['max_missing_section_indices_ratio'], sections)
        plan.blank_value = np.float32(rng.rand() * MAX_FILL_VAL)
        plan.missing_z = [int(z) for z in chosen]
        for z in chosen:
          self._quadrants(plan.blank_mask, plan.blank_yx, z, shape_yx)
    if self.enabled['out_of_focus']:
      if not rng.rand() < c['outoffocus_skip_ratio']:
        chosen = self._chosen_sections(c['max_outoffocus_indices_ratio'],
                                       sections)
        plan.blur_sigma = np.float32(rng.rand() * c['max_filter_stdev'])
        plan.outoffocus_z = [int(z) for z in chosen]
        for z in chosen:
          self._quadrants(plan.blur_mask, plan.blur_yx, z, shape_yx)
    if self.enabled['grayscale']:
      if not rng.rand() < c['grayscale_skip_ratio']:
        def factors():
          # three draws, each centred on 0: a contrast around 1, a brightness
          # around 0, a gamma between 1 / 2 and 2 (float64 until stored)
          u = [rng.rand() for _ in range(3)]
          return (1 + (u[0] - 0.5) * c['max_contrast_factor'],
                  (u[1] - 0.5) * c['max_brightness_factor'],
                  2.0 ** (u[2] * 2 - 1))
        plan.gray[:] = 1
        if rng.rand() < FULL_PROB:
          plan.factors[:] = factors()
        else:
          for z in range(sections):
            plan.factors[z] = factors()
    return plan

  @staticmethod
  def apply(image, labels, plan: SectionPlan, image_zyx=None, label_zyx=None):
    return apply_sections(image, labels, plan, image_zyx, label_zyx)


def gaussian_weights(sigma):
  """w_0 .. w_r of scipy's _gaussian_kernel1d (float64)."""
  sigma = float(sigma)
  radius = blur_radius(sigma)
  if radius == 0:
    return np.ones(1)
  x = np.arange(-radius, radius + 1)
  phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
  return (phi / phi.sum())[radius:]


def _reflect(index, n):
  index = np.mod(index, 2 * n)
  return np.where(index < n, index, 2 * n - 1 - index)


def _blur_axis(plane, weights, axis):
  """One pass of the blur of a float32 [y, x] plane: float64 sums in
  correlate1d's order, rounded to float32."""
  n = plane.shape[axis]
  wide = plane.astype(np.float64)
  at = lambda idx: np.take(wide, _reflect(idx, n), axis=axis)
  base = np.arange(n)
  acc = wide * weights[0]
  for k in range(len(weights) - 1, 0, -1):
    acc = acc + (at(base - k) + at(base + k)) * weights[k]
  return acc.astype(np.float32)


def quadrant_selection(mask, yx, shape_yx):
  """bool [y, x]: the voxels the four bits select around the split point."""
  y, x = np.indices(shape_yx)
  quadrant = (y >= yx[0]).astype(np.int64) + 2 * (x >= yx[1])
  return ((int(mask) >> quadrant) & 1).astype(bool)


def misaligned_indices(plan: SectionPlan, final_zyx, m):
  """(z, y, x) index arrays into the loaded box of an array whose final size is
  `final_zyx`, broadcastable to it."""
  Z, Hf, Wf = final_zyx
  H, W = Hf + 2 * plan.margin_yx[0], Wf + 2 * plan.margin_yx[1]
  z = np.arange(Z)
  zp = z + (m[0] - Z) // 2
  moved = (zp == plan.z0 if plan.kind == SLIP else
           zp >= plan.z0 if plan.kind == TRANSLATION else
           np.zeros(Z, bool))[:, None]
  py = (np.arange(Hf) + (m[1] - Hf) // 2)[None, :]
  px = (np.arange(Wf) + (m[2] - Wf) // 2)[None, :]
  py = np.where(moved, np.mod(py - plan.dy, m[1]), py)
  px = np.where(moved, np.mod(px + plan.dx, m[2]), px)
  jy = np.clip(py - (m[1] - H) // 2, 0, H - 1)
  jx = np.clip(px - (m[2] - W) // 2, 0, W - 1)
  return z[:, None, None], jy[:, :, None], jx[:, None, :]


def apply_sections(image, labels, plan: SectionPlan, image_zyx=None,
                   label_zyx=None):
  """The numpy statement of ffn_evaluation_load_sections' steps 1 - 4.

  image, labels: the boxes read from the volume, [z, y, x], each its final
  size (`image_zyx` / `label_zyx`; default: the box less the margins) enlarged
  by the plan's margins.  -> (float32 image of the final size, before load's
  normalisation; the labels of the final size at the mapped indices, in their
  own dtype)."""
  image, labels = np.asarray(image), np.asarray(labels)
  my, mx = plan.margin_yx
  less = lambda shape: (shape[0], shape[1] - 2 * my, shape[2] - 2 * mx)
  image_zyx = tuple(image_zyx or less(image.shape))
  label_zyx = tuple(label_zyx or less(labels.shape))
  if (less(image.shape) != image_zyx or less(labels.shape) != label_zyx):
    raise ValueError('boxes %r / %r are not the final sizes %r / %r plus the '
                     'margins %r' % (image.shape, labels.shape, image_zyx,
                                     label_zyx, plan.margin_yx))
  check_plan(plan, image_zyx, label_zyx)
  m = padded_size(image_zyx, label_zyx, plan.margin_yx)
  out = image[misaligned_indices(plan, image_zyx, m)].astype(np.float32)
  out_labels = labels[misaligned_indices(plan, label_zyx, m)]
  shape_yx = image_zyx[1:]
  weights = gaussian_weights(plan.blur_sigma)
  for z in range(plan.sections):
    if plan.blank_mask[z]:
      out[z][quadrant_selection(plan.blank_mask[z], plan.blank_yx[z],
                                shape_yx)] = plan.blank_value
    if plan.blur_mask[z] and len(weights) > 1:
      blurred = _blur_axis(_blur_axis(out[z], weights, 0), weights, 1)
      where = quadrant_selection(plan.blur_mask[z], plan.blur_yx[z], shape_yx)
      out[z][where] = blurred[where]
    if plan.gray[z]:
      contrast, brightness, gamma = plan.factors[z]  # float32 scalars
      normalized = out[z] / np.float32(MAX_VAL)
      adjusted = normalized * contrast + brightness
      clipped = np.minimum(np.maximum(adjusted, np.float32(0)), np.float32(1))
      out[z] = np.power(clipped, gamma) * np.float32(MAX_VAL)
  return out, np.ascontiguousarray(out_labels)
