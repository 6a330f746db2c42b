"""The section augmentations on the GPU (include/ffn_evaluation.h
load_sections, EvaluationOps.load_sections, BatchExampleIter(sections=...),
train.py --section_augmentation) against the numpy restatement
(tests/sections_ref.py) and the reference's recorded outputs
(tests/golden/ref_sections.npz).

The yardstick is DESIGN.md 10.8's: labels and seed bit for bit; the image bit
for bit against the f32 statement on every voxel that neither blur nor gray
writes, and within 4 E_ref of the f64 statement everywhere, E_ref = max |f32
statement - f64 statement| of the case, at least one f32 ulp of its largest
value.  Measured distances: DESIGN.md 10.8."""
import json
import os

import numpy as np
import pytest

from tests import sections_ref
from tests import test_sections as cpu
from tests import test_training_loop as loop
from tests import training_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = ((0, 1, 2), (0, 0, 0))


@pytest.fixture(scope='module')
def ev():
  from ffn_amd.training import evaluation
  return evaluation


@pytest.fixture(scope='module')
def aug():
  from ffn_amd.training import augmentation
  return augmentation


@pytest.fixture(scope='module')
def ops(ev):
  return ev.default_ops(0)


def make_geometry(ev, image_zyx, label_zyx, slots):
  """Image and label patches of the given sizes (label <= image per axis);
  everything else is the label patch."""
  l = tuple(label_zyx)
  return ev.Geometry(input_seed=l, input_image=l, pred_mask=l, deltas=(0, 0, 0),
                     canvas=l, image_patch=tuple(image_zyx), label_patch=l,
                     eval=l, slots=slots)


def geom_dict(g):
  return {k: tuple(getattr(g, k)) for k in (
      'input_seed', 'input_image', 'pred_mask', 'deltas', 'canvas',
      'image_patch', 'label_patch', 'eval')}


def make_volume(shape, seed, image_dtype=np.uint8, label_dtype=np.uint64):
  """A random image; labels in 2 x 2 x 2 blocks of four ids which, as uint64,
  differ only above bit 32."""
  rng = np.random.RandomState(seed)
  if image_dtype == np.uint8:
    image = rng.randint(0, 256, shape).astype(np.uint8)
  else:
    image = rng.uniform(0, 255, shape).astype(np.float32)
  ids = rng.randint(0, 4, [(s + 1) // 2 for s in shape])
  for a in range(3):
    ids = np.repeat(ids, 2, a)
  ids = ids[:shape[0], :shape[1], :shape[2]].astype(np.uint64)
  if label_dtype == np.uint64:
    ids = np.where(ids > 0, np.uint64(5) + (ids << np.uint64(32)), 0)
  return image, ids.astype(label_dtype)


def read_slot(ops, s):
  return [ops.read_image(s), ops.read_labels(s), ops.read_seed(s)]


def same(a, b):
  return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_slot(ops, slot, volume, centre, offset, scale, gd, transform, plan,
               worst, note=None):
  """The slot against both statements; `worst` collects (distance / bound,
  distance, bound) per kind of operation.

  E_ref is taken where the yardstick defines it, on what the augmentations
  return (0 ... 255 values, offset 0 and scale 1), and divided by the scale:
  the slot holds (v - offset) / scale, and an ulp of that is finer than an ulp
  of v, so a floor taken after the normalisation would ask for more than the
  f32 operations before it can give (numpy's float32 power alone is one ulp
  off the correctly rounded one on a fifth of its arguments).
  The test against the fixture, at scale 1, applies the yardstick as it
  stands."""
  args = (volume[0], volume[1], centre, offset, scale, gd) + tuple(transform)
  raw = (volume[0], volume[1], centre, 0.0, 1.0, gd) + tuple(transform)
  e = sections_ref.e_ref(
      sections_ref.load_sections(*raw, plan)[0],
      sections_ref.load_sections(*raw, plan, dtype=np.float64)[0]) / scale
  ref32 = sections_ref.load_sections(*args, plan)
  ref64 = sections_ref.load_sections(*args, plan, dtype=np.float64)
  got = read_slot(ops, slot)
  assert np.array_equal(got[1], ref32[1]), note
  assert np.array_equal(got[2], ref32[2]), note
  exact = sections_ref.untouched(plan, gd, *transform)
  ok, distance, bound = sections_ref.within(got[0], ref32[0], ref64[0], exact,
                                            e)
  kind = ('gray' if plan.gray.any() else
          'blur' if not exact.all() else 'exact')
  worst.setdefault(kind, []).append((distance / bound, distance, bound))
  assert ok, (note, distance, bound, int(exact.sum()), exact.size)
  if exact.all():
    assert np.array_equal(got[0], ref32[0]), note


def report(worst):
  for kind, rows in sorted(worst.items()):
    ratio, distance, bound = max(rows)
    print('%s: %d slots, largest distance / bound %.3g (distance %.3g, bound '
          '%.3g, E_ref %.3g)' % (kind, len(rows), ratio, distance, bound,
                                 bound / 4))


def load_all(ops, volumes, centres, offsets, scales, transforms, plans,
             slots=None):
  n = len(plans)
  slots = list(range(n)) if slots is None else slots
  ops.load_sections(slots, volumes, centres, offsets, scales,
                    [p for p, _ in transforms], [r for _, r in transforms],
                    plans, 0.05)
  return slots


# ---- the reference's recorded outputs ---------------------------------------------


def fixture_groups():
  groups = {}
  for name in cpu.CASES:
    c = cpu.FIXTURE[name]
    groups.setdefault((c['image_zyx'], c['label_zyx']), []).append(name)
  return sorted(groups.items())


@pytest.mark.parametrize('sizes,names', fixture_groups(),
                         ids=['x'.join(str(v) for v in s[0])
                              for s, _ in fixture_groups()])
def test_device_reproduces_the_references_outputs(ev, ops, sizes, names):
  """Offset 0 and scale 1 are exact, so the slot holds what the reference's
  functions returned; the plan is the sampler's under the case's seed."""
  image_zyx, label_zyx = sizes
  g = make_geometry(ev, image_zyx, label_zyx, len(names))
  ops.configure(g)
  ops.reset()
  cases = [cpu.FIXTURE[n] for n in names]
  plans = [cpu.sampled_plan(c) for c in cases]
  high = lambda ids: np.where(ids > 0, ids << np.uint64(33), 0).astype(
      np.uint64)
  vols = [ops.add_volume(c['image'], high(c['labels'])) for c in cases]
  n = len(cases)
  load_all(ops, vols, [cpu.centre_of(c) for c in cases], [0.0] * n, [1.0] * n,
           [IDENTITY] * n, plans)
  worst = {}
  for s, (name, c, plan) in enumerate(zip(names, cases, plans)):
    got = read_slot(ops, s)
    centre = c['labels'][tuple((a - 1) // 2 - (f - 1) // 2 + f // 2
                               for a, f in zip(c['labels'].shape, label_zyx))]
    soft = np.where((c['ref_labels'] > 0) & (c['ref_labels'] == centre),
                    np.float32(0.95), np.float32(0.05))
    assert np.array_equal(got[1], soft), name
    exact = cpu.exact_voxels(plan, image_zyx[1:])
    ok, distance, bound = sections_ref.within(got[0], c['ref32'], c['ref64'],
                                              exact)
    worst.setdefault(name.split('_')[0], []).append(
        (distance / bound, distance, bound))
    assert ok, (name, distance, bound)
    if exact.all():
      assert np.array_equal(got[0], c['ref32']), name
  report(worst)


# ---- misalignment ------------------------------------------------------------------


@pytest.mark.parametrize('image_zyx,label_zyx', [((5, 9, 11), (3, 5, 7)),
                                                 ((6, 6, 6), (6, 6, 6))])
def test_misalignment(ev, aug, ops, image_zyx, label_zyx):
  """Slip and translation at z0 = 0, middle and last of the padded z size, the
  offsets at +- their maximum (margin 0: the wrap shows; beyond the margin;
  the padded size itself), three margins; the label patch smaller in z, so
  that its sections are tested one higher than the image's."""
  g = make_geometry(ev, image_zyx, label_zyx, 32)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  shape = (image_zyx[0] + 1, image_zyx[1] + 7, image_zyx[2] + 8)
  volume = make_volume(shape, 3)
  vol = ops.add_volume(*volume)
  centre = tuple((s - 1) // 2 for s in shape)[::-1]
  m_z = max(image_zyx[0], label_zyx[0])
  plans = []
  for margin in ((0, 0), (2, 2), (1, 3)):
    m = aug.padded_size(image_zyx, label_zyx, margin)
    for kind in (aug.SLIP, aug.TRANSLATION):
      for z0 in (0, m_z // 2, m_z - 1):
        for dy, dx in ((2, -2), (-3, 3), (m[1], -m[2])):
          plan = aug.SectionPlan(image_zyx[0], margin)
          plan.kind, plan.z0, plan.dy, plan.dx = kind, z0, dy, dx
          plans.append(plan)
  assert len(plans) == 54
  worst, differing = {}, set()
  for start in (0, 32):
    chunk = plans[start:start + 32]
    n = len(chunk)
    slots = load_all(ops, [vol] * n, [centre] * n, [100.0] * n, [30.0] * n,
                     [IDENTITY] * n, chunk)
    for s, plan in zip(slots, chunk):
      check_slot(ops, s, volume, centre, 100.0, 30.0, gd, IDENTITY, plan,
                 worst, plan.key())
      differing.add(ops.read_image(s).tobytes())
  assert set(worst) == {'exact'} and len(differing) > 20
  report(worst)


# ---- missing section and out of focus: the quadrants ---------------------------------


def test_all_16_masks_of_blank_and_blur(ev, aug, ops):
  """Every mask, the split point at 0, inside and at the size."""
  image_zyx = label_zyx = (3, 9, 11)
  g = make_geometry(ev, image_zyx, label_zyx, 32)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  volume = make_volume((3, 9, 11), 4)
  vol = ops.add_volume(*volume)
  centre = (5, 4, 1)
  plans = []
  for split in ((0, 0), (4, 5), (9, 11), (0, 11), (9, 3)):
    for mask in range(16):
      plan = aug.SectionPlan(3)
      plan.blank_value = np.float32(17.25)
      plan.blur_sigma = np.float32(1.0)
      plan.blank_mask[0], plan.blank_yx[0] = mask, split
      plan.blur_mask[1], plan.blur_yx[1] = mask, split
      # both on one section: the blur sees the blanked section
      plan.blank_mask[2], plan.blank_yx[2] = 15 - mask, split
      plan.blur_mask[2], plan.blur_yx[2] = mask, split
      aug.check_plan(plan, image_zyx, label_zyx)
      plans.append(plan)
  worst = {}
  for start in range(0, len(plans), 32):
    chunk = plans[start:start + 32]
    n = len(chunk)
    slots = load_all(ops, [vol] * n, [centre] * n, [0.0] * n, [1.0] * n,
                     [IDENTITY] * n, chunk)
    for s, plan in zip(slots, chunk):
      check_slot(ops, s, volume, centre, 0.0, 1.0, gd, IDENTITY, plan, worst,
                 (int(plan.blank_mask[0]), tuple(plan.blank_yx[0])))
  report(worst)


# ---- the blur ----------------------------------------------------------------------


def blur_plans(aug, sections, sigmas):
  plans = []
  for sigma in sigmas:
    plan = aug.SectionPlan(sections)
    plan.blur_sigma = np.float32(sigma)
    plan.blur_mask[:], plan.blur_yx[:] = 8, (0, 0)
    plans.append(plan)
  return plans


@pytest.mark.parametrize('image_zyx,sigmas,radii', [
    ((2, 9, 11), (0.1, 0.25, 3.0, 7.75), [0, 1, 12, 31]),
    ((2, 35, 67), (2.0, 7.75), [8, 31]),
    ((1, 128, 128), (2.0,), [8])])
def test_blur(ev, aug, ops, image_zyx, sigmas, radii):
  """Radii 0 (the identity), 1, 12 (more than the plane: several reflections)
  and the largest; rows across 32 and 64 lanes; the largest plane, which
  takes 128 KiB of LDS."""
  g = make_geometry(ev, image_zyx, image_zyx, len(sigmas))
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  assert [aug.blur_radius(np.float32(s)) for s in sigmas] == radii
  volume = make_volume(image_zyx, 5, np.float32)
  vol = ops.add_volume(*volume)
  centre = tuple((s - 1) // 2 for s in image_zyx)[::-1]
  plans = blur_plans(aug, image_zyx[0], sigmas)
  n = len(plans)
  load_all(ops, [vol] * n, [centre] * n, [128.0] * n, [33.0] * n,
           [IDENTITY] * n, plans)
  worst = {}
  for s, plan in enumerate(plans):
    check_slot(ops, s, volume, centre, 128.0, 33.0, gd, IDENTITY, plan, worst,
               float(plan.blur_sigma))
  report(worst)
  if radii[0] == 0:
    plain = sections_ref.load_sections(*volume, centre, 128.0, 33.0, gd,
                                       *IDENTITY, aug.SectionPlan(2))
    assert np.array_equal(ops.read_image(0), plain[0])
  ms, nbytes = ops.last_timing_sections()['load_sections']
  kernel_ms, kernel_bytes = ops.last_timing_sections()['sections_kernel']
  voxels = int(np.prod(image_zyx))
  assert 0 < kernel_ms <= ms
  assert nbytes == n * voxels * (4 + 8 + 3 * 4)
  assert kernel_bytes == n * voxels * (4 + 8 + 2 * 4)


# ---- grayscale ---------------------------------------------------------------------


def test_grayscale(ev, aug, ops):
  """One set of factors for the patch, one per section, and a brightness that
  drives part of a section below 0 and part above 1."""
  image_zyx = (4, 9, 11)
  g = make_geometry(ev, image_zyx, image_zyx, 8)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  plans = []
  for factors in ([(1.2, 0.1, 0.6)] * 4,
                  [(0.8, -0.1, 1.7), (1.3, 0.2, 0.5), (1.0, 0.0, 1.0),
                   (0.7, 0.05, 2.0)],
                  [(1.5, -0.45, 0.8), (1.5, 0.45, 1.3), (2.0, -0.5, 0.5),
                   (1.0, 0.3, 2.0)]):
    plan = aug.SectionPlan(4)
    plan.gray[:] = 1
    plan.factors[:] = factors
    plans.append(plan)
  only_two = aug.SectionPlan(4)
  only_two.gray[2], only_two.factors[2] = 1, (1.1, 0.1, 0.9)
  plans.append(only_two)
  worst = {}
  for dtype in (np.uint8, np.float32):
    volume = make_volume((4, 9, 11), 6, dtype)
    vol = ops.add_volume(*volume)
    n = len(plans)
    load_all(ops, [vol] * n, [(5, 4, 1)] * n, [128.0] * n, [33.0] * n,
             [IDENTITY] * n, plans)
    for s, plan in enumerate(plans):
      check_slot(ops, s, volume, (5, 4, 1), 128.0, 33.0, gd, IDENTITY, plan,
                 worst)
    raw = sections_ref.apply(volume[0], volume[1], plans[2], image_zyx,
                             image_zyx)[0]
    assert (raw == 0).any() and (raw == 255).any()
  report(worst)


# ---- data types, batching, the transform ---------------------------------------------


@pytest.mark.parametrize('image_dtype,label_dtype', [
    (np.uint8, np.uint64), (np.float32, np.uint32)])
def test_32_slots_of_mixed_plans_and_transforms(ev, aug, ops, image_dtype,
                                                label_dtype):
  """9^3 patches: every transform is legal.  Sampled plans (all four
  operations) with 32 of the 48 transforms, x moving in most of them."""
  size = 9
  g = make_geometry(ev, (size,) * 3, (size,) * 3, 32)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  shape = (size + 2, size + 6, size + 7)
  volume = make_volume(shape, 7, image_dtype, label_dtype)
  vol = ops.add_volume(*volume)
  sampler = aug.SectionAugmentations(dict(cpu.FULL, max_filter_stdev=3.0), 9)
  rng = np.random.RandomState(9)
  transforms = [training_ref.all_transforms()[k]
                for k in rng.permutation(48)[:32]]
  assert sum(p[2] != 2 for p, _ in transforms) > 10
  plans = [sampler.sample(g.image_patch, g.label_patch) for _ in range(32)]
  centres = [(4 + 2 + int(rng.randint(0, 4)), 4 + 2 + int(rng.randint(0, 3)),
              4 + int(rng.randint(0, 3))) for _ in range(32)]
  offsets = [100.0 + k for k in range(32)]
  scales = [33.0 - 0.5 * k for k in range(32)]
  slots = [int(s) for s in rng.permutation(32)]
  load_all(ops, [vol] * 32, centres, offsets, scales, transforms, plans, slots)
  worst = {}
  for k, s in enumerate(slots):
    check_slot(ops, s, volume, centres[k], offsets[k], scales[k], gd,
               transforms[k], plans[k], worst, (k, transforms[k]))
  report(worst)


@pytest.mark.parametrize('n', [1, 5])
def test_load_sections_leaves_the_other_slots_alone(ev, aug, ops, n):
  size = 9
  g = make_geometry(ev, (size,) * 3, (size,) * 3, 2 * n + 1)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  shape = (size + 4,) * 3
  volume = make_volume(shape, 8)
  vol = ops.add_volume(*volume)
  vol_nan = ops.add_volume(np.full(shape, np.nan, np.float32), volume[1])
  centre = (size // 2 + 2,) * 3
  every = list(range(g.slots))
  ops.load(every, [vol_nan] * g.slots, [centre] * g.slots, [0.0] * g.slots,
           [1.0] * g.slots, 0.05)
  for s in every:
    ops.write_seed(s, np.full(g.canvas, np.nan, np.float32))
  guards = {s: read_slot(ops, s) for s in range(0, g.slots, 2)}
  assert all(np.isnan(a[0]).all() and np.isnan(a[2]).all()
             for a in guards.values())
  written = list(range(1, g.slots, 2))
  sampler = aug.SectionAugmentations(cpu.FULL, n)
  plans = [sampler.sample(g.image_patch, g.label_patch) for _ in range(n)]
  transforms = [((2, 1, 0), (1, 0, 1)), ((0, 1, 2), (0, 0, 1)),
                ((1, 2, 0), (0, 1, 0)), ((0, 2, 1), (1, 1, 1)),
                ((1, 0, 2), (0, 0, 0))][:n]
  load_all(ops, [vol] * n, [centre] * n, [128.0] * n, [33.0] * n, transforms,
           plans, written)
  worst = {}
  for s, t, plan in zip(written, transforms, plans):
    check_slot(ops, s, volume, centre, 128.0, 33.0, gd, t, plan, worst, t)
  for s, before in guards.items():
    assert same(read_slot(ops, s), before), s


# ---- equalities --------------------------------------------------------------------


def test_the_empty_plan_is_load_augmented_for_all_48_transforms(ev, aug, ops):
  size = 9
  g = make_geometry(ev, (size,) * 3, (size,) * 3, 32)
  ops.configure(g)
  ops.reset()
  shape = (size + 3, size + 2, size + 5)
  volume = make_volume(shape, 10)
  vol = ops.add_volume(*volume)
  transforms = training_ref.all_transforms()
  rng = np.random.RandomState(10)
  for start, n in ((0, 32), (32, 16)):
    chunk = transforms[start:start + n]
    centres = [(4 + int(rng.randint(0, 6)), 4 + int(rng.randint(0, 3)),
                4 + int(rng.randint(0, 4))) for _ in range(n)]
    offsets = [100.0 + k for k in range(n)]
    scales = [33.0 - 0.5 * k for k in range(n)]
    perms, reflects = [p for p, _ in chunk], [r for _, r in chunk]
    ops.load_augmented(list(range(n)), [vol] * n, centres, offsets, scales,
                       perms, reflects, 0.05)
    plain = [read_slot(ops, s) for s in range(n)]
    for s in range(n):
      ops.write_seed(s, np.full(g.canvas, np.nan, np.float32))
    # zero margins, and an operation-free plan with every field set
    idle = aug.SectionPlan(size)
    idle.blank_value, idle.blur_sigma = np.float32(9.0), np.float32(2.0)
    idle.blank_yx[:], idle.blur_yx[:] = (3, 4), (9, 9)
    idle.factors[:] = (1.5, 0.5, 2.0)
    plans = [aug.SectionPlan(size) if k % 2 else idle for k in range(n)]
    load_all(ops, [vol] * n, centres, offsets, scales, chunk, plans)
    for s in range(n):
      assert same(read_slot(ops, s), plain[s]), chunk[s]


# ---- errors ------------------------------------------------------------------------


def test_every_argument_error_leaves_all_slots_unchanged(ev, aug, ops):
  image_zyx, label_zyx = (5, 9, 9), (3, 5, 5)
  g = make_geometry(ev, image_zyx, label_zyx, 4)
  ops.configure(g)
  ops.reset()
  shape = (7, 13, 13)
  volume = make_volume(shape, 11)
  vol = ops.add_volume(*volume)
  centres = [(6, 6, 3), (6, 6, 2), (6, 6, 4), (6, 6, 3)]
  sampler = aug.SectionAugmentations(cpu.FULL, 2)
  plans = [sampler.sample(image_zyx, label_zyx) for _ in range(4)]
  args = ([vol] * 4, centres, [128.0] * 4, [33.0] * 4)
  load_all(ops, *args, [((0, 2, 1), (1, 0, 1))] * 4, plans)
  before = [read_slot(ops, s) for s in range(4)]

  def changed(**change):
    plan = aug.SectionPlan(5, (2, 2))
    for key, value in change.items():
      if isinstance(value, tuple) and key != 'margin_yx':
        getattr(plan, key)[value[0]] = value[1]
      else:
        setattr(plan, key, value)
    return plan

  gray = dict(gray=(1, 1))
  bad_plans = [
      ('margin', changed(margin_yx=(-1, 2))),
      ('margin', changed(margin_yx=(2, -2))),
      ('kind', changed(kind=3)),
      ('kind', changed(kind=-1)),
      ('z0', changed(kind=1, z0=5)),
      ('z0', changed(kind=2, z0=-1)),
      ('exceeds', changed(kind=1, dy=14)),    # M_y = 9 + 4
      ('exceeds', changed(kind=2, dx=-14)),
      ('split point', changed(blank_yx=(0, (10, 0)))),
      ('split point', changed(blur_yx=(4, (0, -1)))),
      ('masks', changed(blank_mask=(2, 16))),
      ('masks', changed(blur_mask=(2, 255))),
      ('masks', changed(gray=(0, 2))),
      ('blur_sigma', changed(blur_sigma=np.float32(-1.0))),
      ('blur_sigma', changed(blur_sigma=np.float32(np.nan))),
      ('radius', changed(blur_sigma=np.float32(7.9))),
      ('blur_sigma', changed(blur_sigma=np.float32(np.inf))),
      ('factors', changed(factors=(1, (1.0, 0.0, 0.0)), **gray)),
      ('factors', changed(factors=(1, (1.0, 0.0, -1.0)), **gray)),
      ('factors', changed(factors=(1, (np.inf, 0.0, 1.0)), **gray)),
      ('factors', changed(factors=(1, (1.0, np.nan, 1.0)), **gray)),
      ('leave volume', changed(margin_yx=(3, 2))),  # y: 6 - 4 - 3 < 0
      ('leave volume', changed(margin_yx=(0, 3))),
  ]
  good = changed()
  for message, plan in bad_plans:
    with pytest.raises(Exception, match=message):
      ops.load_sections([0, 1], [vol] * 2, centres[:2], [0.0] * 2, [1.0] * 2,
                        [(0, 1, 2)] * 2, [(0, 0, 0)] * 2, [good, plan], 0.05)
    assert all(same(read_slot(ops, s), before[s]) for s in range(4)), message
  # what load_augmented refuses
  call = dict(slots=[0, 1], volumes=[vol] * 2, centres=centres[:2],
              perms=[(0, 1, 2), (0, 2, 1)], reflects=[(0, 0, 0), (0, 1, 0)])
  for message, change in [
      ('not a permutation', dict(perms=[(0, 1, 2), (0, 0, 1)])),
      ('differ in patch size', dict(perms=[(0, 1, 2), (1, 0, 2)])),
      ('not 0 or 1', dict(reflects=[(0, 0, 0), (0, 2, 0)])),
      ('leave volume', dict(centres=[(6, 6, 3), (6, 6, 5)])),
      ('no volume', dict(volumes=[vol, vol + 1])),
      ('twice', dict(slots=[1, 1])),
      ('outside', dict(slots=[0, 4]))]:
    c = dict(call, **change)
    with pytest.raises(Exception, match=message):
      ops.load_sections(c['slots'], c['volumes'], c['centres'], [0.0] * 2,
                        [1.0] * 2, c['perms'], c['reflects'], [good, good],
                        0.05)
    assert all(same(read_slot(ops, s), before[s]) for s in range(4)), message
  with pytest.raises(ValueError, match='sections'):
    ops.load_sections([0], [vol], centres[:1], [0.0], [1.0], [(0, 1, 2)],
                      [(0, 0, 0)], [aug.SectionPlan(4)], 0.05)
  with pytest.raises(ValueError, match='per slot'):
    ops.load_sections([0, 1], [vol] * 2, centres[:2], [0.0] * 2, [1.0] * 2,
                      [(0, 1, 2)] * 2, [(0, 0, 0)] * 2, [good], 0.05)
  assert all(same(read_slot(ops, s), before[s]) for s in range(4))
  # the same margins fit one voxel further in
  ops.load_sections([0], [vol], [(6, 6, 3)], [0.0], [1.0], [(0, 1, 2)],
                    [(0, 0, 0)], [changed(margin_yx=(2, 2), kind=1, z0=4,
                                          dy=13, dx=-13)], 0.05)
  # a blur on a plane above 128 x 128 is refused, the same plane unblurred not
  wide = (1, 128, 129)
  ops.configure(make_geometry(ev, wide, wide, 1))
  ops.reset()
  big = make_volume(wide, 12)
  vol = ops.add_volume(*big)
  plan = blur_plans(aug, 1, [1.0])[0]
  with pytest.raises(Exception, match='16384'):
    ops.load_sections([0], [vol], [(64, 63, 0)], [0.0], [1.0], [(0, 1, 2)],
                      [(0, 0, 0)], [plan], 0.05)
  blank = aug.SectionPlan(1)
  blank.blank_mask[0], blank.blank_yx[0] = 4, (100, 100)
  blank.blank_value = np.float32(3.0)
  ops.load_sections([0], [vol], [(64, 63, 0)], [0.0], [1.0], [(0, 1, 2)],
                    [(0, 0, 0)], [blank], 0.05)
  want = big[0].astype(np.float32)
  want[0, :100, 100:] = 3.0
  assert np.array_equal(ops.read_image(0), want)


# ---- the loop ----------------------------------------------------------------------


def seed_forward(seed, image):
  """A network that looks at its seed only, so that the walk on the device
  and the restated one see the same logits whatever the last bits of the
  blurred image: grows the object within its section, so the moves along z
  are refused and an example lasts nine steps."""
  from scipy import ndimage
  del image
  seed = np.asarray(seed, np.float32)
  grown = ndimage.maximum_filter(seed, size=(1, 1, 5, 5), mode='constant',
                                 cval=-10.0)
  return np.maximum(seed, grown - np.float32(0.3)).astype(np.float32)


def test_batch_example_iter_with_sections_against_the_restated_loop(
    ev, aug, ops):
  """Depth-3 geometry (FoV 9^3, deltas 2), batch 2, 12 steps: identical
  offsets, records, transforms and plans; labels and seeds bit for bit and the
  slot images within the yardstick when an example ends or the run does."""
  import torch
  from ffn_amd.training import examples
  F = loop.FIXTURE
  info = loop.Info(F['fov_xyz'], F['deltas_xyz'])
  transform = aug.PermuteAndReflect((0, 1, 2), (0, 1, 2), 11)
  sections = aug.SectionAugmentations(cpu.FULL, 21)
  geometry = ev.Geometry.from_info(info, 'fixed', F['fov_moves'], 2)
  batches = examples.BatchExampleIter(
      info, ops, loop.fixture_volumes(), F['coordinates'], fov_policy='fixed',
      fov_moves=F['fov_moves'], batch_size=2, transform=transform,
      sections=sections, keep_history=True,
      io=examples.torch_io(geometry, 2, torch.device('cuda:0')))
  slots_seen = {}
  steps = 12
  for _ in range(steps):
    seed, image, labels, _ = batches.next()
    for s in range(2):  # what the slot holds for the example it is on
      entry = batches._current[s]
      if id(entry) not in slots_seen:
        slots_seen[id(entry)] = (ops.read_image(s), ops.read_labels(s))
    logits = torch.from_numpy(seed_forward(seed.cpu().numpy(), None)).to(
        'cuda:0')
    torch.cuda.synchronize()
    batches.update_seeds(logits)
  replay = aug.SectionAugmentations(cpu.FULL, 21)
  plans = [replay.sample(geometry.image_patch, geometry.label_patch)
           for _ in batches.history]
  assert [e['plan'] for e in batches.history] == plans
  transforms = [(e['perm'], e['reflect']) for e in batches.history]
  gd = loop.fixture_geometry()
  want = sections_ref.run_loop(seed_forward, loop.fixture_volumes(),
                               batches.coordinates, transforms, plans, gd, 2,
                               steps)
  assert loop.sequences(batches.history) == loop.sequences(want)
  assert len(want) > 2 and batches.skipped > 0
  worst = {}
  image_volume, label_volume, offset, scale = loop.fixture_volumes()['v']
  for e, w in zip(batches.history, want):
    got_image, got_labels = slots_seen[id(e)]
    assert np.array_equal(got_labels, w['labels'])
    centre = batches.coordinates[e['coordinate']][0]
    t = (e['perm'], e['reflect'])
    ref64 = sections_ref.load_sections(image_volume, label_volume, centre,
                                       offset, scale, gd, *t, e['plan'],
                                       dtype=np.float64)[0]
    raw = [sections_ref.load_sections(image_volume, label_volume, centre, 0.0,
                                      1.0, gd, *t, e['plan'], dtype=d)[0]
           for d in (np.float32, np.float64)]
    ok, distance, bound = sections_ref.within(
        got_image, w['image'], ref64,
        sections_ref.untouched(e['plan'], gd, *t),
        sections_ref.e_ref(*raw) / scale)  # as check_slot takes it
    worst.setdefault('loop', []).append((distance / bound, distance, bound))
    assert ok, (distance, bound)
  for s in range(2):  # the examples still open: their seeds as restated
    entry = batches._current[s]
    w = want[batches.history.index(entry)]
    assert np.array_equal(ops.read_seed(s), w['seed'])
  report(worst)


def test_train_script_with_the_flag_stays_finite_and_resumes(ev, ops,
                                                             tmp_path):
  from ffn_amd import synthetic
  from tests import test_gpu_training_loop as base
  shape = (64, 64, 64)
  image = synthetic.cells_volume(shape, seed=12, cells_per_96cube=40.0)
  labels = synthetic.cells_labels(shape, seed=12, cells_per_96cube=40.0)
  np.save(tmp_path / 'image.npy', image)
  np.save(tmp_path / 'labels.npy', labels)
  partitions = np.where(labels > 0, 1, 0).astype(np.uint8)
  partitions[:30] = partitions[34:] = 255  # a thin slab: a small file
  coords = str(tmp_path / 'coords')
  base.script('build_coordinates').build_coordinates(
      [('a', partitions)], (24, 24, 24), coords, seed=5)
  train = base.script('train')
  train_dir = tmp_path / 'run'
  argv = ['--train_coords', coords,
          '--data_volumes', 'a:%s' % (tmp_path / 'image.npy'),
          '--label_volumes', 'a:%s' % (tmp_path / 'labels.npy'),
          '--model_name', 'convstack_3d.ConvStack3DFFNModel', '--model_args',
          '{"depth": 2, "fov_size": [9, 9, 9], "deltas": [2, 2, 2]}',
          '--image_mean', '128', '--image_stddev', '33', '--batch_size', '2',
          '--seed', '7', '--train_dir', str(train_dir), '--checkpoint_steps',
          '3', '--optimizer', 'momentum', '--learning_rate', '0.01',
          '--section_augmentation', json.dumps(cpu.FULL)]
  assert train.main(argv + ['--max_steps', '3']) == 3
  saved = train.load_checkpoint(*train.checkpoint_paths(str(train_dir), 3))
  seen = {}
  make_trainer = train.make_trainer

  def spying(model, config, args):
    trainer = make_trainer(model, config, args)
    load_state = trainer.load_state

    def loading(state):
      load_state(state)
      seen['state'] = trainer.state()

    trainer.load_state = loading
    return trainer

  train.make_trainer = spying
  assert train.main(argv + ['--max_steps', '6']) == 6
  assert seen['state']['global_step'] == 3
  for got, want in zip([seen['state']['variables']] + seen['state']['slots'],
                       [saved['variables']] + saved['slots']):
    assert all(np.array_equal(got[k], want[k]) for k in want)
  final = train.load_checkpoint(*train.checkpoint_paths(str(train_dir), 6))
  assert all(np.isfinite(v).all() for v in final['variables'].values())
  with open(train_dir / 'summaries.jsonl') as f:
    lines = [json.loads(line) for line in f]
  assert [line['step'] for line in lines] == [3, 6]
  for line in lines:
    assert np.isfinite(line['loss'])
    assert line['augmentation/examples'] >= 2
    assert line['augmentation/misalignment'] == line['augmentation/examples']
    assert line['augmentation/grayscale'] == line['augmentation/examples']
    assert line['augmentation/outoffocus_sections'] >= 1
