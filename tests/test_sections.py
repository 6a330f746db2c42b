"""The section augmentations without a GPU: the sampler against the reference's
own decisions and outputs (tests/golden/ref_sections.npz, minted by
tools/make_golden_sections.py from the unmodified ffn/training/augmentation.py),
the two numpy statements against each other, argument validation,
BatchExampleIter with plans over the restated unit, and train.py's flag.

The yardstick: per case E_ref = max |ref f32 - ref f64|, at
least one f32 ulp of the case's largest value; a result equals the f32
reference bit for bit on every voxel that neither blur nor gray writes and
lies within 4 E_ref of the f64 reference everywhere."""
import json
import os

import numpy as np
import pytest

from tests import evaluation_ref
from tests import sections_ref
from tests import test_training_loop as loop
from tests import training_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ref_sections.npz')

FULL = dict(misalignment_skip_ratio=0.0, max_xy_offset=2,
            slip_vs_translate_ratio=0.5, missing_section_skip_ratio=0.0,
            max_missing_section_indices_ratio=0.6, outoffocus_skip_ratio=0.0,
            max_outoffocus_indices_ratio=0.6, max_filter_stdev=2.0,
            grayscale_skip_ratio=0.0, max_contrast_factor=0.6,
            max_brightness_factor=0.6)


def load_fixture():
  g = np.load(GOLDEN)
  cases = {}
  for name in [str(c) for c in g['cases']]:
    image_zyx, label_zyx = [tuple(int(v) for v in s) for s in g[name + '_sizes']]
    cases[name] = dict(
        config=json.loads(str(g[name + '_config'])),
        seed=int(g[name + '_seed']), image_zyx=image_zyx, label_zyx=label_zyx,
        margin=tuple(int(v) for v in g[name + '_margin']),
        image=g[name + '_image'], labels=g[name + '_labels'].astype(np.uint64),
        ref32=g[name + '_ref32'], ref64=g[name + '_ref64'],
        ref_labels=g[name + '_ref_labels'].astype(np.uint64),
        summary=json.loads(str(g[name + '_summary'])))
  return cases


FIXTURE = load_fixture()
CASES = sorted(FIXTURE)


def centre_of(case):
  """(x, y, z): the voxel the fixture's boxes are centred on."""
  return tuple((s - 1) // 2 for s in case['image'].shape)[::-1]


def sampled_plan(case):
  from ffn_amd.training import augmentation
  sampler = augmentation.SectionAugmentations(
      dict(case['config'], margin_yx=case['margin']),
      np.random.RandomState(case['seed']))
  return sampler.sample(case['image_zyx'], case['label_zyx'])


def boxes(case):
  c = centre_of(case)
  return (sections_ref.box_of(case['image'], c, case['image_zyx'],
                              case['margin']),
          sections_ref.box_of(case['labels'], c, case['label_zyx'],
                              case['margin']))


def exact_voxels(plan, shape_yx):
  return ~(sections_ref.touched(plan, shape_yx, 'blur') |
           sections_ref.touched(plan, shape_yx, 'gray'))


# ---- the fixture, the sampler and the restatement ---------------------------------


def test_fixture_covers_what_it_says():
  assert os.path.getsize(GOLDEN) < 300 * 1000 and len(CASES) >= 24
  kinds = set()
  for case in FIXTURE.values():
    assert all(a <= b for a, b in zip(case['image_zyx'], (6, 35, 67)))
    assert case['ref32'].dtype == np.float32
    assert case['ref64'].dtype == np.float64
    s = case['summary']
    kinds |= {k for k in ('missing_z', 'outoffocus_z') if s[k]}
    kinds |= {'moved'} if s['misalignment_z'] >= 0 else set()
    kinds |= {'gray'} if s['grayscale'] else {'no_gray'}
  assert kinds == {'missing_z', 'outoffocus_z', 'moved', 'gray', 'no_gray'}
  assert any(c['margin'] == (0, 0) and c['summary']['misalignment_z'] >= 0
             for c in FIXTURE.values())  # a visible wrap


@pytest.mark.parametrize('name', CASES)
def test_sampler_takes_the_references_decisions(name):
  """Under the case's seed the sampled plan, carried out by the restatement,
  gives what the reference's functions gave."""
  case = FIXTURE[name]
  plan = sampled_plan(case)
  assert plan.summary() == case['summary']
  image, labels = sections_ref.apply(*boxes(case), plan, case['image_zyx'],
                                     case['label_zyx'])
  assert np.array_equal(labels, case['ref_labels'])
  exact = exact_voxels(plan, case['image_zyx'][1:])
  ok, distance, bound = sections_ref.within(image, case['ref32'],
                                            case['ref64'], exact)
  print('%s: distance to f64 %.3g, bound %.3g, E_ref %.3g, exact voxels %d '
        'of %d' % (name, distance, bound, bound / 4, exact.sum(), exact.size))
  assert ok
  if not (plan.blur_mask.any() or plan.gray.any()):
    assert np.array_equal(image, case['ref32'])  # misalignment, missing section


@pytest.mark.parametrize('name', CASES)
def test_apply_sections_equals_the_restatement_on_the_fixture(name):
  from ffn_amd.training import augmentation
  case = FIXTURE[name]
  plan = sampled_plan(case)
  got = augmentation.apply_sections(*boxes(case), plan)
  want = sections_ref.apply(*boxes(case), plan, case['image_zyx'],
                            case['label_zyx'])
  assert got[0].dtype == np.float32 and got[1].dtype == want[1].dtype
  assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
  again = augmentation.SectionAugmentations.apply(*boxes(case), plan,
                                                  case['image_zyx'],
                                                  case['label_zyx'])
  assert np.array_equal(again[0], want[0])


SHAPES = [((5, 9, 11), (3, 5, 7), (2, 2)), ((6, 6, 6), (6, 6, 6), (0, 0)),
          ((4, 7, 9), (6, 9, 5), (1, 3)), ((1, 3, 2), (1, 3, 2), (0, 0))]


def random_boxes(rng, image_zyx, label_zyx, margin, dtype=np.uint8):
  grow = lambda s: (s[0], s[1] + 2 * margin[0], s[2] + 2 * margin[1])
  image = rng.randint(0, 256, grow(image_zyx)).astype(dtype)
  if dtype == np.float32:
    image = image + rng.rand(*image.shape).astype(np.float32)
  return image, rng.randint(0, 5, grow(label_zyx)).astype(np.int64)


def test_apply_sections_equals_the_restatement_on_random_plans():
  """Every shape class: label patch smaller / equal / larger in z than the
  image patch, unequal margins, a plane below the blur radius (multiple
  reflections: max_filter_stdev 7.5 gives radii up to 30 on 3 x 2 planes)."""
  from ffn_amd.training import augmentation
  seen = set()
  for seed in range(120):
    image_zyx, label_zyx, margin = SHAPES[seed % len(SHAPES)]
    config = dict(FULL, margin_yx=margin, max_filter_stdev=7.5,
                  max_brightness_factor=2.5,
                  **({'misalignment_skip_ratio': 0.2,
                      'grayscale_skip_ratio': 0.2} if seed % 3 else {}))
    plan = augmentation.SectionAugmentations(config, seed).sample(image_zyx,
                                                                  label_zyx)
    image, labels = random_boxes(np.random.RandomState(seed), image_zyx,
                                 label_zyx, margin,
                                 np.float32 if seed % 2 else np.uint8)
    got = augmentation.apply_sections(image, labels, plan)
    want = sections_ref.apply(image, labels, plan, image_zyx, label_zyx)
    assert np.array_equal(got[0], want[0]), seed
    assert np.array_equal(got[1], want[1]), seed
    seen.add((plan.kind, augmentation.blur_radius(plan.blur_sigma) > 12,
              bool((want[0] == 0).any()), bool((want[0] == 255).any())))
  assert {k for k, _, _, _ in seen} == {0, 1, 2}
  assert any(wide for _, wide, _, _ in seen)
  assert any(lo and hi for _, _, lo, hi in seen)  # clipped on both sides


def test_the_empty_plan_is_the_centre_crop():
  from ffn_amd.training import augmentation
  rng = np.random.RandomState(3)
  for image_zyx, label_zyx, margin in SHAPES:
    image, labels = random_boxes(rng, image_zyx, label_zyx, margin)
    plan = augmentation.SectionPlan(image_zyx[0], margin)
    assert plan.is_empty()
    got = augmentation.apply_sections(image, labels, plan)
    crop = lambda a: a[:, margin[0]:a.shape[1] - margin[0],
                       margin[1]:a.shape[2] - margin[1]]
    assert np.array_equal(got[0], crop(image).astype(np.float32))
    assert np.array_equal(got[1], crop(labels))


def test_sampler_draws_in_the_documented_order():
  """The legacy generator, call for call (augmentation.py:739-987)."""
  from ffn_amd.training import augmentation
  image_zyx, label_zyx = (5, 9, 11), (7, 5, 7)
  for seed in range(40):
    plan = augmentation.SectionAugmentations(FULL, seed).sample(image_zyx,
                                                                label_zyx)
    rng = np.random.RandomState(seed)
    assert not rng.rand() < 0.0
    dy, dx = rng.randint(-2, 3, 2)
    z0 = rng.randint(0, 7)  # the padded z size
    slip = rng.rand() < 0.5
    assert (plan.dy, plan.dx, plan.z0, plan.kind) == (dy, dx, z0,
                                                      1 if slip else 2)
    assert plan.margin_yx == (2, 2)

    def chosen(mask, yx):
      zs = rng.choice(5, rng.randint(1, max(int(0.6 * 5), 1) + 1),
                      replace=False)
      value = rng.rand()
      for z in zs:
        if rng.rand() < 0.5:
          assert (mask[z], tuple(yx[z])) == (8, (0, 0))
        else:
          bits = rng.rand(4) < 0.5
          y, x = rng.randint(0, 9), rng.randint(0, 11)
          assert mask[z] == sum(int(b) << k for k, b in enumerate(bits))
          assert tuple(yx[z]) == (y, x)
      return zs, value

    assert not rng.rand() < 0.0
    zs, value = chosen(plan.blank_mask, plan.blank_yx)
    assert plan.blank_value == np.float32(value * 256)
    assert sorted(zs) == plan.summary()['missing_z']
    assert not rng.rand() < 0.0
    zs, value = chosen(plan.blur_mask, plan.blur_yx)
    assert plan.blur_sigma == np.float32(value * 2.0)
    assert not rng.rand() < 0.0
    whole = rng.rand() < 0.5
    rows = []
    for _ in range(1 if whole else 5):
      rows.append((1 + (rng.rand() - 0.5) * 0.6, (rng.rand() - 0.5) * 0.6,
                   2.0 ** (rng.rand() * 2 - 1)))
    want = np.array(rows * (5 if whole else 1), np.float32)
    assert np.array_equal(plan.factors, want) and plan.gray.all()
  # an augmentation that is off draws nothing; a ratio of 1 draws once
  off = augmentation.SectionAugmentations({}, 5)
  assert off.sample(image_zyx, label_zyx).is_empty()
  assert off.rng.rand() == np.random.RandomState(5).rand()
  skipping = augmentation.SectionAugmentations(
      {k: (1.0 if k.endswith('skip_ratio') else v) for k, v in FULL.items()},
      5)
  assert skipping.sample(image_zyx, label_zyx).is_empty()
  rng = np.random.RandomState(5)
  rng.rand(4)
  assert skipping.rng.rand() == rng.rand()


# ---- validation --------------------------------------------------------------------


def test_config_validation():
  from ffn_amd.training import augmentation
  S = augmentation.SectionAugmentations
  for key in ('elastic_warp_skip_ratio', 'num_control_points_ratio',
              'affine_transform_skip_ratio', 'rotation_max', 'shear_max'):
    with pytest.raises(ValueError, match='not implemented .*skimage'):
      S(dict(FULL, **{key: 0.5}))
  with pytest.raises(ValueError, match='unknown'):
    S(dict(FULL, max_xy_offsets=2))
  with pytest.raises(ValueError, match='needs all of'):
    S({'max_xy_offset': 2})
  with pytest.raises(ValueError, match='negative'):
    S(dict(FULL, max_filter_stdev=-1.0))
  with pytest.raises(ValueError, match='radius'):
    S(dict(FULL, max_filter_stdev=8.0))
  with pytest.raises(ValueError, match='integer'):
    S(dict(FULL, max_xy_offset=1.5))
  with pytest.raises(ValueError, match='margin'):
    S(dict(FULL, margin_yx=(-1, 0)))
  only_gray = S({k: FULL[k] for k in augmentation.SECTION_KEYS['grayscale']},
                1)
  assert only_gray.margin_yx == (0, 0)
  plan = only_gray.sample((3, 4, 5), (3, 4, 5))
  assert plan.kind == 0 and plan.gray.all() and not plan.blur_mask.any()
  assert S(FULL, 1).margin_yx == (2, 2)
  assert S(dict(FULL, margin_yx=(1, 3)), 1).margin_yx == (1, 3)
  assert isinstance(S(FULL, 1).rng, np.random.RandomState)
  assert 'not reproduced' in augmentation.__doc__
  assert 'elastic_warp' in augmentation.__doc__


def test_plan_validation():
  from ffn_amd.training import augmentation
  image_zyx, label_zyx = (5, 9, 11), (3, 5, 7)
  rng = np.random.RandomState(0)
  image, labels = random_boxes(rng, image_zyx, label_zyx, (1, 1))

  def refused(message, **change):
    plan = augmentation.SectionPlan(5, (1, 1))
    for key, value in change.items():
      if isinstance(value, tuple) and key != 'margin_yx':
        getattr(plan, key)[value[0]] = value[1]
      else:
        setattr(plan, key, value)
    with pytest.raises(ValueError, match=message):
      augmentation.check_plan(plan, image_zyx, label_zyx)
    if key != 'margin_yx':
      with pytest.raises(ValueError, match=message):
        augmentation.apply_sections(image, labels, plan)

  refused('kind', kind=3)
  refused('z0', kind=1, z0=5)
  refused('z0', z0=-1)
  refused('exceeds', kind=2, dy=12)   # M_y = 9 + 2
  refused('exceeds', kind=2, dx=-14)  # M_x = 11 + 2
  refused('blur_sigma', blur_sigma=np.float32(-0.5))
  refused('blur_sigma', blur_sigma=np.float32(np.nan))
  refused('blur_sigma', blur_sigma=np.float32(7.9))  # r = 32
  refused('split point', blank_yx=(2, (10, 0)))
  refused('split point', blur_yx=(0, (0, -1)))
  refused('four bits', blank_mask=(1, 16))
  refused('gray is', gray=(0, 2))
  refused('gamma', gray=(0, 1))  # the factors are still zero
  refused('margin', margin_yx=(-1, 1))
  ok = augmentation.SectionPlan(5, (1, 1))
  ok.kind, ok.z0, ok.dy, ok.dx = 2, 4, 11, -13
  ok.blur_sigma = np.float32(7.8)
  ok.blank_yx[2] = (9, 11)
  augmentation.check_plan(ok, image_zyx, label_zyx)
  with pytest.raises(ValueError, match='sections'):
    augmentation.check_plan(augmentation.SectionPlan(4), image_zyx, label_zyx)
  with pytest.raises(ValueError, match='not the final sizes'):
    augmentation.apply_sections(image, labels, ok, (5, 9, 11), (3, 5, 5))
  big = augmentation.SectionPlan(1)
  big.blur_sigma, big.blur_mask[0] = np.float32(1.0), 8
  with pytest.raises(ValueError, match='16384'):
    augmentation.check_plan(big, (1, 128, 129), (1, 128, 129))
  augmentation.check_plan(big, (1, 128, 128), (1, 128, 128))


def test_ctypes_mirror_of_the_plan(tmp_path):
  """sizeof / offsetof of the two structs as gcc lays them out, and what
  section_plan_arrays writes into them."""
  import ctypes
  import subprocess
  from ffn_amd import _lib
  from ffn_amd.training import augmentation
  from ffn_amd.training import evaluation
  structs = {
      'ffn_evaluation_section_plan': (_lib.EvaluationSectionPlan, [
          'margin_yx', 'kind', 'z0', 'dy', 'dx', 'blank_value', 'blur_sigma']),
      'ffn_evaluation_section': (_lib.EvaluationSection, [
          'blank_mask', 'blur_mask', 'gray', 'reserved', 'blank_yx', 'blur_yx',
          'contrast', 'brightness', 'gamma'])}
  lines = ['#include <stdio.h>', '#include <stddef.h>',
           '#include "ffn_evaluation.h"', 'int main(void) {']
  for name, (_, fields) in structs.items():
    lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
    for f in fields:
      lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' %
                   (name, f, name, f))
  lines += ['  return 0;', '}']
  (tmp_path / 'layout.c').write_text('\n'.join(lines))
  subprocess.check_call(['gcc', '-std=c11', '-I', os.path.join(ROOT, 'include'),
                         '-o', str(tmp_path / 'layout'),
                         str(tmp_path / 'layout.c')])
  out = dict(l.split() for l in subprocess.check_output(
      [str(tmp_path / 'layout')]).decode().splitlines())
  for name, (cls, fields) in structs.items():
    assert int(out[name]) == ctypes.sizeof(cls), name
    for f in fields:
      assert int(out['%s.%s' % (name, f)]) == getattr(cls, f).offset, (name, f)
  assert evaluation.PLAN_DTYPE.itemsize == 32
  assert evaluation.SECTION_DTYPE.itemsize == 32
  plan = augmentation.SectionAugmentations(FULL, 3).sample((5, 9, 11),
                                                           (3, 5, 7))
  plans, sections = evaluation.section_plan_arrays(
      [augmentation.SectionPlan(5), plan], 5)
  assert plans.shape == (2,) and sections.shape == (2, 5)
  assert not plans[0].tobytes().strip(b'\0')
  assert not sections[0].tobytes().strip(b'\0')
  first = _lib.EvaluationSectionPlan.from_buffer_copy(plans[1].tobytes())
  assert (tuple(first.margin_yx), first.kind, first.z0, first.dy, first.dx) == (
      plan.margin_yx, plan.kind, plan.z0, plan.dy, plan.dx)
  assert np.float32(first.blur_sigma) == plan.blur_sigma
  for z in range(5):
    row = _lib.EvaluationSection.from_buffer_copy(sections[1, z].tobytes())
    assert (row.blank_mask, row.blur_mask, row.gray) == (
        plan.blank_mask[z], plan.blur_mask[z], plan.gray[z])
    assert tuple(row.blur_yx) == tuple(plan.blur_yx[z])
    assert [np.float32(v) for v in (row.contrast, row.brightness,
                                    row.gamma)] == list(plan.factors[z])
  with pytest.raises(ValueError, match='sections'):
    evaluation.section_plan_arrays([augmentation.SectionPlan(4)], 5)


# ---- BatchExampleIter --------------------------------------------------------------


def make_batches(ops, sections=None, transform=None, **kw):
  from ffn_amd.training import examples
  F = loop.FIXTURE
  return examples.BatchExampleIter(
      loop.Info(F['fov_xyz'], F['deltas_xyz']), ops, loop.fixture_volumes(),
      kw.pop('coordinates', F['coordinates']), fov_policy='fixed',
      fov_moves=F['fov_moves'], batch_size=2, transform=transform,
      sections=sections, keep_history=True, **kw)


def run(batches, steps):
  for _ in range(steps):
    seed, image, _, _ = batches.next()
    batches.update_seeds(evaluation_ref.toy_forward(seed, image))


def test_without_sections_the_stream_is_the_parents():
  """sections=None takes load_augmented and draws what the parent drew: the
  history equals the independent restatement of the parent's loop."""
  from ffn_amd.training import augmentation
  F = loop.FIXTURE
  transform = augmentation.PermuteAndReflect((0, 1, 2), (0, 1, 2), 11)
  ops = sections_ref.RefOps()
  batches = make_batches(ops, None, transform)
  run(batches, 10)
  assert ops.calls['load_sections'] == 0 and ops.calls['load_augmented'] > 0
  assert all('plan' not in e for e in batches.history)
  replay = augmentation.PermuteAndReflect((0, 1, 2), (0, 1, 2), 11)
  transforms = [replay.sample() for _ in batches.history]
  assert [(e['perm'], e['reflect']) for e in batches.history] == transforms
  assert transform.rng.random() == replay.rng.random()  # no draw besides

  class Toy:
    def train_step_device(self, seed, image, labels, weights):
      return 0.0, evaluation_ref.toy_forward(seed, image), 0

  want = training_ref.run_loop(Toy(), loop.fixture_volumes(), F['coordinates'],
                               transforms, loop.fixture_geometry(), 'fixed', 2,
                               10)
  assert loop.sequences(batches.history) == loop.sequences(want['examples'])
  # sections that are all off: load_sections, the same stream, no draw from
  # the transform's generator more
  ops2 = sections_ref.RefOps()
  off = make_batches(ops2, augmentation.SectionAugmentations({}, 4),
                     augmentation.PermuteAndReflect((0, 1, 2), (0, 1, 2), 11))
  run(off, 10)
  assert ops2.calls['load_augmented'] == 0 and ops2.calls['load_sections'] > 0
  assert loop.sequences(off.history) == loop.sequences(batches.history)
  assert all(e['plan'].is_empty() for e in off.history)
  for s in range(2):
    assert all(np.array_equal(a, b) for a, b in zip(ops.slots[s],
                                                    ops2.slots[s]))


def test_batch_example_iter_with_sections_over_the_restatement():
  from ffn_amd.training import augmentation
  F = loop.FIXTURE
  transform = augmentation.PermuteAndReflect((0, 1, 2), (0, 1, 2), 11)
  sections = augmentation.SectionAugmentations(FULL, 21)
  ops = sections_ref.RefOps()
  batches = make_batches(ops, sections, transform)
  run(batches, 40)
  replay = augmentation.SectionAugmentations(FULL, 21)
  g = batches.geometry
  plans = [replay.sample(g.image_patch, g.label_patch) for _ in batches.history]
  assert [e['plan'] for e in batches.history] == plans
  assert len(set(plans)) == len(plans) > 2
  transforms = [(e['perm'], e['reflect']) for e in batches.history]
  want = sections_ref.run_loop(evaluation_ref.toy_forward,
                               loop.fixture_volumes(), batches.coordinates,
                               transforms, plans, loop.fixture_geometry(), 2,
                               40)
  assert 0 < batches.skipped < len(F['coordinates'])  # the margin tells
  assert loop.sequences(batches.history) == loop.sequences(want)
  counts = batches.section_counts
  assert counts['examples'] == batches.examples_started == len(plans)
  assert counts['misalignment'] == counts['grayscale'] == len(plans)
  assert counts['missing_sections'] == sum(len(p.summary()['missing_z'])
                                           for p in plans)
  assert counts['outoffocus_sections'] >= len(plans)


def test_the_enlarged_box_decides_which_coordinates_fit():
  from ffn_amd.training import augmentation
  from ffn_amd.training import examples
  F = loop.FIXTURE
  shape = F['volume']['shape']
  g = make_batches(sections_ref.RefOps()).geometry
  half = [(s - 1) // 2 for s in g.image_patch]
  # y at its lowest without a margin: fits only there
  edge = ((20, half[1], 20), 'v')
  assert examples.fits(edge[0], shape, g)
  assert not examples.fits(edge[0], shape, g, (1, 0))
  assert examples.fits(edge[0], shape, g, (0, 2))
  assert not examples.fits((shape[2] - 1 - g.image_patch[2] // 2 - 1, 20, 20),
                           shape, g, (0, 2))
  inside = [((20, 20, 20), 'v'), ((18, 21, 19), 'v')]
  plain = make_batches(sections_ref.RefOps(), coordinates=inside + [edge])
  assert plain.skipped == 0
  sections = augmentation.SectionAugmentations(FULL, 1)
  grown = make_batches(sections_ref.RefOps(), sections,
                       coordinates=inside + [edge])
  assert grown.skipped == 1 and len(grown.coordinates) == 2


# ---- train.py ----------------------------------------------------------------------


def test_train_flag(capsys):
  train = loop.script('train')
  base = loop.REQUIRED + ['--image_mean', '128', '--image_stddev', '33']
  assert train.parse_args(base).section_augmentation is None
  args = train.parse_args(base + ['--section_augmentation', json.dumps(FULL)])
  assert args.section_augmentation == FULL
  for bad in ('[1]', '{"rotation_max": 0.1}', '{"max_xy_offset": 2}',
              '{"max_filter_stdev": 9, "outoffocus_skip_ratio": 0, '
              '"max_outoffocus_indices_ratio": 0.5}', 'not json'):
    with pytest.raises(SystemExit):
      train.parse_args(base + ['--section_augmentation', bad])
  assert 'not implemented' in capsys.readouterr().err
