"""The training loop on the GPU (include/ffn_evaluation.h load_augmented /
gather_train, ffn_amd/training/examples.py, trainer.train_step_device,
train.py): the two kernels against the numpy restatement
(tests/training_ref.py) bit for bit, and BatchExampleIter + ConvStackTrainer
against the reference's recorded runs (tests/golden/ref_training.npz).

End-to-end figures (MI355X; S is the fixture's f32-against-f64 spread of the
final seeds, the GPU column the largest |GPU - fixture| over the sampled seeds
in logit units, bound M / 4 = 2.5e-4; the loss column the largest |GPU loss -
fixture f32 loss| over the 30 steps next to its bound at that step): see
DESIGN.md 10.7."""
import importlib.util
import os

import numpy as np
import pytest

from tests import evaluation_ref
from tests import gradients_ref
from tests import test_training_loop as cpu
from tests import training_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = ((0, 1, 2), (0, 0, 0))


@pytest.fixture(scope='module')
def ev():
  from ffn_amd.training import evaluation
  return evaluation


@pytest.fixture(scope='module')
def ops(ev):
  return ev.default_ops(0)


@pytest.fixture(scope='module')
def torch():
  import torch as torch_module
  return torch_module


def make_geometry(ev, seed, pred, deltas, moves, slots):
  grow = lambda size, m: tuple(s + 2 * m * d for s, d in zip(size, deltas))
  return ev.Geometry(input_seed=seed, input_image=seed, pred_mask=pred,
                     deltas=deltas, canvas=grow(seed, moves),
                     image_patch=grow(seed, moves),
                     label_patch=grow(pred, moves), eval=grow(pred, moves),
                     slots=slots)


def patch_geometry(ev, patch, slots):
  """A geometry whose image and label patches are `patch` (zyx)."""
  inner = tuple(p - 2 for p in patch)
  g = make_geometry(ev, inner, inner, (1, 1, 1), 1, slots)
  assert g.image_patch == g.label_patch == g.canvas == tuple(patch)
  return g


def geom_dict(g):
  return {k: tuple(getattr(g, k)) for k in (
      'input_seed', 'input_image', 'pred_mask', 'deltas', 'canvas',
      'image_patch', 'label_patch', 'eval')}


def labelled_volume(shape, label_dtype, image_dtype, seed):
  """A random image, and labels of two slabs along each axis (eight blocks, no
  two alike under any transform) whose ids, as uint64, differ only above bit
  32; a band of background across y."""
  rng = np.random.RandomState(seed)
  if image_dtype == np.uint8:
    image = rng.randint(0, 256, shape).astype(np.uint8)
  else:
    image = rng.normal(100, 50, shape).astype(np.float32)
  ids = np.zeros(shape, np.uint64)
  z, y, x = np.indices(shape)
  block = ((z >= shape[0] // 2).astype(np.uint64) * np.uint64(4) +
           (y >= shape[1] // 2 + 1).astype(np.uint64) * np.uint64(2) +
           (x >= shape[2] // 2 - 1).astype(np.uint64))
  if label_dtype == np.uint64:
    ids = np.uint64(7) + (block << np.uint64(32))
  else:
    ids = np.uint64(7) + block
  ids[:, shape[1] // 3] = 0
  return image, ids.astype(label_dtype)


def device_array(torch, array):
  t = torch.from_numpy(np.ascontiguousarray(array)).to('cuda:0')
  torch.cuda.synchronize()
  return t


def read_slot(ops, s):
  return [ops.read_image(s), ops.read_labels(s), ops.read_seed(s)]


def same(a, b):
  return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def poison(ops, g, vol_nan, centre, slots):
  """NaN in the image and the seed of `slots` (an f32 volume of NaN, and
  write_seed); their labels are what load wrote."""
  n = len(slots)
  ops.load(slots, [vol_nan] * n, [centre] * n, [0.0] * n, [1.0] * n, 0.05)
  for s in slots:
    ops.write_seed(s, np.full(g.canvas, np.nan, np.float32))


# ---- load_augmented ----------------------------------------------------------------


@pytest.mark.parametrize('image_dtype,label_dtype', [
    (np.uint8, np.uint64), (np.float32, np.uint32)])
@pytest.mark.parametrize('size', [6, 9, 35, 67])
def test_load_augmented_all_48_transforms_on_cubes(ev, ops, size, image_dtype,
                                                   label_dtype):
  """Patch edges below a tile (9), across 32 (35), across a 64-voxel tile and
  64 lanes (67), and even (6: the mask is taken before the reflection)."""
  g = patch_geometry(ev, (size,) * 3, 32)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  shape = (size + 3, size + 2, size + 5)
  image, labels = labelled_volume(shape, label_dtype, image_dtype, size)
  # a second volume that is exactly one patch: it touches both corners
  tight = labelled_volume((size,) * 3, label_dtype, image_dtype, size + 1)
  vols = [ops.add_volume(image, labels), ops.add_volume(*tight)]
  data = [(image, labels), tight]
  lo = [(size - 1) // 2] * 3
  hi = [n - size + (size - 1) // 2 for n in shape]
  transforms = training_ref.all_transforms()
  rng = np.random.RandomState(size)
  seen_masks = set()
  for start, n in ((0, 32), (32, 16)):   # 32 slots in one call, then 16
    chunk = transforms[start:start + n]
    which = [1 if k % 7 == 3 else 0 for k in range(n)]
    centres = []
    for k in range(n):
      if which[k]:
        c = lo
      elif k % 3 == 0:
        c = hi
      else:
        c = [int(rng.randint(l, h + 1)) for l, h in zip(lo, hi)]
      centres.append(tuple(c[::-1]))
    offsets = [100.0 + k for k in range(n)]
    scales = [33.0 - 0.5 * k for k in range(n)]
    slot_ids = [int(s) for s in rng.permutation(32)[:n]]
    ops.load_augmented(slot_ids, [vols[w] for w in which], centres, offsets,
                       scales, [p for p, _ in chunk], [r for _, r in chunk],
                       0.05)
    for k, s in enumerate(slot_ids):
      want = training_ref.load_augmented(*data[which[k]], centres[k],
                                         offsets[k], scales[k], gd, *chunk[k])
      assert np.array_equal(ops.read_image(s), want[0]), (chunk[k], k)
      assert np.array_equal(ops.read_labels(s), want[1]), (chunk[k], k)
      assert np.array_equal(ops.read_seed(s), want[2]), (chunk[k], k)
      seen_masks.add(want[1].tobytes())
  assert len(seen_masks) > 8  # the label patches tell the transforms apart


@pytest.mark.parametrize('n', [1, 5])
def test_load_augmented_leaves_the_other_slots_alone(ev, ops, n):
  """Slots of NaN on both sides of every slot written."""
  size = 35
  g = patch_geometry(ev, (size,) * 3, 2 * n + 1)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  shape = (size + 2,) * 3
  image, labels = labelled_volume(shape, np.uint64, np.uint8, 3)
  vol = ops.add_volume(image, labels)
  vol_nan = ops.add_volume(np.full(shape, np.nan, np.float32), labels)
  centre = (size // 2 + 1,) * 3
  poison(ops, g, vol_nan, centre, list(range(g.slots)))
  guards = {s: read_slot(ops, s) for s in range(0, g.slots, 2)}
  assert all(np.isnan(a[0]).all() and np.isnan(a[2]).all()
             for a in guards.values())
  written = list(range(1, g.slots, 2))
  assert len(written) == n
  transforms = [((2, 1, 0), (1, 0, 1)), ((0, 1, 2), (0, 0, 1)),
                ((1, 2, 0), (0, 1, 0)), ((0, 2, 1), (1, 1, 1)),
                ((1, 0, 2), (0, 0, 0))][:n]
  ops.load_augmented(written, [vol] * n, [centre] * n, [128.0] * n, [33.0] * n,
                     [p for p, _ in transforms], [r for _, r in transforms],
                     0.05)
  for s, t in zip(written, transforms):
    want = training_ref.load_augmented(image, labels, centre, 128.0, 33.0, gd,
                                       *t)
    assert same(read_slot(ops, s), want), t
  for s, before in guards.items():
    assert same(read_slot(ops, s), before), s


def test_load_augmented_on_a_patch_that_is_no_cube(ev, ops):
  """(5, 9, 9) in zyx: y and x may change places, z may not."""
  g = patch_geometry(ev, (5, 9, 9), 16)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  shape = (7, 12, 13)
  image, labels = labelled_volume(shape, np.uint64, np.float32, 9)
  vol = ops.add_volume(image, labels)
  allowed = [t for t in training_ref.all_transforms()
             if t[0] in ((0, 1, 2), (0, 2, 1))]
  assert len(allowed) == 16
  centres = [(4 + k % 3, 4 + k % 2, 2 + k % 2) for k in range(16)]
  ops.load_augmented(list(range(16)), [vol] * 16, centres, [90.0] * 16,
                     [20.0] * 16, [p for p, _ in allowed],
                     [r for _, r in allowed], 0.05)
  for s, t in enumerate(allowed):
    want = training_ref.load_augmented(image, labels, centres[s], 90.0, 20.0,
                                       gd, *t)
    assert same(read_slot(ops, s), want), t
  before = [read_slot(ops, s) for s in range(16)]
  for perm in ((1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
    with pytest.raises(Exception, match='differ in patch size'):
      ops.load_augmented([0, 1], [vol] * 2, centres[:2], [0.0] * 2, [1.0] * 2,
                         [(0, 1, 2), perm], [(0, 0, 0)] * 2, 0.05)
  assert all(same(read_slot(ops, s), before[s]) for s in range(16))


def test_identity_equals_load_and_errors_touch_nothing(ev, ops):
  size = 9
  g = patch_geometry(ev, (size,) * 3, 4)
  ops.configure(g)
  ops.reset()
  shape = (size + 4,) * 3
  image, labels = labelled_volume(shape, np.int64, np.uint8, 5)
  vol = ops.add_volume(image, labels)
  centres = [(5, 6, 7), (4, 4, 4), (8, 8, 8), (6, 5, 4)]
  args = ([vol] * 4, centres, [128.0, 100.0, 0.0, 3.5], [33.0, 1.0, 2.0, 7.0])
  ops.load([0, 1, 2, 3], *args, 0.05)
  plain = [read_slot(ops, s) for s in range(4)]
  for s in range(4):
    ops.write_seed(s, np.full(g.canvas, np.nan, np.float32))
  ops.load_augmented([0, 1, 2, 3], *args, [IDENTITY[0]] * 4,
                     [IDENTITY[1]] * 4, 0.05)
  assert all(same(read_slot(ops, s), plain[s]) for s in range(4))
  # every argument error: all four slots as they were
  ops.load_augmented([3, 2, 1, 0], *args, [(2, 1, 0)] * 4, [(1, 1, 1)] * 4,
                     0.05)
  before = [read_slot(ops, s) for s in range(4)]
  assert not same(before[0], plain[0])
  ok_perm, ok_ref = [(0, 1, 2), (1, 0, 2)], [(0, 0, 0), (0, 1, 0)]
  two = lambda a: ([a[0][0]] * 2, a[1][:2], a[2][:2], a[3][:2])
  bad = [
      ('not a permutation', dict(perms=[(0, 1, 2), (0, 0, 1)])),
      ('not a permutation', dict(perms=[(0, 1, 3), (0, 1, 2)])),
      ('not a permutation', dict(perms=[(0, 1, 2), (-1, 1, 2)])),
      ('not 0 or 1', dict(reflects=[(0, 0, 0), (0, 2, 0)])),
      ('leave volume', dict(centres=[(5, 6, 7), (3, 4, 4)])),
      ('leave volume', dict(centres=[(5, 6, 9), (4, 4, 4)])),
      ('no volume', dict(volumes=[vol, vol + 1])),
      ('twice', dict(slots=[1, 1])),
      ('outside', dict(slots=[0, 4])),
  ]
  for message, change in bad:
    volumes, cs, offs, scs = two(args)
    call = dict(slots=[0, 1], volumes=volumes, centres=cs, perms=ok_perm,
                reflects=ok_ref)
    call.update(change)
    with pytest.raises(Exception, match=message):
      ops.load_augmented(call['slots'], call['volumes'], call['centres'], offs,
                         scs, call['perms'], call['reflects'], 0.05)
    assert all(same(read_slot(ops, s), before[s]) for s in range(4)), change
  with pytest.raises(Exception):
    ops.load_augmented([0], [vol], centres[:1], [0.0], [1.0], [(0, 1, 2)],
                       [(0, 0, -1)], 0.05)
  with pytest.raises(Exception):  # more entries than slots
    ops.load_augmented([0, 1, 2, 3, 0], [vol] * 5, centres + centres[:1],
                       [0.0] * 5, [1.0] * 5, [(0, 1, 2)] * 5, [(0, 0, 0)] * 5,
                       0.05)
  assert all(same(read_slot(ops, s), before[s]) for s in range(4))
  timing = ops.last_timing_train()
  assert set(timing) == {'load_augmented', 'gather_train'}
  ms, nbytes = timing['load_augmented']
  voxels = size ** 3
  assert ms > 0 and nbytes == 4 * (voxels * (1 + 8) + 3 * 4 * voxels)


# ---- gather_train ------------------------------------------------------------------

#: name -> (input_seed, pred_mask, deltas (all zyx), fov_moves, slots)
SHAPES = {
    'anisotropic_1': ((9, 13, 17), (7, 11, 15), (1, 2, 3), 1, 5),
    'anisotropic_2': ((9, 13, 17), (7, 11, 15), (1, 2, 3), 2, 32),
    'wide_x': ((5, 7, 67), (5, 7, 67), (1, 1, 4), 1, 5),
    'below_a_wave': ((3, 3, 5), (3, 3, 5), (1, 1, 1), 1, 1),
}


def all_offsets(deltas_zyx, moves):
  shifts = evaluation_ref.model_shifts(deltas_zyx[::-1])
  out = [(0, 0, 0)]
  for m in range(1, moves + 1):
    out += [tuple(m * v for v in s) for s in shifts]
  return out


@pytest.mark.parametrize('shape_name', sorted(SHAPES))
def test_gather_train_at_every_shift(ev, ops, torch, shape_name):
  seed, pred, deltas, moves, slots = SHAPES[shape_name]
  g = make_geometry(ev, seed, pred, deltas, moves, slots)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  rng = np.random.RandomState(11)
  shape = tuple(s + 4 for s in g.image_patch)
  image, labels = labelled_volume(shape, np.uint64, np.uint8, 11)
  vol = ops.add_volume(image, labels)
  lo = [(s - 1) // 2 for s in g.image_patch]
  centres = [tuple(int(l + rng.randint(0, 5)) for l in lo)[::-1]
             for _ in range(slots)]
  ops.load(list(range(slots)), [vol] * slots, centres, [128.0] * slots,
           [33.0] * slots, 0.05)
  state = []
  for s in range(slots):
    arrays = list(evaluation_ref.load(image, labels, centres[s], 128.0, 33.0,
                                      gd))
    arrays[2] = rng.permutation(arrays[2].size).astype(np.float32).reshape(
        g.canvas) * np.float32(0.37) - np.float32(50)
    ops.write_seed(s, arrays[2])
    state.append(arrays)
  make = lambda dims: torch.empty((slots,) + tuple(dims), dtype=torch.float32,
                                  device='cuda:0')
  io = [make(seed), make(seed), make(pred)]
  offsets = all_offsets(deltas, moves)
  assert tuple(-moves * d for d in deltas[::-1]) in offsets  # the extremes
  assert tuple(moves * d for d in deltas[::-1]) in offsets
  for start in range(0, len(offsets), slots):
    chunk = offsets[start:start + slots]
    slot_ids = [int(s) for s in rng.permutation(slots)[:len(chunk)]]
    n = len(chunk)
    for t in io:
      t.fill_(float('nan'))
    torch.cuda.synchronize()
    ops.gather_train(slot_ids, chunk, *io)
    got = [t.cpu().numpy() for t in io]
    for k, (s, off) in enumerate(zip(slot_ids, chunk)):
      want = training_ref.gather_train(state[s], off, gd)
      for a, b in zip(got, want):
        assert np.array_equal(a[k], b), off
    assert all(np.isnan(a[n:]).all() for a in got)
  # one step past the extreme offset: refused, the outputs keep their NaN
  for t in io:
    t.fill_(float('nan'))
  torch.cuda.synchronize()
  for axis in range(3):
    for sign in (-1, 1):
      past = [0, 0, 0]
      past[2 - axis] = sign * (moves * deltas[axis] + 1)
      with pytest.raises(Exception, match='out of its array'):
        ops.gather_train([0], [tuple(past)], *io)
  with pytest.raises(Exception, match='outside'):
    ops.gather_train([slots], [(0, 0, 0)], *io)
  assert all(np.isnan(t.cpu().numpy()).all() for t in io)
  # the unit's own buffers take the same call
  own = ops.alloc_io_train(slots)
  assert own[3].shape == (slots,) + pred and own[3].data_ptr() % 4 == 0
  ops.gather_train([0], [(0, 0, 0)], own[0], own[1], own[3])
  ms, nbytes = ops.last_timing_train()['gather_train']
  assert ms > 0 and nbytes == 8 * (2 * np.prod(seed) + np.prod(pred))


# ---- train_step_device -------------------------------------------------------------


def small_model(variables, depth=3, fov=(9, 9, 9), deltas=(2, 2, 2)):
  from ffn_amd.training.models import convstack_3d
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(fov), deltas=list(deltas),
                                       depth=depth)
  m.set_variables(variables)
  return m


def test_train_step_device_equals_train_step(torch):
  from ffn_amd.training import optimizer
  from ffn_amd.training import trainer as tr
  variables = gradients_ref.random_variables(3, seed=21, stddev=0.05)
  seed, image, labels, weights = gradients_ref.training_inputs(2, (9, 9, 9),
                                                               seed=4)
  cfg = optimizer.OptimizerConfig(optimizer='adam', learning_rate=0.01)
  a = tr.ConvStackTrainer(small_model(variables), cfg, max_batch=2)
  b = tr.ConvStackTrainer(small_model(variables), cfg, max_batch=2)
  try:
    for _ in range(2):
      loss_a, logits_a, step_a = a.train_step(seed, image, labels, weights)
      loss_b, logits_b, step_b = b.train_step_device(
          device_array(torch, seed), device_array(torch, image),
          device_array(torch, labels), device_array(torch, weights))
      assert isinstance(logits_a, np.ndarray)
      assert isinstance(logits_b, torch.Tensor) and logits_b.is_cuda
      assert loss_a == loss_b and step_a == step_b
      assert np.array_equal(logits_a, logits_b.cpu().numpy())
      seed = logits_a
    sa, sb = a.state(), b.state()
    assert sa['global_step'] == sb['global_step'] == 2
    assert sa['beta1_power'] == sb['beta1_power']
    for x, y in zip([sa['variables']] + sa['slots'],
                    [sb['variables']] + sb['slots']):
      assert all(np.array_equal(x[k], y[k]) for k in x)
  finally:
    a.close()
    b.close()


# ---- the minted runs ---------------------------------------------------------------


@pytest.mark.parametrize('name', cpu.CASES)
def test_loop_reproduces_the_reference_run(ev, ops, torch, name):
  from ffn_amd.training import examples
  from ffn_amd.training import optimizer
  from ffn_amd.training import trainer as tr
  F = cpu.FIXTURE
  case = F['cases'][name]
  model = small_model(cpu.fixture_variables(case), F['depth'], F['fov_xyz'],
                      F['deltas_xyz'])
  cfg = optimizer.OptimizerConfig(optimizer=case['rule'],
                                  learning_rate=F['learning_rate'])
  trainer = tr.ConvStackTrainer(model, cfg, max_batch=F['batch'])
  seeds = {}
  try:
    geometry = ev.Geometry.from_info(model.info, 'fixed', F['fov_moves'],
                                     F['batch'])
    batches = examples.BatchExampleIter(
        model.info, ops, cpu.fixture_volumes(), F['coordinates'],
        fov_policy='fixed', fov_moves=F['fov_moves'], batch_size=F['batch'],
        transform=cpu.Replay(F['transforms']), keep_history=True,
        io=examples.torch_io(geometry, F['batch'], trainer.device))
    finish = ops.finish

    def keeping(slot, *args):  # the final seed of the example the slot holds
      seeds[id(batches._current[slot])] = ops.read_seed(slot)
      return finish(slot, *args)

    ops.finish = keeping
    losses = []
    try:
      for _ in range(F['steps']):
        seed, image, labels, weights = batches.next()
        assert all(isinstance(t, torch.Tensor) for t in
                   (seed, image, labels, weights))
        loss, logits, _ = trainer.train_step_device(seed, image, labels,
                                                    weights)
        batches.update_seeds(logits)
        losses.append(loss)
    finally:
      del ops.finish
    for s in range(F['batch']):  # the examples still open
      seeds[id(batches._current[s])] = ops.read_seed(s)
  finally:
    trainer.close()
  assert cpu.sequences(batches.history) == cpu.sequences(case['examples'])
  assert len(seeds) == len(case['examples'])
  worst = max(float(np.abs(evaluation_ref.sample_seed(seeds[id(e)]).astype(
      np.float64) - want).max())
              for e, want in zip(batches.history, case['seeds']))
  distance = np.abs(np.array(losses) - case['loss32'])
  bounds = cpu.loss_bounds(case)
  k = int((distance / bounds).argmax())
  print('%s: S %.3g, GPU seed distance %.3g (bound %.3g); loss distance %.3g '
        'at step %d (bound %.3g), largest loss distance %.3g' % (
            name, case['S'], worst, F['M'] / 4, distance[k], k, bounds[k],
            distance.max()))
  assert worst <= F['M'] / 4
  assert (distance <= bounds).all()
  assert trainer.global_step == F['steps']


# ---- smoke: the flagship network through the loop -----------------------------------


@pytest.mark.parametrize('rule', ['sgd', 'momentum', 'adagrad', 'adam',
                                  'rmsprop'])
def test_three_steps_with_the_fib25_weights(ev, ops, torch, fib25_model, rule):
  from ffn_amd import synthetic
  from ffn_amd.training import augmentation
  from ffn_amd.training import examples
  from ffn_amd.training import optimizer
  from ffn_amd.training import trainer as tr
  shape = (64, 64, 64)
  volumes = {'a': (synthetic.cells_volume(shape, seed=11,
                                          cells_per_96cube=40.0),
                   synthetic.cells_labels(shape, seed=11,
                                          cells_per_96cube=40.0), 128.0, 33.0)}
  coordinates = [((30 + k, 32, 34 - k), 'a') for k in range(4)]
  trainer = tr.ConvStackTrainer(
      fib25_model, optimizer.OptimizerConfig(optimizer=rule), max_batch=2)
  try:
    geometry = ev.Geometry.from_info(fib25_model.info, 'fixed', 1, 2)
    batches = examples.BatchExampleIter(
        fib25_model.info, ops, volumes, coordinates, batch_size=2,
        transform=augmentation.PermuteAndReflect((1, 2), (0, 1, 2), 3),
        io=examples.torch_io(geometry, 2, trainer.device))
    fresh = np.full(geometry.canvas, ev.f32_logit(0.05), np.float32)
    fresh[tuple(c // 2 for c in geometry.canvas)] = ev.f32_logit(0.95)
    for _ in range(3):
      seed, image, labels, weights = batches.next()
      loss, logits, step = trainer.train_step_device(seed, image, labels,
                                                     weights)
      assert np.isfinite(loss)
      batches.update_seeds(logits)
    assert step == trainer.global_step == 3
    for values in [trainer.variables()] + trainer.slot_variables():
      assert all(np.isfinite(v).all() for v in values.values())
    for s in range(2):
      canvas = ops.read_seed(s)
      assert np.isfinite(canvas).all()
      assert (canvas != fresh).sum() > 33 ** 3 // 2  # the slot was pasted
  finally:
    trainer.close()


# ---- train.py end to end -----------------------------------------------------------


def script(name):
  spec = importlib.util.spec_from_file_location(
      name + '_script', os.path.join(ROOT, name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_train_script_writes_resumes_and_is_scored(ev, ops, tmp_path):
  from ffn_amd import engine as hip_engine
  from ffn_amd import synthetic
  from ffn_amd.training.models import convstack_3d
  shape = (64, 64, 64)
  image = synthetic.cells_volume(shape, seed=12, cells_per_96cube=40.0)
  labels = synthetic.cells_labels(shape, seed=12, cells_per_96cube=40.0)
  np.save(tmp_path / 'image.npy', image)
  np.save(tmp_path / 'labels.npy', labels)
  partitions = np.where(labels > 0, 1, 0).astype(np.uint8)
  partitions[:30] = partitions[34:] = 255  # a thin slab: a small file
  coords = str(tmp_path / 'coords')
  script('build_coordinates').build_coordinates(
      [('a', partitions)], (24, 24, 24), coords, seed=5)
  train = script('train')
  train_dir = tmp_path / 'run'
  model_args = '{"depth": 2, "fov_size": [33, 33, 33], "deltas": [8, 8, 8]}'
  argv = ['--train_coords', coords,
          '--data_volumes', 'a:%s' % (tmp_path / 'image.npy'),
          '--label_volumes', 'a:%s' % (tmp_path / 'labels.npy'),
          '--model_name', 'convstack_3d.ConvStack3DFFNModel',
          '--model_args', model_args, '--image_mean', '128',
          '--image_stddev', '33', '--batch_size', '2', '--seed', '7',
          '--train_dir', str(train_dir), '--checkpoint_steps', '4',
          '--optimizer', 'momentum', '--learning_rate', '0.01']
  assert train.main(argv + ['--max_steps', '6']) == 6
  files = sorted(os.listdir(train_dir))
  assert files == ['model.ckpt-4.npz', 'model.ckpt-4.state.npz',
                   'model.ckpt-6.npz', 'model.ckpt-6.state.npz',
                   'summaries.jsonl']
  saved = train.load_checkpoint(*train.checkpoint_paths(str(train_dir), 6))
  assert saved['global_step'] == 6 and len(saved['slots']) == 1

  # the resumed run starts from the saved state, bit for bit
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
  assert train.main(argv + ['--max_steps', '10']) == 10
  assert seen['state']['global_step'] == 6
  for got, want in zip([seen['state']['variables']] + seen['state']['slots'],
                       [saved['variables']] + saved['slots']):
    assert all(np.array_equal(got[k], want[k]) for k in want)
  assert 'model.ckpt-10.npz' in os.listdir(train_dir)
  assert 'model.ckpt-8.state.npz' in os.listdir(train_dir)
  final = train.load_checkpoint(*train.checkpoint_paths(str(train_dir), 10))
  assert final['global_step'] == 10
  assert any(not np.array_equal(final['variables'][k], saved['variables'][k])
             for k in saved['variables'])
  with open(train_dir / 'summaries.jsonl') as f:
    import json
    lines = [json.loads(line) for line in f]
  assert [line['step'] for line in lines] == [6, 10]
  assert all(np.isfinite(line['loss']) and
             abs(line['learning_rate'] - 0.01) < 1e-6 for line in lines)

  # the evaluator takes the checkpoint the script wrote
  model = convstack_3d.ConvStack3DFFNModel(fov_size=[33, 33, 33],
                                           deltas=[8, 8, 8], depth=2)
  model.load_checkpoint(str(train_dir / 'model.ckpt-10.npz'))
  eng = hip_engine.HipEngine.from_model(model, max_batch=2, device_id=0)
  try:
    from ffn_amd import coordinates
    centres, names = coordinates.read_tfrecord(coords)
    evaluator = ev.CheckpointEvaluator(model, eng, ops, 'fixed', 1,
                                       batch_size=2)
    evaluator.add_volume('a', image, labels, 128.0, 33.0)
    result = evaluator.evaluate(zip(centres.tolist(), names), max_examples=3)
    assert result.num_patches == 3 and np.isfinite(result.loss)
    assert 'eval/patch_loss' in result.summaries()
  finally:
    eng.close()
