"""The training loop without a GPU: the numpy restatement
(tests/training_ref.py) against the reference's own example plumbing
(tests/golden/ref_training.npz, minted by tools/make_golden_training.py),
BatchExampleIter with the unit and the trainer stubbed by the restatement,
PermuteAndReflect, and train.py's arguments and checkpoint files."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import coordinates_ref
from tests import evaluation_ref
from tests import gradients_ref
from tests import training_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ref_training.npz')


def _split(flat, lengths):
  out, pos = [], 0
  for n in lengths:
    out.append(flat[pos:pos + n])
    pos += n
  assert pos == len(flat)
  return out


def load_fixture():
  g = np.load(GOLDEN)
  fix = {k: g[k] for k in ('M', 'depth', 'fov_moves', 'batch', 'steps',
                           'learning_rate', 'variables_seed', 'tried',
                           'passed_over')}
  fix = {k: v.item() for k, v in fix.items()}
  fix['fov_xyz'] = tuple(int(v) for v in g['fov_xyz'])
  fix['deltas_xyz'] = tuple(int(v) for v in g['deltas_xyz'])
  fix['volume'] = dict(
      shape=tuple(int(v) for v in g['volume_shape_seed'][:3]),
      seed=int(g['volume_shape_seed'][3]),
      cells_per_96cube=float(g['volume_cells_offset_scale'][0]),
      offset=float(g['volume_cells_offset_scale'][1]),
      scale=float(g['volume_cells_offset_scale'][2]))
  fix['coordinates'] = [(tuple(int(v) for v in c), 'v') for c in g['centres']]
  fix['transforms'] = [
      (tuple(int(v) for v in p), tuple(int(v) for v in r))
      for p, r in zip(g['transform_perms'], g['transform_reflects'])]
  fix['variable_names'] = [str(n) for n in g['variable_names']]
  fix['cases'] = {}
  for name in [str(c) for c in g['cases']]:
    rows = g[name + '_examples']
    offsets = _split(g[name + '_offsets'], g[name + '_offsets_len'])
    records = _split(g[name + '_records'], g[name + '_records_len'])
    examples = []
    for row, offs, recs in zip(rows, offsets, records):
      examples.append({
          'coordinate': int(row[0]), 'slot': int(row[1]),
          'perm': tuple(int(v) for v in row[2:5]),
          'reflect': tuple(int(v) for v in row[5:8]),
          'finished': bool(row[8]),
          'offsets': [tuple(int(v) for v in o) for o in offs],
          'records': [(bool(r[0]), bool(r[1]), tuple(int(v) for v in r[2:]))
                      for r in recs]})
    fix['cases'][name] = dict(
        rule=str(g[name + '_rule']), bias=float(g[name + '_bias']),
        S=float(g[name + '_S']), margin=float(g[name + '_margin']),
        loss32=g[name + '_loss32'], loss64=g[name + '_loss64'],
        examples=examples, seeds=g[name + '_seeds'],
        variable_sums=g[name + '_variable_sums'],
        variable_samples=g[name + '_variable_samples'])
  return fix


FIXTURE = load_fixture() if os.path.exists(GOLDEN) else None
CASES = sorted(FIXTURE['cases']) if FIXTURE else []
_volumes = {}


def fixture_volumes():
  """{'v': (image u8, labels u64, offset, scale)}, generated once."""
  from ffn_amd import synthetic
  if not _volumes:
    v = FIXTURE['volume']
    _volumes['v'] = (
        synthetic.cells_volume(v['shape'], seed=v['seed'],
                               cells_per_96cube=v['cells_per_96cube']),
        synthetic.cells_labels(v['shape'], seed=v['seed'],
                               cells_per_96cube=v['cells_per_96cube']),
        v['offset'], v['scale'])
  return _volumes


def fixture_geometry():
  f = FIXTURE
  return evaluation_ref.geometry(f['fov_xyz'], f['fov_xyz'], f['fov_xyz'],
                                 f['deltas_xyz'], 'fixed', f['fov_moves'])


def fixture_variables(case):
  variables = gradients_ref.random_variables(
      FIXTURE['depth'], seed=FIXTURE['variables_seed'], stddev=0.05)
  variables['seed_update/conv_lom/biases'] = np.array([case['bias']],
                                                      np.float32)
  return variables


def sequences(examples):
  return [(e['coordinate'], e['slot'], e['perm'], e['reflect'], e['offsets'],
           e['records']) for e in examples]


def loss_bounds(case):
  """Per step: 4 x max(the stored |f32 - f64|, one f32 ulp of the loss), the
  factor of the gradient and optimizer tests."""
  ulp = np.spacing(case['loss32'].astype(np.float32)).astype(np.float64)
  return 4.0 * np.maximum(np.abs(case['loss32'] - case['loss64']), ulp)


class Replay:
  """Hands out the fixture's transforms in order, as the minter did."""

  permutable_axes = (0, 1, 2)

  def __init__(self, transforms):
    self.transforms = transforms
    self.k = 0

  def sample(self):
    out = self.transforms[self.k % len(self.transforms)]
    self.k += 1
    return out


class Info:
  """A ModelInfo: xyz arrays."""

  def __init__(self, fov_xyz, deltas_xyz):
    self.deltas = np.array(deltas_xyz)
    self.input_seed_size = np.array(fov_xyz)
    self.input_image_size = np.array(fov_xyz)
    self.pred_mask_size = np.array(fov_xyz)


def script(name):
  spec = importlib.util.spec_from_file_location(
      name + '_script', os.path.join(ROOT, name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


# ---- the fixture and the restatement ---------------------------------------------


def test_fixture_meets_the_conditions_it_was_minted_under():
  f = FIXTURE
  assert os.path.getsize(GOLDEN) < 300 * 1000
  assert f['M'] == 1e-3 and len(CASES) == 2
  assert 2 * f['passed_over'] <= f['tried']
  assert {f['cases'][c]['rule'] for c in CASES} == {'sgd', 'momentum'}
  for name in CASES:
    case = f['cases'][name]
    assert case['S'] <= f['M'] / 8 and case['margin'] >= f['M']
    assert len(case['loss32']) == len(case['loss64']) == f['steps']
    assert sum(len(e['offsets']) for e in case['examples']) == (
        f['steps'] * f['batch'])
    assert max(len(e['offsets']) for e in case['examples']) >= 3
    assert any(not valid for e in case['examples']
               for _, valid, _ in e['records'])
    assert any(e['perm'][2] != 2 for e in case['examples'])
    # examples start in slot order and take the coordinates in turn
    for k, e in enumerate(case['examples']):
      assert e['coordinate'] == k % len(f['coordinates'])
      assert (e['perm'], e['reflect']) == f['transforms'][
          k % len(f['transforms'])]


@pytest.fixture(scope='module', params=CASES)
def restated(request):
  case = FIXTURE['cases'][request.param]
  trainer = training_ref.RefTrainer(
      fixture_variables(case), FIXTURE['depth'], optimizer=case['rule'],
      learning_rate=FIXTURE['learning_rate'])
  run = training_ref.run_loop(
      trainer, fixture_volumes(), FIXTURE['coordinates'],
      FIXTURE['transforms'], fixture_geometry(), 'fixed', FIXTURE['batch'],
      FIXTURE['steps'])
  return case, trainer, run


def test_restatement_reproduces_the_stored_sequences(restated):
  case, _, run = restated
  assert sequences(run['examples']) == sequences(case['examples'])
  assert [e['finished'] for e in run['examples']] == [
      e['finished'] for e in case['examples']]
  assert min(run['margins']) >= FIXTURE['M']


def test_restatement_reproduces_losses_seeds_and_variables(restated):
  case, trainer, run = restated
  # torch's f32 conv order depends on the host: not bit for bit
  distance = np.abs(np.array(run['losses']) - case['loss32'])
  bounds = loss_bounds(case)
  print('largest loss distance %.3g, its bound %.3g' % (
      distance.max(), bounds[distance.argmax()]))
  assert (distance <= bounds).all()
  worst = max(float(np.abs(evaluation_ref.sample_seed(e['seed']).astype(
      np.float64) - want).max())
              for e, want in zip(run['examples'], case['seeds']))
  print('largest seed distance %.3g (bound %.3g)' % (worst, FIXTURE['M'] / 4))
  assert worst <= FIXTURE['M'] / 4
  # 30 updates of at most learning_rate * 0.7 per entry, each f32-rounded:
  # entries agree far below 1e-6
  for k, name in enumerate(FIXTURE['variable_names']):
    v = trainer.variables[name]
    got = v.ravel()[[0, v.size // 2, -1]]
    assert np.allclose(got, case['variable_samples'][k], rtol=0, atol=1e-6)
    assert abs(v.astype(np.float64).sum() - case['variable_sums'][k]) <= (
        1e-6 * v.size)


# ---- BatchExampleIter over the restatement ---------------------------------------


@pytest.mark.parametrize('name', CASES)
def test_batch_example_iter_reproduces_the_fixture(name):
  from ffn_amd.training import examples
  case = FIXTURE['cases'][name]
  ops = training_ref.RefOps()
  batches = examples.BatchExampleIter(
      Info(FIXTURE['fov_xyz'], FIXTURE['deltas_xyz']), ops, fixture_volumes(),
      FIXTURE['coordinates'], fov_policy='fixed',
      fov_moves=FIXTURE['fov_moves'], batch_size=FIXTURE['batch'],
      transform=Replay(FIXTURE['transforms']), keep_history=True)
  trainer = training_ref.RefTrainer(
      fixture_variables(case), FIXTURE['depth'], optimizer=case['rule'],
      learning_rate=FIXTURE['learning_rate'])
  weights = np.ones((FIXTURE['batch'],) + batches.geometry.pred_mask,
                    np.float32)
  for _ in range(FIXTURE['steps']):
    seed, image, labels, none = batches.next()
    assert none is None
    _, logits, _ = trainer.train_step_device(seed, image, labels, weights)
    batches.update_seeds(logits)
  assert sequences(batches.history) == sequences(case['examples'])
  finished = sum(e['finished'] for e in case['examples'])
  assert batches.examples_finished == finished
  assert batches.examples_started == len(case['examples'])
  assert batches.steps == FIXTURE['steps'] and batches.skipped == 0
  assert batches.result.num_patches == finished
  assert ops.calls['gather_train'] == FIXTURE['steps']
  assert ops.calls['gather'] == 0 and ops.calls['load'] == 0
  voxels = int(np.prod(batches.geometry.pred_mask))
  assert batches.result.fov_stats[0] == (
      FIXTURE['steps'] * FIXTURE['batch'] * voxels)
  moves = sum(len(e['records']) for e in batches.history)
  assert batches.result.summaries()['moves/total'] <= moves
  distance = np.abs(np.array(trainer.losses) - case['loss32'])
  assert (distance <= loss_bounds(case)).all()
  with pytest.raises(RuntimeError, match='update_seeds'):
    batches.next()
    batches.next()


def test_batch_example_iter_cycles_shuffles_and_skips():
  from ffn_amd.training import examples
  volumes = fixture_volumes()
  inside = FIXTURE['coordinates'][:3]
  outside = [((2, 20, 20), 'v'), ((20, 20, 38), 'v')]
  make = lambda **kw: examples.BatchExampleIter(
      Info(FIXTURE['fov_xyz'], FIXTURE['deltas_xyz']), training_ref.RefOps(),
      volumes, kw.pop('coordinates', inside + outside), batch_size=2,
      keep_history=True, **kw)

  def run(batches, steps):
    for _ in range(steps):
      seed, _, _, _ = batches.next()
      # a network that refuses every move: one step per example
      batches.update_seeds(np.full(seed.shape, -5.0, np.float32))
    return [e['coordinate'] for e in batches.history]

  plain = make()
  assert plain.skipped == 2 and len(plain.coordinates) == 3
  order = run(plain, 6)
  assert order[:9] == [0, 1, 2, 0, 1, 2, 0, 1, 2] and plain.epochs >= 3
  assert all(e['perm'] == (0, 1, 2) and e['reflect'] == (0, 0, 0)
             for e in plain.history)
  a, b = run(make(shuffle_seed=3), 9), run(make(shuffle_seed=3), 9)
  assert a == b
  for epoch in range(4):
    assert sorted(a[3 * epoch:3 * epoch + 3]) == [0, 1, 2]
  assert len({tuple(a[3 * e:3 * e + 3]) for e in range(6)}) > 1
  with pytest.raises(ValueError, match='none of the'):
    make(coordinates=outside)
  with pytest.raises(KeyError):
    make(coordinates=[((20, 20, 20), 'w')])
  with pytest.raises(ValueError, match='fov_policy'):
    make(fov_policy='no_step')
  # shuffle_moves: a permutation of the shifts, the same under one seed
  shifts = evaluation_ref.model_shifts(FIXTURE['deltas_xyz'])
  assert make().shifts == shifts
  s1 = make(shuffle_moves=True, moves_seed=4).shifts
  assert s1 == make(shuffle_moves=True, moves_seed=4).shifts
  assert s1 != shifts and sorted(s1) == sorted(shifts)


def test_batch_example_iter_max_pred_moves_over_the_restatement():
  """The other policy, against the independent generator restatement, with a
  network that is a fixed function of its inputs."""
  from ffn_amd.training import examples
  volumes = fixture_volumes()
  geom = evaluation_ref.geometry(FIXTURE['fov_xyz'], FIXTURE['fov_xyz'],
                                 FIXTURE['fov_xyz'], FIXTURE['deltas_xyz'],
                                 'max_pred_moves', 1)

  class Toy:
    global_step = 0

    def train_step_device(self, seed, image, labels, weights):
      return 0.0, evaluation_ref.toy_forward(seed, image), 0

  # the arrays hold one more move: 17^3 patches, which not every centre fits
  coordinates = [(c, n) for c, n in FIXTURE['coordinates']
                 if all(8 <= v <= 31 for v in c)]
  assert len(coordinates) >= 2
  want = training_ref.run_loop(Toy(), volumes, coordinates,
                               FIXTURE['transforms'], geom, 'max_pred_moves',
                               3, 12)
  batches = examples.BatchExampleIter(
      Info(FIXTURE['fov_xyz'], FIXTURE['deltas_xyz']), training_ref.RefOps(),
      volumes, coordinates, fov_policy='max_pred_moves',
      fov_moves=1, batch_size=3, transform=Replay(FIXTURE['transforms']),
      keep_history=True)
  assert tuple(batches.geometry.canvas) == geom['canvas']
  for _ in range(12):
    seed, image, _, _ = batches.next()
    batches.update_seeds(evaluation_ref.toy_forward(seed, image))
  assert sequences(batches.history) == sequences(want['examples'])
  assert max(len(e['offsets']) for e in batches.history) > 1


# ---- PermuteAndReflect -------------------------------------------------------------


def test_permute_and_reflect_validates_as_the_reference():
  from ffn_amd.training import augmentation
  P = augmentation.PermuteAndReflect
  with pytest.raises(ValueError, match='permutable_axes must not contain'):
    P([1, 1], [0])
  with pytest.raises(ValueError, match='reflectable_axes must not contain'):
    P([1, 2], [0, 0])
  with pytest.raises(ValueError, match='permutable_axes must be a subset'):
    P([1, 3], [0])
  with pytest.raises(ValueError, match='reflectable_axes must be a subset'):
    P([1, 2], [-1])
  assert P([], [], 0).sample() == ((0, 1, 2), (0, 0, 0))
  assert 'NOT reproduced' in augmentation.__doc__


@pytest.mark.parametrize('permutable,reflectable', [
    ((1, 2), (0, 1, 2)), ((0, 2), (1,)), ((0, 1, 2), ()), ((2, 1), (2, 0))])
def test_permute_and_reflect_samples(permutable, reflectable):
  from ffn_amd.training import augmentation
  make = lambda seed: augmentation.PermuteAndReflect(
      permutable, reflectable, np.random.default_rng(seed))
  a, b = make(5), make(5)
  draws = [a.sample() for _ in range(200)]
  assert draws == [b.sample() for _ in range(200)]
  assert draws != [s for s in (make(6).sample() for _ in range(200))]
  for perm, reflect in draws:
    assert sorted(perm) == [0, 1, 2]
    assert all(perm[a] == a for a in range(3) if a not in permutable)
    assert all(reflect[a] == 0 for a in range(3) if a not in reflectable)
    assert set(reflect) <= {0, 1}
  import math
  assert len({p for p, _ in draws}) == math.factorial(len(permutable))
  assert len({r for _, r in draws}) == 2 ** len(reflectable)
  # the documented use of the generator: decisions first, then the permutation
  rng = np.random.default_rng(5)
  decisions = rng.random(len(reflectable)) > 0.5
  permutation = rng.permutation(np.array(permutable, np.int32))
  perm, reflect = draws[0]
  assert [reflect[a] for a in reflectable] == [int(d) for d in decisions]
  assert [perm[a] for a in permutable] == [int(p) for p in permutation]


def test_apply_is_flip_of_transpose_for_all_48_transforms():
  from ffn_amd.training import augmentation
  x = np.arange(3 * 4 * 5, dtype=np.float32).reshape(3, 4, 5)
  transforms = training_ref.all_transforms()
  assert len(set(transforms)) == 48
  for perm, reflect in transforms:
    want = np.flip(np.transpose(x, perm),
                   [a for a in range(3) if reflect[a]])
    got = augmentation.apply(x, perm, reflect)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(training_ref.transform(x, perm, reflect), want)
    assert augmentation.keeps_shape(x.shape, perm) == (perm == (0, 1, 2))
  with pytest.raises(ValueError):
    augmentation.apply(x, (0, 1, 1), (0, 0, 0))
  with pytest.raises(ValueError):
    augmentation.apply(x, (0, 1, 2), (0, 2, 0))


def test_load_augmented_restatement_takes_the_mask_before_the_transform():
  """An even patch size: the centre index of the reflected patch is not the
  reflection of the centre index."""
  geom = evaluation_ref.geometry((6, 6, 6), (6, 6, 6), (6, 6, 6), (0, 0, 0),
                                 'fixed', 0)
  labels = np.zeros((8, 8, 8), np.uint64)
  labels[:, :, :5] = 5
  labels[:, :, 5:] = 9
  image = np.zeros((8, 8, 8), np.uint8)
  centre = (4, 3, 3)  # the patch covers x = 2 .. 7; its centre index 3 is x = 5
  plain = evaluation_ref.load(image, labels, centre, 0.0, 1.0, geom)[1]
  assert (plain[0, 0] > 0.5).tolist() == [False] * 3 + [True] * 3
  flipped = training_ref.load_augmented(image, labels, centre, 0.0, 1.0, geom,
                                        (0, 1, 2), (0, 0, 1))[1]
  assert np.array_equal(flipped, plain[:, :, ::-1])
  # (a mask taken after the reflection would compare with x = 4, label 5)
  assert flipped[3, 3, 3] == np.float32(0.05)
  with pytest.raises(ValueError):
    training_ref.load_augmented(
        image, labels, centre, 0.0, 1.0,
        dict(geom, image_patch=(4, 6, 6), label_patch=(4, 6, 6)), (2, 1, 0),
        (0, 0, 0))


# ---- train.py ----------------------------------------------------------------------

REQUIRED = ['--train_coords', 'c', '--data_volumes', 'a:i.npy',
            '--label_volumes', 'a:l.npy', '--model_name',
            'convstack_3d.ConvStack3DFFNModel', '--model_args', '{"depth": 3}']


def test_train_arguments_have_the_references_defaults(capsys):
  train = script('train')
  args = train.parse_args(REQUIRED + ['--image_mean', '128', '--image_stddev',
                                      '33'])
  # train.py:75-130 and ffn/training/optimizer.py of the reference
  want = dict(train_dir='/tmp', batch_size=4, max_steps=10000,
              summary_rate_secs=120, seed_pad=0.05, threshold=0.9,
              fov_policy='fixed', fov_moves=1, shuffle_moves=True,
              image_offset_scale_map=None, permutable_axes=[1, 2],
              reflectable_axes=[0, 1, 2], optimizer='sgd', learning_rate=0.001,
              momentum=0.9, learning_rate_decay_factor=None, decay_steps=None,
              rmsprop_decay=0.9, adam_beta1=0.9, adam_beta2=0.999,
              epsilon=1e-8, max_gradient_entry_mag=0.7, seed=None, device=0)
  for key, value in want.items():
    assert getattr(args, key) == value, key
  assert args.model_args == {'depth': 3} and args.data_volumes == ['a:i.npy']
  from ffn_amd.training import optimizer
  assert train.optimizer_config(args) == optimizer.OptimizerConfig()
  args = train.parse_args(REQUIRED + [
      '--image_offset_scale_map', 'a:120:40', '--permutable_axes', '0,1,2',
      '--reflectable_axes', '', '--shuffle_moves', 'false', '--optimizer',
      'adam', '--decay_steps', '100', '--learning_rate_decay_factor', '0.5',
      '--fov_policy', 'max_pred_moves', '--checkpoint_steps', '7'])
  assert args.permutable_axes == [0, 1, 2] and args.reflectable_axes == []
  assert args.shuffle_moves is False and args.checkpoint_steps == 7
  config = train.optimizer_config(args)
  assert (config.optimizer, config.decay_steps,
          config.learning_rate_decay_factor) == ('adam', 100, 0.5)
  for bad in (REQUIRED, REQUIRED + ['--image_mean', '1'],
              REQUIRED + ['--image_mean', '1', '--image_stddev', '1',
                          '--batch_size', '33'],
              REQUIRED + ['--image_mean', '1', '--image_stddev', '1',
                          '--fov_policy', 'no_step']):
    with pytest.raises(SystemExit):
      train.parse_args(bad)
  capsys.readouterr()


def trainer_state(rule, step, seed):
  """What ConvStackTrainer.state() returns, made on the host."""
  from ffn_amd.training import optimizer
  variables = gradients_ref.random_variables(3, seed=seed)
  config = optimizer.OptimizerConfig(optimizer=rule, learning_rate=0.01)
  slots = [{k: np.full(v.shape, init + 0.5 * n, np.float32)
            for k, v in variables.items()}
           for n, init in enumerate(optimizer.SLOT_INIT[rule])]
  return {'variables': variables, 'slots': slots, 'global_step': step,
          'beta1_power': np.float32(0.9) ** 3,
          'beta2_power': np.float32(0.999) ** 3, 'config': config.to_dict()}


@pytest.mark.parametrize('rule', ['sgd', 'momentum', 'adam'])
def test_checkpoint_pair_round_trips(tmp_path, rule):
  from ffn_amd.training import optimizer
  from ffn_amd.training.models import convstack_3d
  train = script('train')
  state = trainer_state(rule, 12, 3)
  paths = train.save_checkpoint(str(tmp_path), state)
  assert [os.path.basename(p) for p in paths] == [
      'model.ckpt-12.npz', 'model.ckpt-12.state.npz']
  assert sorted(os.listdir(tmp_path)) == sorted(os.path.basename(p)
                                                for p in paths)
  back = train.load_checkpoint(*paths)
  assert back['global_step'] == 12 and back['config'] == state['config']
  assert back['beta1_power'] == state['beta1_power']
  assert back['beta2_power'] == state['beta2_power']
  assert optimizer.OptimizerConfig.from_dict(back['config']).optimizer == rule
  assert len(back['slots']) == len(state['slots']) == len(
      optimizer.SLOT_INIT[rule])
  for got, want in zip([back['variables']] + back['slots'],
                       [state['variables']] + state['slots']):
    assert sorted(got) == sorted(want)
    for k in want:
      assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k])
  model = convstack_3d.ConvStack3DFFNModel(fov_size=[9, 9, 9],
                                           deltas=[2, 2, 2], depth=3)
  model.load_checkpoint(paths[0])
  for k, v in state['variables'].items():
    assert np.array_equal(model.variables[k], v)


def test_resume_takes_the_newest_complete_pair(tmp_path):
  train = script('train')
  assert train.newest_checkpoint(str(tmp_path / 'missing')) is None
  assert train.newest_checkpoint(str(tmp_path)) is None
  for step in (6, 100, 20):
    train.save_checkpoint(str(tmp_path), trainer_state('sgd', step, step))
  # a variables file without its state, other files: not a pair
  np.savez(str(tmp_path / 'model.ckpt-300.npz'), x=np.zeros(1))
  np.savez(str(tmp_path / 'model.ckpt-400.state.npz'), x=np.zeros(1))
  (tmp_path / 'model.ckpt-500.npz.tmp').write_bytes(b'')
  (tmp_path / 'summaries.jsonl').write_text('')
  step, variables_path, state_path = train.newest_checkpoint(str(tmp_path))
  assert step == 100
  assert train.load_checkpoint(variables_path, state_path)['global_step'] == 100
  want = gradients_ref.random_variables(3, seed=100)
  got = train.load_checkpoint(variables_path, state_path)['variables']
  assert all(np.array_equal(got[k], want[k]) for k in want)


def test_train_raises_without_the_device_library(tmp_path, monkeypatch):
  """No fallback: with the library (or the GPU) missing, the script raises
  before it writes anything."""
  from ffn_amd import _lib
  train = script('train')
  image, labels, _, _ = fixture_volumes()['v']
  np.save(tmp_path / 'image.npy', image)
  np.save(tmp_path / 'labels.npy', labels.astype(np.int64))
  centres = np.array([c for c, _ in FIXTURE['coordinates']], np.int64)
  (tmp_path / 'coords').write_bytes(coordinates_ref.tfrecord_bytes(
      centres, np.zeros(len(centres), np.int64), ['v']))

  def missing():
    raise _lib.FFNHipError('libffn_hip.so is not available')

  monkeypatch.setattr(_lib, 'load', missing)
  train_dir = tmp_path / 'run'
  with pytest.raises(_lib.FFNHipError, match='not available'):
    train.main(['--train_coords', str(tmp_path / 'coords'),
                '--data_volumes', 'v:%s' % (tmp_path / 'image.npy'),
                '--label_volumes', 'v:%s' % (tmp_path / 'labels.npy'),
                '--model_name', 'convstack_3d.ConvStack3DFFNModel',
                '--model_args', json.dumps({'depth': 3, 'fov_size': [9, 9, 9],
                                            'deltas': [2, 2, 2]}),
                '--image_mean', '128', '--image_stddev', '33',
                '--train_dir', str(train_dir), '--max_steps', '2',
                '--batch_size', '2', '--seed', '1'])
  assert not train_dir.exists() or not os.listdir(train_dir)
