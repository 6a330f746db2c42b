"""Forward-only evaluation without a GPU: the numpy restatement
(tests/evaluation_ref.py) against the reference's own training FoV loop
(tests/golden/ref_evaluation.npz, minted by tools/make_golden_evaluation.py),
CheckpointEvaluator's bookkeeping with the unit and the engine stubbed by the
restatement, the summary formulas against hand counts, and the script's
argument parsing and coordinate filtering."""
import json
import os

import numpy as np
import pytest

from tests import evaluation_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ref_evaluation.npz')
ACCUMULATORS = ('moves', 'loss', 'num_patches', 'num_voxels',
                'prediction_counts', 'fov_stats', 'moves_by_r', 'radii')


def _split(flat, lengths):
  out, pos = [], 0
  for n in lengths:
    out.append(flat[pos:pos + n])
    pos += n
  assert pos == len(flat)
  return out


def load_fixture():
  g = np.load(GOLDEN)
  fix = dict(M=float(g['M']), fov_xyz=tuple(int(v) for v in g['fov_xyz']),
             deltas_xyz=tuple(int(v) for v in g['deltas_xyz']),
             depth=int(g['depth']), volumes={}, cases={})
  for name in g['volume_names']:
    name = str(name)
    params = [int(v) for v in g['volume_%s' % name]]
    offset, scale = (float(v) for v in g['volume_%s_offset_scale' % name])
    fix['volumes'][name] = dict(shape=tuple(params[:3]), seed=params[3],
                                offset=offset, scale=scale)
  for case in g['cases']:
    case = str(case)
    offsets = [tuple(int(v) for v in o) for o in g[case + '_offsets']]
    records = [(bool(r[0]), bool(r[1]), tuple(int(v) for v in r[2:]))
               for r in g[case + '_records']]
    fix['cases'][case] = dict(
        policy=str(g[case + '_policy']), fov_moves=int(g[case + '_fov_moves']),
        coordinates=[(tuple(int(v) for v in c), str(n)) for c, n in
                     zip(g[case + '_centres'], g[case + '_volumes'])],
        offsets=_split(offsets, g[case + '_offsets_len']),
        records=_split(records, g[case + '_records_len']),
        S=float(g[case + '_S']), n_near=int(g[case + '_n_near']),
        seeds=g[case + '_seeds'],
        **{k: g['%s_%s' % (case, k)] for k in ACCUMULATORS})
  return fix


FIXTURE = load_fixture() if os.path.exists(GOLDEN) else None
CASES = sorted(FIXTURE['cases']) if FIXTURE else []
_volumes = {}


def fixture_volumes():
  """{name: (image u8, labels u64, offset, scale)}, generated once."""
  from ffn_amd import synthetic
  if not _volumes:
    for name, v in FIXTURE['volumes'].items():
      _volumes[name] = (synthetic.cells_volume(v['shape'], seed=v['seed']),
                        synthetic.cells_labels(v['shape'], seed=v['seed']),
                        v['offset'], v['scale'])
  return _volumes


def case_geometry(case):
  f = FIXTURE
  return evaluation_ref.geometry(f['fov_xyz'], f['fov_xyz'], f['fov_xyz'],
                                 f['deltas_xyz'], case['policy'],
                                 case['fov_moves'])


def test_fixture_has_the_cases_the_specification_names():
  assert set(CASES) == {'fixed', 'background', 'max_pred_moves', 'no_step'}
  assert os.path.getsize(GOLDEN) < 300 * 1000
  M = FIXTURE['M']
  assert M == 1e-3
  cases = FIXTURE['cases']
  fixed = cases['fixed']
  assert fixed['policy'] == 'fixed' and fixed['fov_moves'] == 1
  assert len(fixed['coordinates']) >= 6
  assert {n for _, n in fixed['coordinates']} == set(FIXTURE['volumes'])
  a, b = (FIXTURE['volumes'][n] for n in sorted(FIXTURE['volumes']))
  assert a['offset'] != b['offset'] and a['scale'] != b['scale']
  background = cases['background']
  assert background['offsets'] == [[(0, 0, 0)]]
  assert not any(w for w, _, o in background['records'][0] if o != (0, 0, 0))
  assert int(background['prediction_counts'][0]) == 0  # nothing true, none hit
  mp = cases['max_pred_moves']
  assert mp['policy'] == 'max_pred_moves' and mp['fov_moves'] == 1
  geom = case_geometry(mp)
  assert geom['label_patch'] == (65, 65, 65) and geom['eval'] == (49, 49, 49)
  assert list(mp['radii']) == [0, 8, 11, 13]
  assert mp['moves_by_r'][1:].sum() == 0  # everything under r = 0
  assert cases['no_step']['offsets'] == [[(0, 0, 0)]] * 3
  for case in cases.values():
    voxels = int(np.prod(case_geometry(case)['eval']))
    assert case['S'] <= M / 8
    assert case['n_near'] <= 0.002 * voxels * len(case['coordinates'])
    assert int(case['num_patches'][0]) == len(case['coordinates'])
    assert int(case['prediction_counts'].sum()) == int(case['num_voxels'][0])


@pytest.fixture(scope='module')
def oracle_forward(fib25_blob):
  from oracle import ffn_oracle
  depth = FIXTURE['depth']
  return lambda seed, image: ffn_oracle.forward(image, seed, fib25_blob, depth)


@pytest.mark.parametrize('name', CASES)
def test_restatement_reproduces_the_reference(name, oracle_forward):
  case = FIXTURE['cases'][name]
  geom = case_geometry(case)
  tracker, offsets, records, seeds = evaluation_ref.evaluate(
      oracle_forward, fixture_volumes(), case['coordinates'], geom,
      case['policy'])
  assert offsets == case['offsets']
  assert records == case['records']
  for key in ('moves', 'num_patches', 'num_voxels', 'prediction_counts',
              'fov_stats'):
    assert np.array_equal(getattr(tracker, key), case[key]), key
  assert sorted(tracker.moves_by_r) == list(case['radii'])
  for k, r in enumerate(case['radii']):
    assert np.array_equal(tracker.moves_by_r[int(r)], case['moves_by_r'][k])
  assert abs(float(tracker.loss[0]) - float(case['loss'][0])) <= (
      1e-12 * float(case['loss'][0]))
  got = np.stack([evaluation_ref.sample_seed(s) for s in seeds])
  assert np.array_equal(got, case['seeds'])


# ---- CheckpointEvaluator over the stubbed unit -----------------------------------


class ToyModel:
  """Carries `info` and `shifts` like ConvStack3DFFNModel; any geometry."""

  def __init__(self, seed_xyz, pred_xyz, deltas_xyz):
    from ffn_amd.training import model as model_lib
    info = model_lib.ModelInfo(deltas_xyz, pred_xyz, seed_xyz, seed_xyz)
    self.base = model_lib.FFNModel(info)
    self.info = self.base.info
    self.shifts = self.base.shifts


def toy_volumes(shape=(40, 44, 48), seed=7):
  rng = np.random.RandomState(seed)
  labels = np.zeros(shape, np.uint64)
  labels[:, :, :24] = 3
  labels[:, 22:, 24:] = 5
  labels[18:22] = 0
  image = np.where(labels > 0, 160, 60).astype(np.uint8)
  image += rng.randint(0, 8, shape).astype(np.uint8)
  return image, labels


def test_model_shifts_are_the_references():
  model = ToyModel((9, 7, 5), (9, 7, 5), (3, 2, 1))
  assert model.shifts == evaluation_ref.model_shifts((3, 2, 1))
  assert len(model.shifts) == 26 and model.shifts[0] == (-3, -2, -1)
  assert model.shifts[-1] == (3, 2, 1) and model.shifts[1] == (-3, -2, 0)


@pytest.mark.parametrize('policy', ['fixed', 'max_pred_moves', 'no_step'])
@pytest.mark.parametrize('batch_size', [1, 3, 8])
def test_evaluator_over_stub_equals_the_loop_restatement(policy, batch_size):
  from ffn_amd.training import evaluation
  model = ToyModel((11, 9, 9), (9, 7, 7), (3, 2, 2))
  image, labels = toy_volumes()
  other_image, other_labels = toy_volumes((36, 40, 52), seed=8)
  rng = np.random.RandomState(3)
  coords = [((int(rng.randint(14, 30)), int(rng.randint(13, 27)),
              int(rng.randint(12, 24))), 'ab'[k % 2]) for k in range(7)]
  coords.insert(2, ((2, 20, 20), 'a'))  # leaves the volume: skipped
  volumes = {'a': (image, labels, 100.0, 30.0),
             'b': (other_image, other_labels, 90.0, 25.0)}
  ops = evaluation_ref.RefOps()
  engine = evaluation_ref.RefEngine(evaluation_ref.toy_forward)
  ev = evaluation.CheckpointEvaluator(model, engine, ops, policy, 1,
                                      batch_size=batch_size)
  for name, v in volumes.items():
    ev.add_volume(name, *v)
  result = ev.evaluate(coords)
  assert result.skipped == 1

  geom = evaluation_ref.geometry((11, 9, 9), (11, 9, 9), (9, 7, 7), (3, 2, 2),
                                 policy, 1)
  assert {k: tuple(getattr(ev.geometry, k)) for k in geom} == geom
  kept = [c for c in coords if c[0] != (2, 20, 20)]
  tracker, offsets, records, _ = evaluation_ref.evaluate(
      evaluation_ref.toy_forward, volumes, kept, geom, policy)
  assert result.offsets == offsets
  assert result.records == records
  assert result.moves == tracker.moves.tolist()
  assert {r: v for r, v in result.moves_by_r.items()} == {
      r: v.tolist() for r, v in tracker.moves_by_r.items()}
  assert result.num_patches == len(kept)
  assert result.num_voxels == tracker.num_voxels.tolist()
  assert result.prediction_counts == tracker.prediction_counts.tolist()
  assert result.fov_stats == [float(v) for v in tracker.fov_stats]
  assert result.loss == pytest.approx(float(tracker.loss[0]), rel=1e-6)
  # the slots stay busy: every step but the tail runs the full batch
  full = min(batch_size, len(kept))
  assert max(engine.batches) == full
  assert sum(engine.batches) == sum(len(o) for o in offsets)
  tail = [n for n in engine.batches if n < full]
  assert engine.batches[:len(engine.batches) - len(tail)] == [full] * (
      len(engine.batches) - len(tail))
  if policy == 'fixed':
    assert max(len(o) for o in offsets) > 3  # the examples do move


def test_evaluator_takes_a_shift_list_or_a_seed():
  import random
  from ffn_amd.training import evaluation
  model = ToyModel((9, 9, 9), (9, 9, 9), (2, 2, 2))
  make = lambda batch_size=2, **kw: evaluation.CheckpointEvaluator(
      model, evaluation_ref.RefEngine(evaluation_ref.toy_forward),
      evaluation_ref.RefOps(), 'fixed', 1, batch_size=batch_size, **kw)
  assert make().shifts == model.shifts
  mine = list(reversed(model.shifts))
  assert make(shifts=mine).shifts == mine
  want = list(model.shifts)
  random.Random(5).shuffle(want)
  assert make(shuffle_seed=5).shifts == want and want != model.shifts
  with pytest.raises(ValueError):
    evaluation.Geometry.from_info(model.info, 'fixed_offsets_window', 1, 1)
  with pytest.raises(ValueError):
    make(batch_size=33)


def test_thresholds_are_exact_for_float32_values():
  from ffn_amd.training import evaluation
  t = evaluation.logit(0.9)
  c = evaluation.ceil_f32(t)
  below = np.nextafter(c, np.float32(-np.inf))
  assert float(c) >= t > float(below)
  assert evaluation.ceil_f32(0.5) == np.float32(0.5)
  from scipy import special
  assert evaluation.f32_logit(0.05) == special.logit(np.float32(0.05))
  assert evaluation.f32_logit(0.95).dtype == np.float32
  assert t == float(special.logit(0.9))


# ---- summaries ---------------------------------------------------------------------


def test_summaries_against_hand_counts():
  from ffn_amd.training import evaluation
  r = evaluation.EvalResult([(8, 0, 0), (8, 8, 0), (8, 8, 8)])
  assert sorted(r.moves_by_r) == [0, 8, 11, 13]
  assert r.summaries() == {}  # no patch yet, as the reference
  r.record_move(True, True, (0, 0, 0))     # correct
  r.record_move(True, False, (8, 0, 0))    # missed
  r.record_move(False, True, (8, 8, 0))    # spurious
  r.record_move(False, False, (8, 8, 8))   # not counted
  r.record_move(True, True, (8, 0, 0))
  r.track_weights(1000)
  r.add_patch(0.5, [30, 50, 10, 10], 100, 0)
  r.add_patch(0.25, [0, 90, 10, 0], 100, 0)
  s = r.summaries()
  assert r.moves == [2, 1, 1]
  assert s['moves/total'] == 4
  assert s['moves/all/correct'] == 0.5 and s['moves/all/missed'] == 0.25
  assert s['moves/all/spurious'] == 0.25
  assert s['moves/r=8/correct'] == 0.5 and s['moves/r=8/missed'] == 0.5
  assert s['moves/r=8/total'] == 2 and s['moves/r=11/spurious'] == 1.0
  # max(..., 1): a radius without moves
  assert s['moves/r=13/total'] == 1 and s['moves/r=13/correct'] == 0.0
  assert s['eval/patches'] == 2 and s['eval/patch_loss'] == 0.375
  assert s['eval/all/accuracy'] == 170 / 200
  assert s['eval/all/precision'] == 30 / 50
  assert s['eval/all/recall'] == 30 / 40
  assert s['eval/all/specificity'] == 140 / 160
  assert s['eval/all/f1'] == pytest.approx(2 * 0.6 * 0.75 / 1.35)
  assert s['masked_voxel_fraction'] == 0.0
  assert s['fov/masked_voxel_fraction'] == 0.0 and s['fov/average_weight'] == 1.0
  assert set(s) == {
      'fov/masked_voxel_fraction', 'fov/average_weight', 'masked_voxel_fraction',
      'eval/patch_loss', 'eval/patches', 'moves/total', 'moves/all/correct',
      'moves/all/missed', 'moves/all/spurious', 'eval/all/accuracy',
      'eval/all/precision', 'eval/all/recall', 'eval/all/specificity',
      'eval/all/f1'} | {'moves/r=%d/%s' % (rr, k) for rr in (0, 8, 11, 13)
                        for k in ('correct', 'spurious', 'missed', 'total')}


def test_summaries_guards_and_the_f1_zero_branch():
  from ffn_amd.training import evaluation
  r = evaluation.EvalResult([])
  r.add_patch(1.0, [0, 40, 0, 0], 40, 0)  # nothing predicted, nothing true
  s = r.summaries()
  assert s['eval/all/precision'] == 0.0 and s['eval/all/recall'] == 0.0
  assert s['eval/all/f1'] == 0.0
  assert s['eval/all/accuracy'] == 1.0 and s['eval/all/specificity'] == 1.0
  assert s['moves/total'] == 1 and s['moves/all/correct'] == 0.0
  assert s['fov/average_weight'] == 0.0  # max(total voxels, 1)
  r2 = evaluation.EvalResult([])
  r2.add_patch(1.0, [0, 0, 0, 7], 7, 0)  # only misses: tn + fp = 0
  assert r2.summaries()['eval/all/specificity'] == 0.0
  assert r2.summaries()['eval/all/f1'] == 0.0
  with pytest.raises(ValueError):
    r.record_move(True, True, (8, 0, 0))  # a radius the shifts do not have


def test_summaries_of_a_minted_case_follow_the_accumulators():
  from ffn_amd.training import evaluation
  case = FIXTURE['cases']['fixed']
  r = evaluation.EvalResult(evaluation_ref.model_shifts(FIXTURE['deltas_xyz']))
  r.moves = case['moves'].tolist()
  r.moves_by_r = {int(k): v.tolist() for k, v in
                  zip(case['radii'], case['moves_by_r'])}
  r.loss = float(case['loss'][0])
  r.num_patches = int(case['num_patches'][0])
  r.num_voxels = case['num_voxels'].tolist()
  r.prediction_counts = case['prediction_counts'].tolist()
  r.fov_stats = case['fov_stats'].tolist()
  s = r.summaries()
  tp, tn, fp, fn = r.prediction_counts
  assert s['eval/all/recall'] == tp / (tp + fn)
  assert s['moves/total'] == sum(r.moves)
  assert s['eval/patch_loss'] == r.loss / 6


# ---- the script --------------------------------------------------------------------


def _script():
  import importlib.util
  spec = importlib.util.spec_from_file_location(
      'evaluate_checkpoint_script', os.path.join(ROOT, 'evaluate_checkpoint.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_script_volume_specs_and_offset_scale_map():
  script = _script()
  assert script.split_volume_spec('a:x.npy') == ('a', 'x.npy', None)
  assert script.split_volume_spec('a:x.npz:raw') == ('a', 'x.npz', 'raw')
  assert script.split_volume_spec('a:x.h5:stack') == ('a', 'x.h5', 'stack')
  for bad in ('x.npy', 'a:x.npz', 'a:', 'a:x.npy:extra', 'a:x.h5'):
    with pytest.raises(ValueError):
      script.split_volume_spec(bad)
  assert script.offset_scale_map(['a:120:40', 'b:1.5:2']) == {
      'a': (120.0, 40.0), 'b': (1.5, 2.0)}
  with pytest.raises(ValueError):
    script.offset_scale_map(['a:120'])
  args = script.parse_args([
      '--train_coords', 'c', '--data_volumes', 'a:i.npy,b:j.npy',
      '--label_volumes', 'a:l.npy,b:m.npy', '--checkpoint', 'w.npz',
      '--model_args', '{"depth": 12, "fov_size": [33, 33, 33], '
      '"deltas": [8, 8, 8]}', '--image_mean', '128', '--image_stddev', '33'])
  assert args.batch_size == 4 and args.fov_policy == 'fixed'
  assert args.fov_moves == 1 and args.threshold == 0.9 and args.seed_pad == 0.05
  assert args.model_name == 'convstack_3d.ConvStack3DFFNModel'
  assert args.data_volumes == ['a:i.npy', 'b:j.npy']
  with pytest.raises(SystemExit):  # neither mean / stddev nor a map
    script.parse_args(['--train_coords', 'c', '--data_volumes', 'a:i.npy',
                       '--label_volumes', 'a:l.npy', '--checkpoint', 'w.npz',
                       '--model_args', '{}'])
  with pytest.raises(SystemExit):
    script.parse_args(['--train_coords', 'c', '--data_volumes', 'a:i.npy',
                       '--label_volumes', 'a:l.npy', '--checkpoint', 'w.npz',
                       '--model_args', '{}', '--image_mean', '1',
                       '--image_stddev', '1', '--fov_policy', 'window'])


def test_script_filters_coordinates_and_writes_json(tmp_path, monkeypatch):
  """End to end on .npy inputs and an uncompressed TFRecord file, the unit and
  the engine stubbed by the restatement."""
  from tests import coordinates_ref
  script = _script()
  image, labels = toy_volumes()
  np.save(tmp_path / 'image.npy', image)
  np.save(tmp_path / 'labels.npy', labels)
  centres = np.array([[20, 22, 18], [2, 20, 20], [26, 20, 22], [24, 24, 60],
                      [22, 18, 20]], np.int64)
  names = ['vol'] * 5
  coords_path = str(tmp_path / 'coords')
  with open(coords_path, 'wb') as f:
    f.write(coordinates_ref.tfrecord_bytes(centres, [0] * 5, ['vol']))
  model = ToyModel((11, 9, 9), (9, 7, 7), (3, 2, 2))
  made = {}

  def make_backend(args, loaded_model):
    made['model_args'] = args.model_args
    return (model, evaluation_ref.RefEngine(evaluation_ref.toy_forward),
            evaluation_ref.RefOps())

  monkeypatch.setattr(script, 'make_backend', make_backend)
  out = str(tmp_path / 'out.json')
  result = script.main([
      '--train_coords', coords_path,
      '--data_volumes', 'vol:%s' % (tmp_path / 'image.npy'),
      '--label_volumes', 'vol:%s' % (tmp_path / 'labels.npy'),
      '--checkpoint', 'unused.npz', '--model_args',
      '{"depth": 2, "fov_size": [11, 9, 9], "deltas": [3, 2, 2]}',
      '--image_offset_scale_map', 'vol:100:30', '--batch_size', '2',
      '--max_examples', '2', '--output', out])
  with open(out) as f:
    written = json.load(f)
  assert written['skipped'] == 1 and written['examples'] == 2
  assert written['accumulators']['num_patches'] == 2
  assert written['summaries'] == json.loads(json.dumps(result.summaries()))
  assert written['summaries']['eval/patches'] == 2
  geom = evaluation_ref.geometry((11, 9, 9), (11, 9, 9), (9, 7, 7), (3, 2, 2),
                                 'fixed', 1)
  tracker, offsets, _, _ = evaluation_ref.evaluate(
      evaluation_ref.toy_forward, {'vol': (image, labels, 100.0, 30.0)},
      [((20, 22, 18), 'vol'), ((26, 20, 22), 'vol')], geom, 'fixed')
  assert result.offsets == offsets
  assert written['accumulators']['prediction_counts'] == (
      tracker.prediction_counts.tolist())
  assert names and made['model_args']['depth'] == 2
