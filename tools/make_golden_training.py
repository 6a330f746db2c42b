#!/usr/bin/env python3
"""Mints tests/golden/ref_training.npz with the reference's own example
plumbing: ffn/training/examples.py (get_example, BatchExampleIter and its
update_seeds, fixed_offsets), mask.py and tracker.py of the google/ffn
checkout, imported through tools/ref_shims as tools/make_golden_evaluation.py
imports them, and driven for a few training steps at batch size 2.

Runs in the build container only (needs the reference checkout).  What stands
in for the reference's surroundings, besides what make_golden_evaluation.py
states for TensorFlow and the tracker:

  * `load_example` serves numpy patches built as train.py:232-274 builds them:
    the label box turned into a soft local object mask, all-one weights, the
    transform on labels, image and weights, then the image less offset, divided
    by scale.
  * The transform.  The reference's augmentation.py imports TensorFlow and
    cannot run here, so PermuteAndReflect is numpy's `transpose` and `flip` on
    the [1, z, y, x, 1] arrays, with the decisions drawn once from a seeded
    generator and stored in the fixture.
  * The "session" is the restated train step (tests/training_ref.RefTrainer:
    gradients_ref.run + optimizer_ref.Optimizer), run once in float32 and once
    in float64.  The seed canvases are float32 in both.
  * `_batch_gen` asks its generators from a thread pool; here the pool runs
    each call where it is submitted, so the generators take their coordinates
    in slot order, which is what ffn_amd/training/examples.py defines.

The volume comes from ffn_amd/synthetic.py; the file stores the generator
parameters, not voxels.  Per case it stores the coordinates, per example
started its coordinate, slot, transform, offsets and (wanted, valid, offset)
records, per step the loss of both runs, the final (or, for the examples still
open, current) seeds sampled with evaluation_ref.sample_seed, and per final
variable its float64 sum and a few entries.

Conditions, with M = 1e-3 logit units.  A configuration that
breaks one is passed over; at most half of those tried may be, their number is
stored, and M is never loosened.
  * the f32 and f64 runs take identical offset and record sequences;
  * every seed value compared with the move threshold lies at least M from it
    in both runs;
  * S, the largest |f32 - f64| over the final seeds, is at most M / 8;
  * the run holds an example of at least 3 steps, a refused move, and a
    transform that moves x.
Adam, adagrad and rmsprop amplify rounding too much to qualify (DESIGN.md
10.7); only sgd and momentum runs are minted.
The numpy restatement of the loop (tests/training_ref.run_loop) must reproduce
every stored sequence, loss and seed.
"""
import functools
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, ROOT)

import make_golden_evaluation as base  # noqa: E402  (sets the reference's paths)
import numpy as np  # noqa: E402
from scipy import ndimage  # noqa: E402
from scipy import special  # noqa: E402

from ffn_amd import synthetic  # noqa: E402
from ffn_amd.training import augmentation  # noqa: E402
from tests import evaluation_ref  # noqa: E402
from tests import gradients_ref  # noqa: E402
from tests import training_ref  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
MAX_BYTES = 300 * 1000
M = evaluation_ref.M
DEPTH = 3
FOV_XYZ = (9, 9, 9)
DELTAS_XYZ = (2, 2, 2)
FOV_MOVES = 1
BATCH = 2
STEPS = 30
LEARNING_RATE = 0.001
VOLUME = {'shape': (40, 40, 40), 'seed': 4, 'cells_per_96cube': 25.0,
          'offset': 128.0, 'scale': 33.0}
N_COORDINATES = 8
COORDINATE_SEED = 5
TRANSFORM_SEED = 7
N_TRANSFORMS = 16
VARIABLES_SEED = 1
#: (optimizer, conv_lom bias), in the order tried; the first WANTED that meet
#: every condition are minted
CONFIGURATIONS = [('sgd', 5.6), ('momentum', 5.7), ('sgd', 5.5),
                  ('momentum', 5.5)]
WANTED = 2


class SerialPool:
  """futures.ThreadPoolExecutor that runs a call where it is submitted."""

  def __init__(self, max_workers=None):
    del max_workers

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    return False

  def submit(self, fn, *args):
    value = fn(*args)
    return types.SimpleNamespace(result=lambda: value)


def make_volume():
  v = VOLUME
  return (synthetic.cells_volume(v['shape'], seed=v['seed'],
                                 cells_per_96cube=v['cells_per_96cube']),
          synthetic.cells_labels(v['shape'], seed=v['seed'],
                                 cells_per_96cube=v['cells_per_96cube']),
          v['offset'], v['scale'])


def make_coordinates(labels, geom):
  """Seeded voxels at least 2 from a membrane, far enough from the border."""
  rng = np.random.RandomState(COORDINATE_SEED)
  ok = ndimage.distance_transform_edt(labels > 0) >= 2
  for a in range(3):
    margin = max(geom['image_patch'][a], geom['label_patch'][a]) // 2 + 1
    sel = [slice(None)] * 3
    for s in (slice(None, margin), slice(-margin, None)):
      sel[a] = s
      ok[tuple(sel)] = False
  pool = np.argwhere(ok)
  picks = pool[rng.choice(len(pool), N_COORDINATES, replace=False)]
  return [((int(x), int(y), int(z)), 'v') for z, y, x in picks]


def make_transforms():
  sampler = augmentation.PermuteAndReflect(
      (0, 1, 2), (0, 1, 2), np.random.default_rng(TRANSFORM_SEED))
  return [sampler.sample() for _ in range(N_TRANSFORMS)]


def make_variables(bias):
  variables = gradients_ref.random_variables(DEPTH, seed=VARIABLES_SEED,
                                             stddev=0.05)
  variables['seed_update/conv_lom/biases'] = np.array([bias], np.float32)
  return variables


def run_reference(mods, trainer, volumes, coordinates, transforms, geom):
  """The reference's loop for STEPS steps -> (log of examples in starting
  order, losses)."""
  examples, tracker_lib, model_lib = mods
  examples.futures = types.SimpleNamespace(ThreadPoolExecutor=SerialPool)
  info = model_lib.ModelInfo(np.array(DELTAS_XYZ), np.array(FOV_XYZ),
                             np.array(FOV_XYZ), np.array(FOV_XYZ))
  shifts = evaluation_ref.model_shifts(DELTAS_XYZ)
  eval_tracker = tracker_lib.EvalTracker(list(geom['eval']), shifts)
  log = []
  active = [None]  # the log entry of the generator that is running

  def load_example(slot):
    k = len(log)
    index = k % len(coordinates)
    centre, name = coordinates[index]
    perm, reflect = transforms[k % len(transforms)]
    image_volume, label_volume, offset, scale = volumes[name]
    lab = evaluation_ref.patch_of(label_volume, centre, geom['label_patch'])
    lab = lab.reshape((1,) + lab.shape + (1,))
    radii = [s // 2 for s in geom['label_patch']]
    lom = np.logical_and(lab > 0,
                         lab == lab[0, radii[0], radii[1], radii[2], 0])
    labels = np.where(lom, np.float32(0.95), np.float32(0.05))
    weights = np.ones(labels.shape, np.float32)
    patch = evaluation_ref.patch_of(image_volume, centre, geom['image_patch'])
    patch = patch.reshape((1,) + patch.shape + (1,))

    def transform_axes(x):  # rank 5: the zyx axes are 1, 2, 3
      x = np.transpose(x, (0,) + tuple(p + 1 for p in perm) + (4,))
      axes = tuple(a + 1 for a in range(3) if reflect[a])
      return np.flip(x, axes) if axes else x

    labels = transform_axes(labels)
    patch = transform_axes(patch)
    weights = transform_axes(weights)
    patch = (patch.astype(np.float32) - np.float32(offset)) / np.float32(scale)
    assert patch.dtype == np.float32 and labels.dtype == np.float32
    entry = {'coordinate': index, 'slot': slot, 'perm': tuple(perm),
             'reflect': tuple(reflect), 'offsets': [], 'records': [],
             'seed': None, 'finished': False}
    log.append(entry)
    active[0] = entry
    return patch, labels, weights, np.array([centre]), name

  record_move = eval_tracker.record_move

  def recording(wanted, executed, offset_xyz):
    active[0]['records'].append((bool(wanted), bool(executed),
                                 tuple(int(v) for v in offset_xyz)))
    record_move(wanted, executed, offset_xyz)

  eval_tracker.record_move = recording
  policy = functools.partial(examples.fixed_offsets, fov_shifts=shifts,
                             threshold=special.logit(0.9))

  def noting(info_, seed, labels, tracker_):
    entry = active[0]  # set by the load_example call just before
    entry['seed'] = seed
    walk = policy(info_, seed, labels, tracker_)
    while True:
      active[0] = entry
      try:
        off = next(walk)
      except StopIteration:
        break
      entry['offsets'].append(tuple(int(v) for v in off))
      yield off
    entry['finished'] = True

  slots = iter(range(BATCH))

  def make_example():
    slot = next(slots)
    return examples.get_example(functools.partial(load_example, slot),
                                eval_tracker, info, noting, 0.05,
                                seed_shape=geom['canvas'])

  batch_it = examples.BatchExampleIter(make_example, eval_tracker, BATCH, info)
  losses = []
  for _ in range(STEPS):
    seed, patches, labels, weights = next(batch_it)
    loss, logits, _ = trainer.train_step_device(
        seed[..., 0], patches[..., 0], labels[..., 0], weights[..., 0])
    losses.append(loss)
    batch_it.update_seeds(logits[..., np.newaxis])
  for entry in log:
    entry['seed'] = np.array(entry['seed'][0, ..., 0])
  return log, losses


def sequences(log):
  return [(e['coordinate'], e['slot'], e['perm'], e['reflect'], e['offsets'],
           e['records'], e['finished']) for e in log]


def try_configuration(mods, rule, bias, volumes, coordinates, transforms, geom):
  """-> (reason it is passed over, None) or (None, results)."""
  runs = []
  for f64 in (False, True):
    trainer = training_ref.RefTrainer(make_variables(bias), DEPTH, f64=f64,
                                      optimizer=rule,
                                      learning_rate=LEARNING_RATE)
    log, losses = run_reference(mods, trainer, volumes, coordinates,
                                transforms, geom)
    mine_trainer = training_ref.RefTrainer(make_variables(bias), DEPTH,
                                           f64=f64, optimizer=rule,
                                           learning_rate=LEARNING_RATE)
    mine = training_ref.run_loop(mine_trainer, volumes, coordinates,
                                 transforms, geom, 'fixed', BATCH, STEPS)
    # the restatement takes the same steps on the same numbers
    assert sequences(mine['examples']) == sequences(log), (rule, bias)
    assert mine['losses'] == losses, (rule, bias)
    for a, b in zip(mine['examples'], log):
      assert np.array_equal(a['seed'], b['seed']), (rule, bias)
    runs.append((log, losses, mine['margins'], trainer.variables))
  (log32, loss32, margins32, vars32), (log64, loss64, margins64, _) = runs
  if sequences(log32) != sequences(log64):
    return 'the f32 and f64 runs take different steps', None
  margin = min(margins32 + margins64)
  if margin < M:
    return 'a compared seed value lies %.3g from the threshold' % margin, None
  spread = max(float(np.abs(a['seed'].astype(np.float64) - b['seed']).max())
               for a, b in zip(log32, log64))
  if spread > M / 8:
    return 'S = %.3g' % spread, None
  if max(len(e['offsets']) for e in log32) < 3:
    return 'no example of 3 steps', None
  refused = sum(1 for e in log32 for _, valid, _ in e['records'] if not valid)
  if not refused:
    return 'no refused move', None
  if not any(e['perm'][2] != 2 for e in log32):
    return 'no transform moves x', None
  return None, {'log': log32, 'loss32': loss32, 'loss64': loss64, 'S': spread,
                'margin': margin, 'refused': refused, 'variables': vars32}


def main():
  mods = base.install()
  geom = evaluation_ref.geometry(FOV_XYZ, FOV_XYZ, FOV_XYZ, DELTAS_XYZ, 'fixed',
                                 FOV_MOVES)
  volume = make_volume()
  volumes = {'v': volume}
  coordinates = make_coordinates(volume[1], geom)
  transforms = make_transforms()
  out = {'M': np.array(M), 'fov_xyz': np.array(FOV_XYZ),
         'deltas_xyz': np.array(DELTAS_XYZ), 'depth': np.array(DEPTH),
         'fov_moves': np.array(FOV_MOVES), 'batch': np.array(BATCH),
         'steps': np.array(STEPS), 'learning_rate': np.array(LEARNING_RATE),
         'variables_seed': np.array(VARIABLES_SEED),
         'volume_shape_seed': np.array(list(VOLUME['shape']) + [VOLUME['seed']],
                                       np.int64),
         'volume_cells_offset_scale': np.array(
             [VOLUME['cells_per_96cube'], VOLUME['offset'], VOLUME['scale']]),
         'centres': np.array([c for c, _ in coordinates], np.int32),
         'transform_perms': np.array([p for p, _ in transforms], np.int8),
         'transform_reflects': np.array([r for _, r in transforms], np.int8)}
  cases, tried, passed_over = [], 0, 0
  for rule, bias in CONFIGURATIONS:
    if len(cases) == WANTED:
      break
    tried += 1
    reason, got = try_configuration(mods, rule, bias, volumes, coordinates,
                                    transforms, geom)
    if reason is not None:
      print('%s, bias %.1f: passed over: %s' % (rule, bias, reason), flush=True)
      passed_over += 1
      continue
    case = '%s_%d' % (rule, round(bias * 10))
    cases.append(case)
    log = got['log']
    out[case + '_rule'] = np.array(rule)
    out[case + '_bias'] = np.array(bias)
    out[case + '_S'] = np.array(got['S'])
    out[case + '_margin'] = np.array(got['margin'])
    out[case + '_loss32'] = np.array(got['loss32'], np.float64)
    out[case + '_loss64'] = np.array(got['loss64'], np.float64)
    out[case + '_examples'] = np.array(
        [(e['coordinate'], e['slot']) + e['perm'] + e['reflect'] +
         (int(e['finished']),) for e in log], np.int32)
    out[case + '_offsets'] = np.array(
        [o for e in log for o in e['offsets']], np.int8).reshape(-1, 3)
    out[case + '_offsets_len'] = np.array([len(e['offsets']) for e in log],
                                          np.int32)
    out[case + '_records'] = np.array(
        [(w, v) + o for e in log for w, v, o in e['records']],
        np.int8).reshape(-1, 5)
    out[case + '_records_len'] = np.array([len(e['records']) for e in log],
                                          np.int32)
    out[case + '_seeds'] = np.stack(
        [evaluation_ref.sample_seed(e['seed']) for e in log]).astype(np.float32)
    names = sorted(got['variables'])
    out[case + '_variable_sums'] = np.array(
        [got['variables'][k].astype(np.float64).sum() for k in names])
    out[case + '_variable_samples'] = np.stack(
        [got['variables'][k].ravel()[[0, got['variables'][k].size // 2, -1]]
         for k in names]).astype(np.float32)
    print('%s: %d examples, steps %s, %d refused, S %.3g, smallest margin %.3g, '
          'largest |loss32 - loss64| %.3g' % (
              case, len(log), [len(e['offsets']) for e in log], got['refused'],
              got['S'], got['margin'],
              np.abs(out[case + '_loss32'] - out[case + '_loss64']).max()),
          flush=True)
  assert len(cases) == WANTED, cases
  assert 2 * passed_over <= tried, (passed_over, tried)
  out['cases'] = np.array(cases)
  out['variable_names'] = np.array(sorted(make_variables(0.0)))
  out['tried'] = np.array(tried)
  out['passed_over'] = np.array(passed_over)
  dst = os.path.join(GOLD, 'ref_training.npz')
  np.savez_compressed(dst, **out)
  size = os.path.getsize(dst)
  print('wrote', dst, size, 'bytes')
  assert size < MAX_BYTES, size


if __name__ == '__main__':
  main()
