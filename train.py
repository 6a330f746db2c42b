#!/usr/bin/env python3
r"""Trains a ConvStack3DFFNModel on one MI355X: the reference's train.py with
every voxel array resident on the GPU.

  python train.py --train_coords tf_record_file \
      --data_volumes validation1:grayscale.npy \
      --label_volumes validation1:groundtruth.npy \
      --model_name convstack_3d.ConvStack3DFFNModel \
      --model_args '{"depth": 12, "fov_size": [33, 33, 33], "deltas": [8, 8, 8]}' \
      --image_mean 128 --image_stddev 33 --train_dir /tmp/ffn_run

The flags it shares with the reference mean what they mean there.  Volumes are
given as evaluate_checkpoint.py takes them (`<name>:<file>.npy`,
`<name>:<file>.npz:<array>`, or `<name>:<file>:<dataset>` of an HDF5 file where
h5py is installed); coordinates come from a TFRecord file as
build_coordinates.py writes it.  The loop is the reference's: next batch ->
train step -> update_seeds, with the examples, their augmentation and the FoV
moves in ffn_amd/training/examples.py and the step in
ffn_amd/training/trainer.py.  There is no CPU fallback: without a GPU the
script raises.

Every --checkpoint_steps steps and at the end two files are written to
--train_dir:

  model.ckpt-<step>.npz        the variables under their TensorFlow names;
                               evaluate_checkpoint.py --checkpoint takes it
  model.ckpt-<step>.state.npz  the rest of ConvStackTrainer.state(): optimizer
                               slots, step counter, adam's beta powers, flags

A run resumes from the newest pair found in --train_dir (its example streams
start afresh, as the reference's do).  Summaries are appended to
<train_dir>/summaries.jsonl as JSON lines every --summary_rate_secs seconds:
step, loss, learning rate, clipped gradient entries and the tracker's eval/*
and moves/* summaries, which are then reset (train.py:422-423).  With
--section_augmentation (misalignment, missing section, out-of-focus section,
grayscale perturbation of the reference's augmentation.py, on the device:
ffn_amd/training/augmentation.py) a line also counts, since the start of the
run, the examples, those misaligned, the sections blanked and blurred, and the
examples perturbed, under augmentation/*.  A loss or a
gradient that is not finite ends the run with InvalidLossError; the last
checkpoint written stays as it is.

With --sync_sgd --replicas_to_aggregate R a step takes R batches of
--batch_size FoVs (R "replicas", each with its own example stream: coordinates
r::R of the file, seeds --seed + r), their gradients all under the same
variables, clips each, averages them in replica order and applies the mean
once (ConvStackTrainer.contribute / apply_contributions; the reference clips
before SyncReplicasOptimizer averages, model.py:142-145).  One process hosts
all R; started by torch.distributed.run, every rank hosts R / world of them
on its own GPU (--ranks_share_gpus with --collective_backend gloo: on GPU
local_rank % device_count), the ranks all-gather the raw gradients and every
rank folds them itself, so the result depends on neither the collective
library's summation order nor the number of ranks.  The seed is rank 0's;
every rank resumes from the newest pair in --train_dir; only rank 0 writes
checkpoints and summaries, whose lines then carry `replicas` and `world`, the
loss as the mean over all R, and eval/*, moves/* of rank 0's replicas; before
every checkpoint the ranks compare a checksum of their parameters and stop
if they differ.  No run on more than one GPU exists yet.

Not here: TensorFlow-format checkpoints, asynchronous replicas (--master,
--task, --ps_tasks, --replica_step_delay), backup replicas (--total_replicas
above --replicas_to_aggregate), tf.train.shuffle_batch's queue (the
coordinates are cycled, reshuffled per epoch), image summaries, the elastic,
affine, rotation and tf.image contrast augmentations.  TensorFlow's
random number streams are not reproduced: --seed makes a run of this script
reproducible.
"""

import argparse
import json
import logging
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import evaluate_checkpoint as volumes_lib  # noqa: E402  (volume, map helpers)
from ffn_amd import coordinates as coordinate_ops  # noqa: E402
from ffn_amd.training import augmentation  # noqa: E402
from ffn_amd.training import evaluation  # noqa: E402
from ffn_amd.training import examples  # noqa: E402
from ffn_amd.training import optimizer as optimizer_lib  # noqa: E402
from ffn_amd.training import replicas as replicas_lib  # noqa: E402
from ffn_amd.training.import_util import import_symbol  # noqa: E402

CHECKPOINT_RE = re.compile(r'^model\.ckpt-(\d+)\.npz$')


def _csv(text):
  return [v for v in text.split(',') if v.strip()]


def _axes(text):
  return [int(v) for v in _csv(text)]


def _boolean(text):
  if text.lower() in ('true', '1', 'yes'):
    return True
  if text.lower() in ('false', '0', 'no'):
    return False
  raise argparse.ArgumentTypeError('expected true or false, got %r' % text)


def job_environment(environ=None):
  """(rank, world, local rank, launched) from the environment that
  torch.distributed.run gives its workers; (0, 1, 0, False) outside one."""
  environ = os.environ if environ is None else environ
  if 'RANK' not in environ or 'WORLD_SIZE' not in environ:
    return 0, 1, 0, False
  rank, world = int(environ['RANK']), int(environ['WORLD_SIZE'])
  return rank, world, int(environ.get('LOCAL_RANK', rank)), True


def parse_args(argv=None):
  ap = argparse.ArgumentParser(
      description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  # training data (train.py:50-72)
  ap.add_argument('--train_coords', required=True,
                  help='TFRecord file of coordinates (GZIP or plain)')
  ap.add_argument('--data_volumes', required=True, type=_csv,
                  help='comma-separated image volumes, <name>:<file>...')
  ap.add_argument('--label_volumes', required=True, type=_csv,
                  help='comma-separated label volumes under the same names')
  ap.add_argument('--model_name', required=True)
  ap.add_argument('--model_args', required=True, type=json.loads,
                  help='JSON arguments of the model class')
  # training infra (train.py:75-88)
  ap.add_argument('--train_dir', default='/tmp')
  ap.add_argument('--batch_size', type=int, default=4)
  ap.add_argument('--max_steps', type=int, default=10000)
  ap.add_argument('--summary_rate_secs', type=int, default=120)
  # FFN training options (train.py:91-130)
  ap.add_argument('--seed_pad', type=float, default=0.05)
  ap.add_argument('--threshold', type=float, default=0.9)
  ap.add_argument('--fov_policy', default='fixed',
                  choices=examples.TRAIN_POLICIES)
  ap.add_argument('--fov_moves', type=int, default=1)
  ap.add_argument('--shuffle_moves', type=_boolean, nargs='?', const=True,
                  default=True)
  ap.add_argument('--image_mean', type=float, default=None)
  ap.add_argument('--image_stddev', type=float, default=None)
  ap.add_argument('--image_offset_scale_map', type=_csv, default=None)
  ap.add_argument('--permutable_axes', type=_axes, default=[1, 2],
                  help='subset of 0,1,2: the z, y, x axes that may change '
                  'places')
  ap.add_argument('--reflectable_axes', type=_axes, default=[0, 1, 2],
                  help='subset of 0,1,2: the z, y, x axes that may be reversed')
  ap.add_argument('--section_augmentation', type=json.loads, default=None,
                  help='JSON arguments of the section augmentations under the '
                  "reference's names (misalignment_skip_ratio, max_xy_offset, "
                  'slip_vs_translate_ratio, missing_section_skip_ratio, '
                  'max_missing_section_indices_ratio, outoffocus_skip_ratio, '
                  'max_outoffocus_indices_ratio, max_filter_stdev, '
                  'grayscale_skip_ratio, max_contrast_factor, '
                  'max_brightness_factor); an augmentation whose keys are '
                  'absent is off; default: none of them')
  # the optimizer's flags (ffn/training/optimizer.py)
  defaults = optimizer_lib.OptimizerConfig()
  ap.add_argument('--optimizer', default=defaults.optimizer,
                  choices=optimizer_lib.RULES)
  for name in optimizer_lib.OptimizerConfig.FIELDS[1:]:
    kind = int if name == 'decay_steps' else float
    ap.add_argument('--' + name, type=kind, default=getattr(defaults, name))
  # this script's own
  ap.add_argument('--seed', type=int, default=None,
                  help='seeds the initial weights, the order of moves and '
                  'coordinates, and the augmentation (default: the clock, as '
                  'train.py:437)')
  ap.add_argument('--checkpoint_steps', type=int, default=1000)
  ap.add_argument('--device', type=int, default=0)
  # synchronous replicas (ffn/training/optimizer.py:58-70)
  ap.add_argument('--sync_sgd', type=_boolean, nargs='?', const=True,
                  default=False,
                  help='every step averages the clipped gradients of '
                  '--replicas_to_aggregate batches of --batch_size FoVs, all '
                  'taken under the same variables, and applies them once')
  ap.add_argument('--replicas_to_aggregate', type=int, default=None,
                  help='R, the replicas of a step over all ranks of the job; '
                  'a multiple of the number of ranks')
  ap.add_argument('--total_replicas', type=int, default=None,
                  help='accepted only where it equals --replicas_to_aggregate')
  ap.add_argument('--collective_backend', choices=('nccl', 'gloo'),
                  default='nccl',
                  help='torch.distributed backend of a job started by '
                  'torch.distributed.run: nccl exchanges device arrays, gloo '
                  'host arrays')
  ap.add_argument('--ranks_share_gpus', action='store_true',
                  help='rank k runs on GPU local_rank %% device_count instead '
                  'of needing a GPU of its own (needs --collective_backend '
                  'gloo)')
  args = ap.parse_args(argv)
  world = job_environment()[1]
  if args.sync_sgd:
    if args.replicas_to_aggregate is None:
      ap.error('--sync_sgd needs --replicas_to_aggregate')
    try:
      replicas_lib.per_rank(args.replicas_to_aggregate, world)
    except ValueError as e:
      ap.error('--replicas_to_aggregate: %s' % e)
    if (args.total_replicas is not None and
        args.total_replicas != args.replicas_to_aggregate):
      ap.error('--total_replicas %d differs from --replicas_to_aggregate %d: '
               'backup replicas are not mirrored' %
               (args.total_replicas, args.replicas_to_aggregate))
    if args.ranks_share_gpus and args.collective_backend == 'nccl':
      ap.error('--ranks_share_gpus needs --collective_backend gloo: nccl '
               'cannot run two ranks on one GPU')
  elif world > 1:
    ap.error('a job of %d ranks needs --sync_sgd' % world)
  if ((args.image_stddev is None or args.image_mean is None) and
      not args.image_offset_scale_map):
    ap.error('--image_mean, --image_stddev or --image_offset_scale_map need to '
             'be defined')
  if not 1 <= args.batch_size <= evaluation.MAX_SLOTS:
    ap.error('--batch_size must be in [1, %d]' % evaluation.MAX_SLOTS)
  if args.checkpoint_steps < 1:
    ap.error('--checkpoint_steps must be at least 1')
  if args.section_augmentation is not None:
    if not isinstance(args.section_augmentation, dict):
      ap.error('--section_augmentation takes a JSON object')
    try:
      augmentation.SectionAugmentations(args.section_augmentation, 0)
    except (TypeError, ValueError) as e:
      ap.error('--section_augmentation: %s' % e)
  return args


def optimizer_config(args):
  return optimizer_lib.OptimizerConfig(
      **{k: getattr(args, k) for k in optimizer_lib.OptimizerConfig.FIELDS})


# ---- checkpoints -------------------------------------------------------------------


def checkpoint_paths(train_dir, step):
  prefix = os.path.join(train_dir, 'model.ckpt-%d' % step)
  return prefix + '.npz', prefix + '.state.npz'


def _savez(path, arrays):
  tmp = path + '.tmp'
  with open(tmp, 'wb') as f:
    np.savez(f, **arrays)
  os.replace(tmp, path)


def save_checkpoint(train_dir, state):
  """Writes the pair of files of a ConvStackTrainer.state(); returns their
  paths.  The state file goes first: a pair is complete once the variables
  exist."""
  os.makedirs(train_dir, exist_ok=True)
  variables_path, state_path = checkpoint_paths(train_dir,
                                                int(state['global_step']))
  rest = {'global_step': np.int64(state['global_step']),
          'beta1_power': np.float32(state['beta1_power']),
          'beta2_power': np.float32(state['beta2_power']),
          'config': np.array(json.dumps(state['config'], sort_keys=True)),
          'num_slots': np.int64(len(state['slots']))}
  for k, slot in enumerate(state['slots']):
    for name, value in slot.items():
      rest['slot%d/%s' % (k, name)] = np.asarray(value, np.float32)
  _savez(state_path, rest)
  _savez(variables_path, {k: np.asarray(v, np.float32)
                          for k, v in state['variables'].items()})
  return variables_path, state_path


def load_checkpoint(variables_path, state_path):
  """-> a state as ConvStackTrainer.load_state takes it."""
  with np.load(variables_path) as d:
    variables = {k: d[k] for k in d.files}
  with np.load(state_path) as d:
    slots = [{} for _ in range(int(d['num_slots']))]
    for key in d.files:
      if key.startswith('slot'):
        k, name = key.split('/', 1)
        slots[int(k[4:])][name] = d[key]
    return {'variables': variables, 'slots': slots,
            'global_step': int(d['global_step']),
            'beta1_power': np.float32(d['beta1_power']),
            'beta2_power': np.float32(d['beta2_power']),
            'config': json.loads(str(d['config']))}


def newest_checkpoint(train_dir):
  """(step, variables path, state path) of the complete pair with the largest
  step in train_dir, or None."""
  if not os.path.isdir(train_dir):
    return None
  best = None
  for name in os.listdir(train_dir):
    m = CHECKPOINT_RE.match(name)
    if not m:
      continue
    step = int(m.group(1))
    paths = checkpoint_paths(train_dir, step)
    if os.path.exists(paths[1]) and (best is None or step > best[0]):
      best = (step,) + paths
  return best


# ---- the run -----------------------------------------------------------------------


def load_volumes(args):
  """-> {name: (image, labels, offset, scale)}."""
  images = dict(volumes_lib.load_volume(spec) for spec in args.data_volumes)
  labels = dict(volumes_lib.load_volume(spec) for spec in args.label_volumes)
  if set(images) != set(labels):
    raise ValueError('image volumes %r and label volumes %r differ' %
                     (sorted(images), sorted(labels)))
  scales = volumes_lib.offset_scale_map(args.image_offset_scale_map)
  out = {}
  for name in sorted(images):
    offset, scale = scales.get(name, (args.image_mean, args.image_stddev))
    if offset is None or scale is None:
      raise ValueError('no offset and scale for volume %r' % name)
    out[name] = (images[name], labels[name], offset, scale)
  return out


def make_trainer(model, config, args):
  """The device half: raises without a GPU (there is no other path)."""
  from ffn_amd.training import trainer as trainer_lib  # pylint:disable=g-import-not-at-top
  return trainer_lib.ConvStackTrainer(model, config, max_batch=args.batch_size,
                                      device_id=args.device)


def write_summary(f, trainer, batches, seconds):
  stats = trainer.last_stats or {}
  line = {'step': int(trainer.global_step), 'loss': stats.get('loss'),
          'learning_rate': stats.get('learning_rate'),
          'clipped': stats.get('clipped'), 'seconds': seconds,
          'examples_finished': batches.examples_finished,
          'epochs': batches.epochs}
  line.update(batches.result.summaries())
  if batches.sections is not None:
    line.update({'augmentation/' + k: int(v)
                 for k, v in batches.section_counts.items()})
  batches.reset_result()
  f.write(json.dumps({k: (float(v) if isinstance(v, np.floating) else v)
                      for k, v in line.items()}, sort_keys=True) + '\n')
  f.flush()


def replica_batches(args, model, volumes, coordinates, seed, replica, ops,
                    device, result):
  """The example stream of global replica `replica` of
  args.replicas_to_aggregate: its shard of the coordinates and its own random
  streams (replicas.shard, replicas.stream_seeds), so it is the same stream
  whichever rank hosts it."""
  seeds = replicas_lib.stream_seeds(seed, replica)
  transform = augmentation.PermuteAndReflect(
      args.permutable_axes, args.reflectable_axes,
      np.random.default_rng(seeds['transform_seed']))
  sections = None
  if args.section_augmentation is not None:
    sections = augmentation.SectionAugmentations(
        args.section_augmentation,
        np.random.RandomState(seeds['sections_seed'] % (1 << 32)))
  geometry = evaluation.Geometry.from_info(model.info, args.fov_policy,
                                           args.fov_moves, args.batch_size)
  return examples.BatchExampleIter(
      model.info, ops, volumes,
      replicas_lib.shard(coordinates, replica, args.replicas_to_aggregate),
      fov_policy=args.fov_policy, fov_moves=args.fov_moves,
      batch_size=args.batch_size, threshold=args.threshold,
      seed_pad=args.seed_pad, shifts=model.shifts,
      shuffle_moves=args.shuffle_moves, moves_seed=seeds['moves_seed'],
      transform=transform, shuffle_seed=seeds['shuffle_seed'],
      sections=sections, io=examples.torch_io(geometry, args.batch_size, device),
      result=result)


def write_sync_summary(f, trainer, streams, seconds, world):
  """A summary line of a --sync_sgd run: the loss is the mean over all
  replicas of the last step; eval/*, moves/* and the counts are those of this
  rank's replicas (rank 0 writes)."""
  stats = trainer.last_stats or {}
  line = {'step': int(trainer.global_step), 'loss': stats.get('loss'),
          'learning_rate': stats.get('learning_rate'),
          'clipped': stats.get('clipped'), 'seconds': seconds,
          'replicas': stats.get('replicas'), 'world': world,
          'examples_finished': sum(b.examples_finished for b in streams),
          'epochs': max(b.epochs for b in streams)}
  line.update(streams[0].result.summaries())
  if streams[0].sections is not None:
    for key in streams[0].section_counts:
      line['augmentation/' + key] = int(sum(b.section_counts[key]
                                            for b in streams))
  fresh = evaluation.EvalResult(streams[0].shifts)
  for b in streams:
    b.reset_result(fresh)
  f.write(json.dumps({k: (float(v) if isinstance(v, np.floating) else v)
                      for k, v in line.items()}, sort_keys=True) + '\n')
  f.flush()


def main_sync(args):
  """The --sync_sgd run: this process is one rank of the job (the only one
  outside torch.distributed.run) and hosts R / world replicas."""
  import torch  # pylint:disable=g-import-not-at-top
  from ffn_amd.training import trainer as trainer_lib  # pylint:disable=g-import-not-at-top
  rank, world, local_rank, launched = job_environment()
  per_rank = replicas_lib.per_rank(args.replicas_to_aggregate, world)
  device_id = args.device
  if launched:
    device_id = (local_rank % max(torch.cuda.device_count(), 1)
                 if args.ranks_share_gpus else local_rank)
  group = None
  if launched:
    import torch.distributed as dist  # pylint:disable=g-import-not-at-top
    if args.collective_backend == 'nccl':
      dist.init_process_group('nccl',
                              device_id=torch.device('cuda', device_id))
    else:
      dist.init_process_group('gloo')
  trainer, replica_ops = None, []
  try:
    if launched:
      group = replicas_lib.ReplicaGroup(torch.device('cuda', device_id))
    seed = int(time.time()) if args.seed is None else args.seed
    if group is not None:
      seed = group.rank0_value(seed)
    logging.info('Random seed: %r (rank %d of %d, %d replicas here, GPU %d)',
                 seed, rank, world, per_rank, device_id)
    volumes = load_volumes(args)
    centres, names = coordinate_ops.read_tfrecord(args.train_coords)
    coordinates = list(zip(centres.tolist(), names))
    model = import_symbol(args.model_name)(batch_size=args.batch_size,
                                           **args.model_args)
    config = optimizer_config(args)
    resume = newest_checkpoint(args.train_dir)
    if resume is None:
      model.init_random(seed=seed % (1 << 32))
    else:
      model.load_checkpoint(resume[1])
    trainer = trainer_lib.ConvStackTrainer(
        model, config, max_batch=args.batch_size, device_id=device_id,
        replicas=per_rank, group=group)
    if resume is not None:
      trainer.load_state(load_checkpoint(resume[1], resume[2]))
      logging.info('Resumed from %s at step %d', resume[1],
                   trainer.global_step)
    trainer.check_ranks_agree()  # same start, whatever each rank found on disk
    result, streams = None, []
    for k in range(per_rank):
      ops = evaluation.EvaluationOps(device_id)
      replica_ops.append(ops)
      batches = replica_batches(
          args, model, volumes, coordinates, seed,
          replicas_lib.global_index(rank, k, per_rank), ops, trainer.device,
          result)
      result = batches.result
      streams.append(batches)
      if batches.skipped:
        logging.info('replica %d: %d coordinates skipped (patch leaves the '
                     'volume)', replicas_lib.global_index(rank, k, per_rank),
                     batches.skipped)
    chief = rank == 0
    if chief:
      os.makedirs(args.train_dir, exist_ok=True)
    saved = trainer.global_step if resume is not None else None

    def checkpoint():
      trainer.check_ranks_agree()
      logging.info('rank %d: ranks agree at step %d', rank,
                   trainer.global_step)
      if chief:
        save_checkpoint(args.train_dir, trainer.state())

    t_begin = t_last = time.time()
    summ = (open(os.path.join(args.train_dir, 'summaries.jsonl'), 'a')
            if chief else None)
    try:
      while trainer.global_step < args.max_steps:
        for k, batches in enumerate(streams):
          seed_io, image, labels, weights = batches.next()
          _, logits = trainer.contribute(k, seed_io, image, labels, weights)
          batches.update_seeds(logits)
        step = trainer.apply_contributions()
        now = time.time()
        if chief and now - t_last > args.summary_rate_secs:
          write_sync_summary(summ, trainer, streams, now - t_begin, world)
          t_last = now
        if step % args.checkpoint_steps == 0:
          checkpoint()
          saved = step
      if saved != trainer.global_step:
        checkpoint()
      if chief:
        write_sync_summary(summ, trainer, streams, time.time() - t_begin,
                           world)
    finally:
      if summ is not None:
        summ.close()
    logging.info('Done at step %d', trainer.global_step)
    return trainer.global_step
  finally:
    if trainer is not None:
      trainer.close()
    for ops in replica_ops:
      ops.close()
    if launched:
      import torch.distributed as dist  # pylint:disable=g-import-not-at-top
      dist.destroy_process_group()


def main(argv=None):
  args = parse_args(argv)
  logging.basicConfig(level=logging.INFO)
  if args.sync_sgd:
    return main_sync(args)
  seed = int(time.time()) if args.seed is None else args.seed
  logging.info('Random seed: %r', seed)
  volumes = load_volumes(args)
  centres, names = coordinate_ops.read_tfrecord(args.train_coords)
  model = import_symbol(args.model_name)(batch_size=args.batch_size,
                                         **args.model_args)
  config = optimizer_config(args)
  resume = newest_checkpoint(args.train_dir)
  if resume is None:
    model.init_random(seed=seed % (1 << 32))
  else:
    model.load_checkpoint(resume[1])
  trainer = make_trainer(model, config, args)
  try:
    if resume is not None:
      trainer.load_state(load_checkpoint(resume[1], resume[2]))
      logging.info('Resumed from %s at step %d', resume[1],
                   trainer.global_step)
    transform = augmentation.PermuteAndReflect(
        args.permutable_axes, args.reflectable_axes,
        np.random.default_rng(seed))
    sections = None
    if args.section_augmentation is not None:
      sections = augmentation.SectionAugmentations(
          args.section_augmentation, np.random.RandomState(seed % (1 << 32)))
    ops = evaluation.default_ops(args.device)
    geometry = evaluation.Geometry.from_info(model.info, args.fov_policy,
                                             args.fov_moves, args.batch_size)
    batches = examples.BatchExampleIter(
        model.info, ops, volumes, zip(centres.tolist(), names),
        fov_policy=args.fov_policy, fov_moves=args.fov_moves,
        batch_size=args.batch_size, threshold=args.threshold,
        seed_pad=args.seed_pad, shifts=model.shifts,
        shuffle_moves=args.shuffle_moves, moves_seed=seed, transform=transform,
        shuffle_seed=seed, sections=sections,
        io=examples.torch_io(geometry, args.batch_size, trainer.device))
    if batches.skipped:
      logging.info('%d coordinates skipped (patch leaves the volume)',
                   batches.skipped)
    os.makedirs(args.train_dir, exist_ok=True)
    saved = trainer.global_step if resume is not None else None
    t_begin = t_last = time.time()
    with open(os.path.join(args.train_dir, 'summaries.jsonl'), 'a') as summ:
      while trainer.global_step < args.max_steps:
        seed_io, image, labels, weights = batches.next()
        _, logits, step = trainer.train_step_device(seed_io, image, labels,
                                                    weights)
        batches.update_seeds(logits)
        now = time.time()
        if now - t_last > args.summary_rate_secs:
          write_summary(summ, trainer, batches, now - t_begin)
          t_last = now
        if step % args.checkpoint_steps == 0:
          save_checkpoint(args.train_dir, trainer.state())
          saved = step
      if saved != trainer.global_step:
        save_checkpoint(args.train_dir, trainer.state())
      write_summary(summ, trainer, batches, time.time() - t_begin)
    logging.info('Done at step %d', trainer.global_step)
    return trainer.global_step
  finally:
    trainer.close()


if __name__ == '__main__':
  main()
