"""Synchronous replicas on the GPU: ffn_optimizer_aggregate against the numpy
fold (tests/replicas_ref.py), ConvStackTrainer.contribute /
apply_contributions against the optimizer oracle, and train.py --sync_sgd in
one process, as two ranks on one GPU (gloo) and once over the nccl backend.

Every comparison is of bits: the feature adds no arithmetic whose error needs
a tolerance.  Whether a replica's gradient is right is
tests/test_gpu_gradients.py's business.
"""
import ctypes
import importlib.util
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from tests import gradients_ref as gref
from tests import optimizer_ref as ref
from tests import replicas_ref as rref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
GUARD = 64
F32 = np.float32
DEPTH12_TOTAL = 638436  # arena_layout(12).total: 638433 variables + pads
COUNTS = [1, 3, 4, 5, 1023, 4097, DEPTH12_TOTAL]
NS = [1, 2, 3, 8]
PLANTED = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-41, -1e-41, 3e-39,
                    0.7, -0.7, 0.70000005, -0.70000005, 5.0, -5.0], np.float32)
ZYX = (9, 9, 9)


@pytest.fixture(scope='module')
def torch():
  import torch as torch_module
  return torch_module


@pytest.fixture(scope='module')
def opt():
  from ffn_amd.training import optimizer
  return optimizer


@pytest.fixture(scope='module')
def tr():
  from ffn_amd.training import trainer
  return trainer


@pytest.fixture(scope='module')
def ops(opt):
  return opt.default_ops(0)


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
  return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def guarded(torch, values, fill=np.nan):
  host = np.full(len(values) + GUARD, fill, np.float32)
  host[:len(values)] = values
  t = torch.from_numpy(host).to('cuda:0')
  torch.cuda.synchronize()
  assert t.data_ptr() % 16 == 0
  return t


# -- 1. aggregate -------------------------------------------------------------
def aggregate_inputs(count, n, stride, seed):
  """n rows ~ N(0, 0.5) (one entry in six beyond the clip) `stride` apart, the
  gaps filled with 77 (never read).  The planted values rotate through the
  rows at the front and, from the back, in the tail elements; where there is
  room, one element holds the triple whose sum depends on the order and one
  its small twin inside the clip (rows past the third hold 0 there)."""
  rng = np.random.RandomState(seed)
  src = np.full(n * stride, 77.0, np.float32)
  rows = [src[r * stride:r * stride + count] for r in range(n)]
  for r, row in enumerate(rows):
    row[:] = rng.normal(0, 0.5, count).astype(np.float32)
    planted = np.roll(PLANTED, 3 * r)
    m = min(count, len(planted))
    row[:m] = planted[:m]
    if count > 2 * len(planted):
      row[-len(planted):] = planted[::-1]
  if count > 64:
    for at, triple in ((40, rref.ORDER_TRIPLE), (count // 2,
                                                 rref.ORDER_TRIPLE_SMALL)):
      for r, row in enumerate(rows):
        row[at] = triple[r] if r < 3 else 0.0
  return src


def run_aggregate(ops, torch, count, n, stride, clip, src):
  sd = guarded(torch, src)
  dd = guarded(torch, np.full(count, -9.0, np.float32), fill=-9.0)
  ops.aggregate(count, n, sd, stride, clip, dd)
  got = dd.cpu().numpy()
  assert np.all(got[count:] == -9.0)  # nothing behind the last element
  back = sd.cpu().numpy()
  assert same_bits(back[:len(src)], src) and np.all(np.isnan(back[len(src):]))
  return got[:count]


@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('count', COUNTS)
def test_aggregate_equals_the_fold_bit_for_bit(ops, torch, count, n):
  stride = -(-count // 4) * 4
  src = aggregate_inputs(count, n, stride, seed=count + n)
  for clip in (0.7, 0.0):
    want = rref.fold_strided(src, count, n, stride, clip)
    got = run_aggregate(ops, torch, count, n, stride, clip, src)
    differ = np.flatnonzero(bits(got) != bits(want))
    assert differ.size == 0, (clip, differ[:8], got[differ[:8]],
                              want[differ[:8]])
    assert same_bits(run_aggregate(ops, torch, count, n, stride, clip, src),
                     got)
  if count > 64 and n >= 3:
    # the planted triples (clip 0 ran last): 0 in replica order only
    assert got[40] == 0 and got[count // 2] == 0
  assert ops.last_timing_aggregate() > 0


def test_aggregate_with_a_larger_stride(ops, torch):
  count, n, stride = 4097, 3, 4100 + 24
  src = aggregate_inputs(count, n, stride, seed=5)
  for clip in (0.7, 0.0):
    want = rref.fold_strided(src, count, n, stride, clip)
    assert same_bits(run_aggregate(ops, torch, count, n, stride, clip, src),
                     want)
  # the order is the rows': reversed rows give other bits
  rev = np.concatenate([src[r * stride:(r + 1) * stride]
                        for r in reversed(range(n))])
  assert not same_bits(rref.fold_strided(rev, count, n, stride, 0.0), want)
  assert same_bits(run_aggregate(ops, torch, count, n, stride, 0.0, rev),
                   rref.fold_strided(rev, count, n, stride, 0.0))


def test_aggregate_of_one_keeps_the_clipped_bits(ops, torch):
  row = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1e-41, -1e-41, 0.9,
                  -0.9], np.float32)
  want = np.array([-0.0, 0.0, np.nan, 0.7, -0.7, 1e-41, -1e-41, 0.7, -0.7],
                  np.float32)
  src = np.zeros(12, np.float32)
  src[:9] = row
  assert same_bits(run_aggregate(ops, torch, 9, 1, 12, 0.7, src), want)
  assert same_bits(run_aggregate(ops, torch, 9, 1, 12, 0.0, src), row)


def test_aggregate_refuses_bad_arguments_and_writes_nothing(ops, torch):
  count, n, stride = 64, 3, 64
  src = torch.full((n * stride + 8,), 1.0, dtype=torch.float32,
                   device='cuda:0')
  dst = torch.full((count + 8,), -9.0, dtype=torch.float32, device='cuda:0')
  torch.cuda.synchronize()
  lib, h = ops._lib, ops._h
  P = lambda t, off=0: ctypes.c_void_p(0 if t is None else t.data_ptr() + off)

  def call(handle=h, count=count, n=n, s=P(src), stride=stride, clip=0.7,
           d=P(dst)):
    return lib.ffn_optimizer_aggregate(handle, count, n, s, stride, clip, d)

  assert call(handle=None) == ERR_ARG
  assert call(n=0) == ERR_ARG
  assert call(n=-1) == ERR_ARG
  assert call(n=257) == ERR_ARG
  assert call(count=0) == ERR_ARG
  assert call(count=2 ** 31) == ERR_ARG
  assert call(s=P(None)) == ERR_ARG
  assert call(d=P(None)) == ERR_ARG
  assert call(stride=66) == ERR_ARG          # not a multiple of 4
  assert call(count=63, stride=62) == ERR_ARG
  assert call(stride=60) == ERR_ARG          # below count
  assert call(clip=float('nan')) == ERR_ARG
  assert call(s=P(src, 4)) == ERR_ARG        # alignment
  assert call(d=P(dst, 4)) == ERR_ARG
  assert call(d=P(src)) == ERR_ARG           # dst on the first row
  assert call(d=P(src, 4 * (2 * stride + 32))) == ERR_ARG  # in the last row
  assert call(n=2, count=32, d=P(src, 4 * 40)) == ERR_ARG  # between the rows
  assert lib.ffn_last_error()
  torch.cuda.synchronize()
  assert np.all(dst.cpu().numpy() == -9.0)
  assert np.all(src.cpu().numpy() == 1.0)
  # dst right behind the rows that are read is no overlap; the handle works
  assert call(n=2, d=P(src, 4 * 2 * stride)) == 0
  got = src.cpu().numpy()
  assert np.all(got[2 * stride:3 * stride] == 0.7) and np.all(got[3 * stride:]
                                                             == 1.0)


# -- 2. the trainer -----------------------------------------------------------
def make_model(variables, depth, zyx=ZYX):
  from ffn_amd.training.models import convstack_3d
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(zyx[::-1]),
                                       deltas=[1, 1, 1], depth=depth)
  m.set_variables(variables)
  return m


def assert_same_dict(got, want, what):
  assert sorted(got) == sorted(want), what
  for k in want:
    assert same_bits(got[k], want[k]), (what, k)


def assert_same_state(got, want):
  assert_same_dict(got['variables'], want['variables'], 'variables')
  assert len(got['slots']) == len(want['slots'])
  for j, (a, b) in enumerate(zip(got['slots'], want['slots'])):
    assert_same_dict(a, b, 'slot %d' % j)
  assert got['global_step'] == want['global_step']
  for key in ('beta1_power', 'beta2_power'):
    assert np.float32(got[key]).tobytes() == np.float32(want[key]).tobytes()
  assert got['config'] == want['config']


@pytest.fixture(scope='module')
def batches():
  """Three batches of two FoVs, shared and never written."""
  return [gref.training_inputs(2, ZYX, seed=s) for s in (33, 34, 35)]


@pytest.mark.parametrize('rule', ref.RULES)
def test_one_replica_is_the_plain_step(opt, tr, batches, rule):
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  cfg = opt.OptimizerConfig(optimizer=rule, decay_steps=1,
                            learning_rate_decay_factor=0.5)
  plain = tr.ConvStackTrainer(make_model(variables, 3), cfg, max_batch=2)
  one = None
  try:
    one = tr.ConvStackTrainer(make_model(variables, 3), cfg, max_batch=2,
                              replicas=1)
    for k in range(2):
      want_loss, want_logits, want_step = plain.train_step(*batches[k])
      loss, logits = one.contribute(0, *batches[k])
      assert np.float32(loss).tobytes() == np.float32(want_loss).tobytes()
      assert same_bits(logits.cpu().numpy(), want_logits)
      assert one.global_step == k  # nothing applied yet
      assert one.apply_contributions() == want_step == k + 1
      assert_same_state(one.state(), plain.state())
      assert one.last_stats == dict(plain.last_stats, replicas=1)
  finally:
    plain.close()
    if one is not None:
      one.close()


def test_two_replicas_fold_in_order_under_the_same_variables(opt, tr, batches):
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  cfg = opt.OptimizerConfig(optimizer='adam', learning_rate=0.01)
  # weights that push gradient entries beyond the clip
  first = batches[0][:3] + (batches[0][3] * np.float32(300),)
  second = batches[1]
  trainer = tr.ConvStackTrainer(make_model(variables, 3), cfg, max_batch=2,
                                replicas=2)
  twin = None
  try:
    twin = tr.ConvStackTrainer(make_model(variables, 3), cfg, max_batch=2)
    flags = dict(cfg.to_dict(), max_gradient_entry_mag=0)
    oracle = ref.Optimizer(np.float32, **flags)
    before = trainer.variables()
    for step in range(2):
      loss0, _ = trainer.contribute(0, *first)
      g0 = trainer.gradients()
      loss1, _ = trainer.contribute(1, *second)
      g1 = trainer.gradients()
      # both under the variables before the update: the twin's are those
      twin.load_state(dict(trainer.state()))
      want0, _ = twin.csg.loss_and_gradients_device(*first)
      want1, _ = twin.csg.loss_and_gradients_device(*second)
      assert np.float32(loss0).tobytes() == np.float32(want0).tobytes()
      assert np.float32(loss1).tobytes() == np.float32(want1).tobytes()
      assert_same_dict(trainer.variables(), before, 'untouched by contribute')
      assert trainer.apply_contributions() == step + 1
      folded = {k: rref.fold([g0[k], g1[k]], 0.7) for k in g0}
      assert_same_dict(trainer.gradients(), folded, 'aggregated gradient')
      want = oracle.step(before, folded)
      after = trainer.variables()
      assert_same_dict(after, want, 'variables after step %d' % step)
      for j, got_slot in enumerate(trainer.slot_variables()):
        assert_same_dict(got_slot, {key: s[j] for key, s in
                                    oracle.slots.items()}, 'slot %d' % j)
      assert np.float32(trainer.beta1_power) == oracle.b1p
      assert np.float32(trainer.beta2_power) == oracle.b2p
      stats = trainer.last_stats
      assert stats['replicas'] == 2
      assert stats['loss'] == (float(loss0) + float(loss1)) / 2
      clipped = [sum(int(np.sum(np.abs(g) > np.float32(0.7)))
                     for g in gs.values()) for gs in (g0, g1)]
      assert stats['clipped'] == sum(clipped) and clipped[0] > 0
      assert stats['max_abs'] == max(float(np.max(np.abs(g)))
                                     for gs in (g0, g1) for g in gs.values())
      # the clip was each replica's: the mean of the raw gradients is another
      raw = {k: rref.fold([g0[k], g1[k]], 0.0) for k in g0}
      assert any(not same_bits(raw[k], folded[k]) for k in raw)
      assert any(not same_bits(after[k], before[k]) for k in after)
      before = after
  finally:
    trainer.close()
    if twin is not None:
      twin.close()


def test_a_replica_that_is_not_finite_voids_the_step(opt, tr, batches):
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  cfg = opt.OptimizerConfig(optimizer='adam')
  trainer = tr.ConvStackTrainer(make_model(variables, 3), cfg, max_batch=2,
                                replicas=2)
  try:
    trainer.contribute(0, *batches[0])
    trainer.contribute(1, *batches[1])
    trainer.apply_contributions()  # slots and powers away from their start
    held = trainer.state()
    poisoned = batches[2][3].copy()
    poisoned[1, 4, 4, 4] = np.nan
    trainer.contribute(0, *batches[0])
    trainer.contribute(1, *(batches[2][:3] + (poisoned,)))
    with pytest.raises(tr.InvalidLossError, match='Invalid loss detected'):
      trainer.apply_contributions()
    assert_same_state(trainer.state(), held)
    # the contributions are dropped
    with pytest.raises(RuntimeError, match='not contributed'):
      trainer.apply_contributions()
    assert_same_state(trainer.state(), held)
    trainer.contribute(0, *batches[0])
    trainer.contribute(1, *batches[2])
    assert trainer.apply_contributions() == 2
    assert np.isfinite(trainer.last_stats['loss'])
  finally:
    trainer.close()


def test_a_missing_replica_is_an_error_that_changes_nothing(opt, tr, batches):
  variables = gref.random_variables(2, seed=22, stddev=0.05)
  trainer = tr.ConvStackTrainer(make_model(variables, 2),
                                opt.OptimizerConfig(optimizer='momentum'),
                                max_batch=2, replicas=2)
  plain = None
  try:
    held = trainer.state()
    with pytest.raises(RuntimeError, match='not contributed'):
      trainer.apply_contributions()
    trainer.contribute(1, *batches[1])
    with pytest.raises(RuntimeError, match=r'\[0\]'):
      trainer.apply_contributions()
    assert_same_state(trainer.state(), held)
    with pytest.raises(ValueError):
      trainer.contribute(2, *batches[0])
    # the contribution held is still good
    trainer.contribute(0, *batches[0])
    assert trainer.apply_contributions() == 1
    # and a trainer without replicas has no contributions to apply
    plain = tr.ConvStackTrainer(make_model(variables, 2), max_batch=2)
    with pytest.raises(RuntimeError):
      plain.apply_contributions()
    with pytest.raises(ValueError):
      tr.ConvStackTrainer(make_model(variables, 2), max_batch=2, replicas=257)
  finally:
    trainer.close()
    if plain is not None:
      plain.close()


# -- 3. train.py --------------------------------------------------------------
def script(name):
  spec = importlib.util.spec_from_file_location(
      name + '_script', os.path.join(ROOT, name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.fixture(scope='module')
def run_args(tmp_path_factory):
  """The flags of a small run (FoV 33^3, depth 2, batch 1) without
  --train_dir, --max_steps and the replica flags."""
  from ffn_amd import synthetic
  tmp = tmp_path_factory.mktemp('replicas_data')
  shape = (64, 64, 64)
  image = synthetic.cells_volume(shape, seed=12, cells_per_96cube=40.0)
  labels = synthetic.cells_labels(shape, seed=12, cells_per_96cube=40.0)
  np.save(tmp / 'image.npy', image)
  np.save(tmp / 'labels.npy', labels)
  partitions = np.where(labels > 0, 1, 0).astype(np.uint8)
  partitions[:30] = partitions[34:] = 255  # a thin slab: a small file
  coords = str(tmp / 'coords')
  script('build_coordinates').build_coordinates(
      [('a', partitions)], (24, 24, 24), coords, seed=5)
  model_args = '{"depth": 2, "fov_size": [33, 33, 33], "deltas": [8, 8, 8]}'
  return ['--train_coords', coords,
          '--data_volumes', 'a:%s' % (tmp / 'image.npy'),
          '--label_volumes', 'a:%s' % (tmp / 'labels.npy'),
          '--model_name', 'convstack_3d.ConvStack3DFFNModel',
          '--model_args', model_args, '--image_mean', '128',
          '--image_stddev', '33', '--batch_size', '1', '--seed', '7',
          '--optimizer', 'momentum', '--learning_rate', '0.01', '--sync_sgd']


def read_pair(train, train_dir, step):
  """Every array of the checkpoint pair of `step`, by file and name."""
  out = {}
  for path in train.checkpoint_paths(str(train_dir), step):
    with np.load(path) as d:
      for key in d.files:
        out[os.path.basename(path) + ':' + key] = d[key]
  return out


def assert_same_pair(got, want):
  assert sorted(got) == sorted(want)
  for key, value in want.items():
    assert got[key].dtype == value.dtype and got[key].shape == value.shape, key
    assert got[key].tobytes() == value.tobytes(), key


def test_train_script_with_two_replicas_writes_and_resumes(run_args, tmp_path):
  train = script('train')
  train_dir = tmp_path / 'run'
  argv = run_args + ['--replicas_to_aggregate', '2', '--train_dir',
                     str(train_dir), '--checkpoint_steps', '4']
  assert train.main(argv + ['--max_steps', '6']) == 6
  assert sorted(os.listdir(train_dir)) == [
      'model.ckpt-4.npz', 'model.ckpt-4.state.npz', 'model.ckpt-6.npz',
      'model.ckpt-6.state.npz', 'summaries.jsonl']
  saved = train.load_checkpoint(*train.checkpoint_paths(str(train_dir), 6))
  assert saved['global_step'] == 6 and len(saved['slots']) == 1
  assert train.main(argv + ['--max_steps', '8']) == 8
  final = train.load_checkpoint(*train.checkpoint_paths(str(train_dir), 8))
  assert final['global_step'] == 8
  assert any(not np.array_equal(final['variables'][k], saved['variables'][k])
             for k in saved['variables'])
  with open(train_dir / 'summaries.jsonl') as f:
    lines = [json.loads(line) for line in f]
  assert [line['step'] for line in lines] == [6, 8]
  for line in lines:
    assert line['replicas'] == 2 and line['world'] == 1
    assert np.isfinite(line['loss'])
    assert abs(line['learning_rate'] - 0.01) < 1e-6
  # the resumed run started from the saved state: a fresh run of eight steps
  # takes the same examples for steps 1 .. 6 only, so it ends elsewhere, but
  # one resumed from a copy of the pair repeats steps 7 and 8 bit for bit
  again = tmp_path / 'again'
  os.makedirs(again)
  for path in train.checkpoint_paths(str(train_dir), 6):
    with open(path, 'rb') as src, open(
        again / os.path.basename(path), 'wb') as dst:
      dst.write(src.read())
  assert train.main(run_args + ['--replicas_to_aggregate', '2', '--train_dir',
                                str(again), '--max_steps', '8']) == 8
  assert_same_pair(read_pair(train, again, 8), read_pair(train, train_dir, 8))


CHILD_SECONDS = 150


def start_rank(argv, rank, world, port, log):
  env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world),
             LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1',
             MASTER_PORT=str(port))
  return subprocess.Popen(
      ['timeout', '-k', '10', str(CHILD_SECONDS), sys.executable,
       os.path.join(ROOT, 'train.py')] + argv,
      env=env, cwd=ROOT, stdout=log, stderr=subprocess.STDOUT)


def wait_for_ranks(children):
  """Ends at the first child that fails (the others are then stopped);
  returns once all have ended well."""
  pending = dict(enumerate(children))
  try:
    while pending:
      for rank, child in list(pending.items()):
        code = child.poll()
        if code is None:
          continue
        del pending[rank]
        assert code == 0, 'rank %d ended with %r' % (rank, code)
      if pending:
        try:
          next(iter(pending.values())).wait(timeout=0.2)
        except subprocess.TimeoutExpired:
          pass
  finally:
    for child in children:
      if child.poll() is None:
        child.kill()
        child.wait()


def free_port():
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    return s.getsockname()[1]


@pytest.fixture(scope='module')
def one_process_run(run_args, tmp_path_factory):
  """Three steps of four replicas in this process, no group: (the train
  script module, its train_dir)."""
  train = script('train')
  train_dir = tmp_path_factory.mktemp('one_process') / 'run'
  assert train.main(run_args + ['--replicas_to_aggregate', '4', '--train_dir',
                                str(train_dir), '--max_steps', '3']) == 3
  return train, train_dir


def test_two_ranks_on_one_gpu_equal_one_process(run_args, one_process_run,
                                                tmp_path):
  train, want_dir = one_process_run
  port = free_port()
  dirs = [tmp_path / 'rank0', tmp_path / 'rank1']
  logs = [open(tmp_path / ('rank%d.log' % r), 'w') for r in range(2)]
  try:
    children = [
        start_rank(run_args + [
            '--replicas_to_aggregate', '4', '--total_replicas', '4',
            '--train_dir', str(dirs[r]), '--max_steps', '3',
            '--collective_backend', 'gloo', '--ranks_share_gpus'],
                   r, 2, port, logs[r]) for r in range(2)]
    try:
      wait_for_ranks(children)
    finally:
      for log in logs:
        log.close()
      for r in range(2):
        with open(tmp_path / ('rank%d.log' % r)) as f:
          print('---- rank %d\n%s' % (r, f.read()[-3000:]))
  finally:
    for log in logs:
      log.close()
  assert_same_pair(read_pair(train, dirs[0], 3), read_pair(train, want_dir, 3))
  for r in range(2):
    with open(tmp_path / ('rank%d.log' % r)) as f:
      text = f.read()
    assert 'rank %d: ranks agree at step 3' % r in text
    assert 'rank %d of 2, 2 replicas here' % r in text
  # only the chief writes
  assert sorted(os.listdir(dirs[0])) == [
      'model.ckpt-3.npz', 'model.ckpt-3.state.npz', 'summaries.jsonl']
  assert not dirs[1].exists()
  with open(dirs[0] / 'summaries.jsonl') as f:
    line = json.loads(f.readline())
  assert (line['replicas'], line['world'], line['step']) == (4, 2, 3)
  with open(want_dir / 'summaries.jsonl') as f:
    alone = json.loads(f.readline())
  assert line['loss'] == alone['loss'] and line['clipped'] == alone['clipped']


def test_the_nccl_backend_at_world_one_equals_no_group(run_args,
                                                       one_process_run,
                                                       tmp_path):
  train, want_dir = one_process_run
  train_dir = tmp_path / 'nccl'
  with open(tmp_path / 'nccl.log', 'w') as log:
    child = start_rank(run_args + [
        '--replicas_to_aggregate', '4', '--train_dir', str(train_dir),
        '--max_steps', '3', '--collective_backend', 'nccl'], 0, 1,
                       free_port(), log)
    try:
      wait_for_ranks([child])
    finally:
      log.flush()
      with open(tmp_path / 'nccl.log') as f:
        print(f.read()[-3000:])
  assert_same_pair(read_pair(train, train_dir, 3),
                   read_pair(train, want_dir, 3))
  with open(tmp_path / 'nccl.log') as f:
    assert 'rank 0: ranks agree at step 3' in f.read()
