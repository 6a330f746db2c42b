"""Synchronous replicas without a GPU: the numpy restatement of the fold
(tests/replicas_ref.py), the split of coordinates and seeds over replicas
(ffn_amd/training/replicas.py), train.py's flags, and ReplicaGroup at world 2
under gloo on CPU tensors."""
import importlib.util
import os
import socket

import numpy as np
import pytest

from tests import replicas_ref as rref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def script(name):
  spec = importlib.util.spec_from_file_location(
      name + '_script', os.path.join(ROOT, name + '.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def bits(a):
  return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the fold ----------------------------------------------------------------------


def test_fold_is_ordered_left_to_right():
  for triple in (rref.ORDER_TRIPLE, rref.ORDER_TRIPLE_SMALL):
    a, b, c = triple
    assert F32(F32(a + b) + c) != F32(a + F32(b + c))
    rows = [np.array([v], F32) for v in triple]
    got = rref.fold(rows, 0.0)
    assert got[0] == F32(F32(F32(a + b) + c) / F32(3))
    assert got[0] == 0
    # the other order is another number
    assert rref.fold(rows[::-1], 0.0)[0] != 0
  # the small triple lies inside the clip, the large one does not
  small = [np.array([v], F32) for v in rref.ORDER_TRIPLE_SMALL]
  assert rref.fold(small, 0.7)[0] == 0
  large = [np.array([v], F32) for v in rref.ORDER_TRIPLE]
  assert rref.fold(large, 0.7)[0] == F32(F32(F32(0.7) + F32(0.7)) -
                                         F32(0.7)) / F32(3)


def test_fold_clips_each_replica_before_the_sum():
  rows = [np.array([3.0, -3.0, 0.25], F32), np.array([-0.5, 0.5, 0.25], F32)]
  got = rref.fold(rows, 0.7)
  clip = F32(0.7)
  assert got[0] == F32(F32(clip + F32(-0.5)) / F32(2))
  assert got[1] == F32(F32(-clip + F32(0.5)) / F32(2))
  assert got[2] == F32(0.25)
  assert np.array_equal(rref.fold(rows, 0.0), np.array([1.25, -1.25, 0.25],
                                                       F32))


def test_fold_of_one_keeps_the_bits():
  row = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf, 1e-41, -1e-41, 0.9,
                  -0.9], F32)
  got = rref.fold([row], 0.7)
  want = np.array([-0.0, 0.0, np.nan, 0.7, -0.7, 1e-41, -1e-41, 0.7, -0.7],
                  F32)
  assert np.array_equal(bits(got), bits(want))
  assert np.array_equal(bits(rref.fold([row], 0.0)), bits(row))


def test_fold_strided_reads_the_rows():
  count, n, stride = 5, 3, 8
  src = np.arange(n * stride, dtype=np.float32) / F32(64)
  want = rref.fold([src[0:5], src[8:13], src[16:21]], 0.2)
  assert np.array_equal(rref.fold_strided(src, count, n, stride, 0.2), want)


def test_the_mean_may_pass_the_clip():
  """Why apply_contributions applies with clip 0: the sum of n clipped values
  divided by n need not be the clipped value again (every partial sum
  rounds), so a second clip would change bits."""
  clip = F32(0.7)
  above = [n for n in range(2, 65)
           if rref.fold([np.array([5.0], F32)] * n, clip)[0] > clip]
  assert above
  assert rref.fold([np.array([5.0], F32)] * 2, clip)[0] == clip  # exact


# ---- the split ---------------------------------------------------------------------


def test_shards_are_disjoint_complete_and_know_no_ranks():
  from ffn_amd.training import replicas
  items = [((i, 2 * i, 3 * i), 'v%d' % (i % 3)) for i in range(23)]
  for total in (1, 2, 4, 5, 23, 24):
    shards = [replicas.shard(items, r, total) for r in range(total)]
    flat = [x for s in shards for x in s]
    assert len(flat) == len(items) and set(flat) == set(items)
    for r, s in enumerate(shards):
      assert s == items[r::total]  # file order
  # the deal to ranks does not enter: replica r of R is rank * K + k
  total = 4
  for world in (1, 2, 4):
    k_per = replicas.per_rank(total, world)
    seen = []
    for rank in range(world):
      for k in range(k_per):
        r = replicas.global_index(rank, k, k_per)
        seen.append(r)
        assert replicas.shard(items, r, total) == items[r::total]
        assert replicas.stream_seeds(11, r) == {
            'shuffle_seed': 11 + r, 'transform_seed': 11 + r,
            'sections_seed': 11 + r, 'moves_seed': 11}
    assert seen == list(range(total))
  with pytest.raises(ValueError):
    replicas.shard(items, 4, 4)
  with pytest.raises(ValueError):
    replicas.per_rank(5, 2)
  with pytest.raises(ValueError):
    replicas.per_rank(512, 2)
  with pytest.raises(ValueError):
    replicas.global_index(0, 2, 2)


def test_replica_streams_take_their_shards_and_share_one_result():
  """Two replicas' iterators over the restated unit: each cycles its own
  shard in file order, and both score into the one EvalResult."""
  from ffn_amd.training import evaluation
  from ffn_amd.training import examples
  from ffn_amd.training import replicas
  from tests import test_training_loop as loop
  from tests import training_ref
  volumes = loop.fixture_volumes()
  coordinates = loop.FIXTURE['coordinates'][:4]
  info = loop.Info(loop.FIXTURE['fov_xyz'], loop.FIXTURE['deltas_xyz'])

  def run(batches, steps):
    for _ in range(steps):
      seed, _, _, _ = batches.next()
      # a network that refuses every move: one step per example
      batches.update_seeds(np.full(seed.shape, -5.0, np.float32))

  alone = examples.BatchExampleIter(info, training_ref.RefOps(), volumes,
                                    coordinates, batch_size=1)
  own = alone.result
  run(alone, 3)
  assert alone.result is own and own.num_patches == alone.examples_finished
  alone.reset_result()
  assert alone.result is not own and alone.result.num_patches == 0

  shared = None
  streams = []
  for r in range(2):
    batches = examples.BatchExampleIter(
        info, training_ref.RefOps(), volumes,
        replicas.shard(coordinates, r, 2), batch_size=1, keep_history=True,
        result=shared)
    shared = batches.result
    streams.append(batches)
  assert streams[0].result is streams[1].result
  for _ in range(3):
    for batches in streams:
      run(batches, 1)
  for r, batches in enumerate(streams):
    taken = [batches.coordinates[e['coordinate']] for e in batches.history]
    want = [(tuple(c), n) for c, n in coordinates[r::2]]
    assert taken[:2] == want
  finished = sum(b.examples_finished for b in streams)
  assert finished >= 4 and shared.num_patches == finished
  fresh = evaluation.EvalResult(streams[0].shifts)
  for batches in streams:
    batches.reset_result(fresh)
  assert all(b.result is fresh for b in streams)


# ---- train.py's flags --------------------------------------------------------------

REQUIRED = ['--train_coords', 'c', '--data_volumes', 'a:i.npy',
            '--label_volumes', 'a:l.npy', '--model_name',
            'convstack_3d.ConvStack3DFFNModel', '--model_args', '{"depth": 3}',
            '--image_mean', '128', '--image_stddev', '33']


def test_train_flags_of_sync_replicas(monkeypatch, capsys):
  train = script('train')
  for name in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
    monkeypatch.delenv(name, raising=False)
  args = train.parse_args(REQUIRED)
  assert args.sync_sgd is False and args.replicas_to_aggregate is None
  assert args.total_replicas is None and args.collective_backend == 'nccl'
  assert args.ranks_share_gpus is False
  assert (args.batch_size, args.max_steps, args.optimizer) == (4, 10000, 'sgd')
  # without --sync_sgd the replica flags decide nothing
  args = train.parse_args(REQUIRED + ['--replicas_to_aggregate', '3'])
  assert args.sync_sgd is False
  args = train.parse_args(REQUIRED + ['--sync_sgd', '--replicas_to_aggregate',
                                      '3', '--total_replicas', '3'])
  assert args.sync_sgd is True and args.replicas_to_aggregate == 3
  assert train.job_environment({}) == (0, 1, 0, False)
  assert train.job_environment({'RANK': '3', 'WORLD_SIZE': '4',
                                'LOCAL_RANK': '1'}) == (3, 4, 1, True)

  def refused(extra, word):
    with pytest.raises(SystemExit):
      train.parse_args(REQUIRED + extra)
    assert word in capsys.readouterr().err

  refused(['--sync_sgd'], 'replicas_to_aggregate')
  refused(['--sync_sgd', '--replicas_to_aggregate', '0'], 'replicas')
  refused(['--sync_sgd', '--replicas_to_aggregate', '2', '--total_replicas',
           '3'], 'backup replicas are not mirrored')
  refused(['--sync_sgd', '--replicas_to_aggregate', '2', '--ranks_share_gpus'],
          'gloo')
  args = train.parse_args(REQUIRED + [
      '--sync_sgd', '--replicas_to_aggregate', '2', '--ranks_share_gpus',
      '--collective_backend', 'gloo'])
  assert args.ranks_share_gpus is True
  # a job of two ranks
  monkeypatch.setenv('RANK', '1')
  monkeypatch.setenv('WORLD_SIZE', '2')
  refused(['--sync_sgd', '--replicas_to_aggregate', '3'], 'evenly')
  refused([], '--sync_sgd')
  args = train.parse_args(REQUIRED + ['--sync_sgd', '--replicas_to_aggregate',
                                      '4'])
  assert args.replicas_to_aggregate == 4


# ---- the group, world 2, gloo, CPU tensors ---------------------------------------

K, TOTAL = 2, 12


def _row(r):
  return np.arange(TOTAL, dtype=np.float32) + F32(100 * r)


def _group_worker(rank, world, port, tmpdir):
  import torch
  import torch.distributed as dist
  from ffn_amd.training import replicas
  os.environ['MASTER_ADDR'] = '127.0.0.1'
  os.environ['MASTER_PORT'] = str(port)
  dist.init_process_group('gloo', rank=rank, world_size=world)
  try:
    group = replicas.ReplicaGroup()
    assert (group.rank, group.world, group.backend) == (rank, world, 'gloo')
    stash = torch.from_numpy(np.stack(
        [_row(replicas.global_index(rank, k, K)) for k in range(K)]))
    for turn in range(2):  # the second call reuses the group's buffer
      arena = group.gather_arena(stash + turn)
      np.save(os.path.join(tmpdir, 'arena%d_%d.npy' % (turn, rank)),
              arena.numpy())
    # rank 1's second replica comes with a loss that is not finite
    status = np.array([[0.5 + rank * K + k, 0.1 * (rank * K + k), rank, 0]
                       for k in range(K)], np.float64)
    if rank == 1:
      status[1, 0] = np.nan
    np.save(os.path.join(tmpdir, 'status_%d.npy' % rank),
            group.gather_status(status))
    np.save(os.path.join(tmpdir, 'seed_%d.npy' % rank),
            np.array([group.rank0_value(1000 + rank)]))
    group.check_same([7, -3, 2 ** 62])
    try:
      group.check_same([7, rank])
      diverged = False
    except replicas.ReplicasDivergedError:
      diverged = True
    np.save(os.path.join(tmpdir, 'diverged_%d.npy' % rank),
            np.array([diverged]))
    dist.barrier()
  finally:
    dist.destroy_process_group()


def test_group_world2_gloo_orders_rows_by_replica(tmp_path):
  import torch.multiprocessing as mp
  with socket.socket() as s:
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
  world = 2
  mp.spawn(_group_worker, args=(world, port, str(tmp_path)), nprocs=world,
           join=True)
  want = np.stack([_row(r) for r in range(world * K)])
  for rank in range(world):
    for turn in range(2):
      got = np.load(tmp_path / ('arena%d_%d.npy' % (turn, rank)))
      assert np.array_equal(got, want + turn), (rank, turn)
    status = np.load(tmp_path / ('status_%d.npy' % rank))
    assert status.shape == (world * K, 4)
    assert np.array_equal(status[:3, 0], [0.5, 1.5, 2.5])
    assert np.isnan(status[3, 0])  # seen by both ranks, in row rank * K + k
    assert np.array_equal(status[:, 2], [0, 0, 1, 1])
    assert np.load(tmp_path / ('seed_%d.npy' % rank))[0] == 1000
    assert np.load(tmp_path / ('diverged_%d.npy' % rank))[0]
