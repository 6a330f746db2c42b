"""Synchronous replicas of a training step: who holds which replica, and the
exchange between the processes of a job.

A replica is a unit of work, not a process: one batch whose gradient is taken
under the variables of the step, clipped on its own and averaged with the
others before one update (the reference's --sync_sgd, model.py:142-145 and
optimizer.py:114-128: clip, then SyncReplicasOptimizer's mean).  A process
("rank") holds K local replicas; a job of `world` ranks has R = world * K, and
the global index of local replica k on rank `rank` is rank * K + k.  Everything
a replica computes depends on (seed, r, R) only, never on the rank that hosts
it, and the fold over the replicas is the optimizer unit's own kernel in
replica order (include/ffn_optimizer.h, aggregate), so the ranks exchange raw
gradients with an all-gather and no collective library's summation order
enters the result.

`ReplicaGroup` is that exchange over torch.distributed.  Under the nccl
backend (RCCL) the collectives run on device tensors; under gloo they run on
host tensors, device arrays going through pinned host buffers.  CPU tensors
work under gloo as they are, which is how the ordering is tested without a
GPU.  A trainer without a group (`group=None`) is one process and issues no
collective at all.

`shard` and `stream_seeds` say which coordinates and which random streams a
global replica owns.  No run on more than one GPU exists yet; nothing here
claims a scaling number.
"""

from __future__ import annotations

import numpy as np

#: columns of a status row
STATUS = ('loss', 'max_abs', 'clipped', 'nonfinite')
#: what one aggregate folds (ffn_optimizer.h)
MAX_REPLICAS = 256


def global_index(rank: int, local: int, per_rank: int) -> int:
  """Global replica index of local replica `local` on rank `rank`."""
  if not 0 <= local < per_rank:
    raise ValueError('local replica %d of %d' % (local, per_rank))
  return int(rank) * int(per_rank) + int(local)


def shard(items, replica: int, replicas: int):
  """The items global replica `replica` of `replicas` owns: items[r::R], in
  their order.  The shards of r = 0 .. R - 1 are disjoint and together
  complete, and one depends on (r, R) only, not on how many ranks host the
  replicas."""
  if not 0 <= int(replica) < int(replicas):
    raise ValueError('replica %r of %r' % (replica, replicas))
  return list(items)[int(replica)::int(replicas)]


def stream_seeds(seed: int, replica: int):
  """The seeds of global replica `replica`'s example stream: the coordinate
  shuffle, the augmentation generators and the section generator are its own
  (seed + r); the order of moves is the job's (train.py:353-355 shuffles
  model.shifts once)."""
  own = int(seed) + int(replica)
  return {'shuffle_seed': own, 'transform_seed': own, 'sections_seed': own,
          'moves_seed': int(seed)}


def per_rank(replicas: int, world: int) -> int:
  """K of R = world * K."""
  if replicas < 1 or world < 1 or replicas % world:
    raise ValueError('%d replicas cannot be dealt evenly to %d ranks' %
                     (replicas, world))
  if replicas > MAX_REPLICAS:
    raise ValueError('%d replicas, at most %d' % (replicas, MAX_REPLICAS))
  return replicas // world


class ReplicasDivergedError(RuntimeError):
  """The ranks of a job no longer hold the same parameters."""


class ReplicaGroup:
  """The ranks of a job, over an initialised torch.distributed process group.

  device: the torch device of this rank's arrays (None: CPU tensors only).
  rank, world, backend are the process group's.
  """

  def __init__(self, device=None, process_group=None):
    import torch  # pylint:disable=g-import-not-at-top
    import torch.distributed as dist  # pylint:disable=g-import-not-at-top
    if not dist.is_initialized():
      raise RuntimeError('ReplicaGroup needs torch.distributed.'
                         'init_process_group first')
    self.torch, self.dist = torch, dist
    self.pg = process_group
    self.rank = int(dist.get_rank(process_group))
    self.world = int(dist.get_world_size(process_group))
    self.backend = str(dist.get_backend(process_group))
    self.device = None if device is None else torch.device(device)
    if self.backend == 'nccl' and (self.device is None or
                                   self.device.type != 'cuda'):
      raise ValueError('the nccl backend needs a GPU device')
    self._host_in = self._host_out = self._out = None

  # -- small host values ---------------------------------------------------------
  def gather_rows(self, rows: np.ndarray) -> np.ndarray:
    """rows [k, ...] of every rank (same shape and dtype everywhere) ->
    [world * k, ...] in rank order, on the host."""
    rows = np.ascontiguousarray(rows)
    torch, dist = self.torch, self.dist
    mine = torch.from_numpy(rows.reshape(-1).copy())
    if self.backend == 'nccl':
      mine = mine.to(self.device)
    parts = [torch.empty_like(mine) for _ in range(self.world)]
    dist.all_gather(parts, mine, group=self.pg)
    out = np.stack([p.cpu().numpy() for p in parts])
    return out.reshape((self.world * rows.shape[0],) + rows.shape[1:])

  def gather_status(self, rows) -> np.ndarray:
    """One float64 row of STATUS per local replica -> [R, 4] rows in global
    replica order (rank * K + k), the same on every rank."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 2 or rows.shape[1] != len(STATUS):
      raise ValueError('status rows of shape %r' % (rows.shape,))
    return self.gather_rows(rows)

  def rank0_value(self, value: int) -> int:
    """Rank 0's `value` (an int64), on every rank."""
    return int(self.gather_rows(np.array([int(value)], np.int64))[0])

  def check_same(self, values, what: str = 'parameters'):
    """Raises ReplicasDivergedError on every rank unless all ranks came with
    the same int64 `values`."""
    got = self.gather_rows(np.asarray(values, np.int64).reshape(1, -1))
    differ = [r for r in range(self.world) if not np.array_equal(got[r],
                                                                 got[0])]
    if differ:
      raise ReplicasDivergedError(
          'the %s of rank(s) %s differ from rank 0\'s (checksums %s)' %
          (what, differ, got.tolist()))

  # -- the gradient arenas -------------------------------------------------------
  def gather_arena(self, stash):
    """stash [K, total] f32 (this rank's replicas, on its device or on the
    host) -> [world * K, total] in global replica order, where `stash` lives.
    The result is the group's own buffer, valid until the next call."""
    torch, dist = self.torch, self.dist
    if stash.dim() != 2 or not stash.is_contiguous():
      raise ValueError('stash must be a dense [K, total] array')
    k, total = stash.shape
    shape = (self.world * k, total)
    if self._out is None or tuple(self._out.shape) != shape or (
        self._out.device != stash.device):
      self._out = torch.empty(shape, dtype=stash.dtype, device=stash.device)
      self._host_in = self._host_out = None
    out = self._out
    if self.backend == 'nccl':
      dist.all_gather_into_tensor(out, stash, group=self.pg)
      torch.cuda.synchronize(self.device)
      return out
    # gloo: host tensors; a device array goes through pinned buffers
    if stash.device.type == 'cpu':
      dist.all_gather(list(out.view(self.world, k, total).unbind(0)), stash,
                      group=self.pg)
      return out
    if self._host_in is None:
      self._host_in = torch.empty((k, total), dtype=stash.dtype,
                                  pin_memory=True)
      self._host_out = torch.empty(shape, dtype=stash.dtype, pin_memory=True)
    self._host_in.copy_(stash, non_blocking=True)
    torch.cuda.synchronize(stash.device)
    dist.all_gather(
        list(self._host_out.view(self.world, k, total).unbind(0)),
        self._host_in, group=self.pg)
    out.copy_(self._host_out, non_blocking=True)
    torch.cuda.synchronize(stash.device)
    return out
