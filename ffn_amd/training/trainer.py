"""One training step of ConvStack3DFFNModel with everything resident on the GPU.

`ConvStackTrainer` composes the gradients unit (gradients.ConvStackGradients)
and the optimizer unit (optimizer.OptimizerOps) into "loss -> gradients ->
update", what reference model.set_up_optimizer and train.py's
run_training_step do for one batch: the loss and every weight gradient, the
clip of every gradient entry, one of five update rules with the staircase
learning-rate decay, and the step counter.

The variables, their gradients and the optimizer's slots each live in one flat
device array (optimizer.arena_layout); the gradient kernels read and write
views into these arrays and the update is one launch over all of them.  No
gradient or parameter crosses to the host in a step.  The example iterator is
training/examples.py, the loop and the checkpoint files are train.py's.  There
is no CPU fallback: without a GPU the constructor raises.

Synchronous replicas (the reference's --sync_sgd; training/replicas.py says
what a replica is): a trainer made with `replicas=K` also keeps a stash of K
gradient arenas.  `contribute(k, batch)` takes the loss and the gradient of one
replica under the current variables and stores the raw gradient in row k;
`apply_contributions()` gathers the stashes of all ranks of `group` into
[R][total] in replica order, has the optimizer unit clip every replica, fold
them in that order and divide by R (aggregate), and applies the result once
with no further clip.  `train_step` does not touch any of this.
"""

from __future__ import annotations

import numpy as np

from . import gradients as gradients_lib
from . import optimizer as optimizer_lib
from . import replicas as replicas_lib


class InvalidLossError(ArithmeticError):
  """The loss or a gradient entry of a step is not finite (the reference's
  check_numerics, 'Invalid loss detected'); the step changed nothing."""


class ConvStackTrainer:
  """Trains `model` (a ConvStack3DFFNModel with variables; any depth >= 2, 32
  features, any FoV) on batches of up to `max_batch` FoVs on device
  `device_id`.  The model object is read once and not written.

  replicas: K >= 1 local replicas for contribute / apply_contributions (0: a
    trainer for train_step only, with no stash).
  group: a replicas.ReplicaGroup of the job's ranks; None: this process is the
    whole job and no collective is issued."""

  def __init__(self, model, config=None, max_batch: int = 1,
               device_id: int = 0, replicas: int = 0, group=None):
    config = config if config is not None else optimizer_lib.OptimizerConfig()
    if not isinstance(config, optimizer_lib.OptimizerConfig):
      raise TypeError('config must be an OptimizerConfig')
    if model.variables is None:
      raise ValueError('model has no weights (load_checkpoint / init_random)')
    replicas = int(replicas)
    if replicas < 0:
      raise ValueError('replicas = %d, expected >= 0' % replicas)
    if group is not None and replicas < 1:
      raise ValueError('a group needs replicas >= 1')
    world = 1 if group is None else int(group.world)
    if replicas * world > replicas_lib.MAX_REPLICAS:
      raise ValueError('%d replicas on %d ranks: at most %d in all' %
                       (replicas, world, replicas_lib.MAX_REPLICAS))
    self.config = config
    self.replicas = replicas
    self.group = group
    # (before the library is loaded: torch brings its own copy of the HIP
    # runtime, and the process must end up with one)
    import torch  # pylint:disable=g-import-not-at-top
    self.ops = optimizer_lib.OptimizerOps(device_id)  # raises without a GPU
    self.csg = None
    try:
      self.torch = torch
      self.device = torch.device('cuda', device_id)
      self.layout = optimizer_lib.arena_layout(model.depth, model.features)
      self.params = self._upload(
          optimizer_lib.pack(model.variables, self.layout))
      self.grads = torch.zeros((self.layout.total,), dtype=torch.float32,
                               device=self.device)
      self.slots = [
          torch.full((self.layout.total,), init, dtype=torch.float32,
                     device=self.device)
          for init in optimizer_lib.SLOT_INIT[config.optimizer]]
      storage = {'w': {}, 'b': {}, 'dw': {}, 'db': {}}
      for e in self.layout.entries:
        _, scope, kind = e.name.split('/')
        key = 'w' if kind == 'weights' else 'b'
        storage[key][scope] = self.params[e.offset:e.offset + e.size]
        storage['d' + key][scope] = self.grads[e.offset:e.offset + e.size]
      self.stash = None
      if replicas:
        self.stash = torch.zeros((replicas, self.layout.total),
                                 dtype=torch.float32, device=self.device)
      torch.cuda.synchronize(self.device)
      self.csg = gradients_lib.ConvStackGradients(model, max_batch, device_id,
                                                  storage=storage)
    except Exception:
      self.ops.close()
      raise
    self.global_step = 0
    self.beta1_power, self.beta2_power = config.initial_powers()
    self.last_stats = None
    self._status = [None] * replicas  # a STATUS row per contribution held

  def _upload(self, flat):
    t = self.torch.from_numpy(np.ascontiguousarray(flat, np.float32))
    return t.to(self.device)

  def close(self):
    if self.csg is not None:
      self.csg.close()
    self.ops.close()

  # -- the step ------------------------------------------------------------------
  def train_step(self, seed, image, labels, weights):
    """train_step_device with the updated seed as numpy [n, z, y, x]."""
    loss, logits_dev, step = self.train_step_device(seed, image, labels,
                                                    weights)
    return loss, logits_dev.cpu().numpy(), step

  def train_step_device(self, seed, image, labels, weights):
    """seed, image, labels, weights: [n, z, y, x], numpy or device arrays.

    Returns (loss, logits, step): the loss of the batch under the variables
    before the update, the updated seed [n, z, y, x] as a device tensor that is
    valid until the next step, and the step counter after the update.  Raises
    InvalidLossError, having changed nothing, if the loss or a gradient entry
    is not finite."""
    cfg, total = self.config, self.layout.total
    loss, logits_dev = self.csg.loss_and_gradients_device(seed, image, labels,
                                                          weights)
    if not np.isfinite(loss):
      raise InvalidLossError('Invalid loss detected: loss = %r at step %d' %
                             (loss, self.global_step))
    clip = cfg.max_gradient_entry_mag
    max_abs, clipped, nonfinite = self.ops.grad_stats(total, self.grads, clip)
    if nonfinite:
      raise InvalidLossError(
          'Invalid loss detected: %d gradient entries are not finite at step '
          '%d' % (nonfinite, self.global_step))
    lr, c0, c1, eps = cfg.coefficients(self.global_step, self.beta1_power,
                                       self.beta2_power)
    self.ops.apply(cfg.rule, total, self.params, self.grads,
                   self.slots[0] if len(self.slots) > 0 else None,
                   self.slots[1] if len(self.slots) > 1 else None,
                   lr=lr, clip=clip, c0=c0, c1=c1, eps=eps)
    self.last_stats = {
        'loss': loss, 'max_abs': max_abs, 'clipped': clipped,
        'learning_rate': cfg.learning_rate_at(self.global_step)}
    self.global_step += 1
    if cfg.optimizer == 'adam':
      self.beta1_power, self.beta2_power = cfg.advance_powers(
          self.beta1_power, self.beta2_power)
    return loss, logits_dev, self.global_step

  # -- synchronous replicas -------------------------------------------------------
  def contribute(self, k, seed, image, labels, weights):
    """The loss and the gradient of local replica `k` for the coming update,
    under the current variables: (loss, logits), the logits as
    train_step_device returns them, valid until the next contribute.  The raw
    gradient goes to row k of the stash; a second contribution of a replica
    replaces its first.  Nothing is refused here: apply_contributions decides
    for all replicas of all ranks at once."""
    if not 0 <= int(k) < self.replicas:
      raise ValueError('local replica %r of %d' % (k, self.replicas))
    loss, logits_dev = self.csg.loss_and_gradients_device(seed, image, labels,
                                                          weights)
    max_abs, clipped, nonfinite = self.ops.grad_stats(
        self.layout.total, self.grads, self.config.max_gradient_entry_mag)
    self.stash[int(k)].copy_(self.grads)
    self.torch.cuda.synchronize(self.device)
    self._status[int(k)] = (float(loss), float(max_abs), float(clipped),
                            float(nonfinite))
    return loss, logits_dev

  def apply_contributions(self):
    """One update from the contributions of all R = world * K replicas;
    returns the step counter after it.  RuntimeError, with nothing changed, if
    a local replica has not contributed since the last update.  If any loss or
    gradient entry of any replica on any rank is not finite, every rank raises
    InvalidLossError: parameters, slots, step counter and beta powers stay as
    they are and the contributions are dropped."""
    cfg, total = self.config, self.layout.total
    missing = [k for k, row in enumerate(self._status) if row is None]
    if missing or not self.replicas:
      raise RuntimeError('apply_contributions: local replica(s) %s of %d have '
                         'not contributed' % (missing, self.replicas))
    status = np.asarray(self._status, np.float64)
    if self.group is not None:
      status = self.group.gather_status(status)
    count = status.shape[0]
    self._status = [None] * self.replicas
    bad = [r for r in range(count)
           if not np.isfinite(status[r, 0]) or status[r, 3] != 0]
    if bad:
      r = bad[0]
      raise InvalidLossError(
          'Invalid loss detected: replica(s) %s of %d at step %d (replica %d: '
          'loss = %r, %d gradient entries not finite)' %
          (bad, count, self.global_step, r, status[r, 0], int(status[r, 3])))
    gathered = (self.stash if self.group is None
                else self.group.gather_arena(self.stash))
    # clip per replica, then the mean (model.py:142-145 clips before
    # SyncReplicasOptimizer averages); the quotient may round one ulp past the
    # clip, so the update itself must not clip again
    self.ops.aggregate(total, count, gathered, total,
                       cfg.max_gradient_entry_mag, self.grads)
    lr, c0, c1, eps = cfg.coefficients(self.global_step, self.beta1_power,
                                       self.beta2_power)
    self.ops.apply(cfg.rule, total, self.params, self.grads,
                   self.slots[0] if len(self.slots) > 0 else None,
                   self.slots[1] if len(self.slots) > 1 else None,
                   lr=lr, clip=0.0, c0=c0, c1=c1, eps=eps)
    self.last_stats = {
        'loss': float(np.mean(status[:, 0])),
        'max_abs': float(np.max(status[:, 1])),
        'clipped': int(np.sum(status[:, 2])),
        'learning_rate': cfg.learning_rate_at(self.global_step),
        'replicas': count}
    self.global_step += 1
    if cfg.optimizer == 'adam':
      self.beta1_power, self.beta2_power = cfg.advance_powers(
          self.beta1_power, self.beta2_power)
    return self.global_step

  def parameter_checksum(self):
    """Two int64 sums over the bits of the parameter arena, taken on the
    device: the plain sum and the sum weighted by position (both modulo
    2^64)."""
    torch = self.torch
    bits = self.params.view(torch.int32).to(torch.int64)
    weights = torch.arange(1, bits.numel() + 1, dtype=torch.int64,
                           device=self.device)
    sums = torch.stack([bits.sum(), (bits * weights).sum()])
    return [int(v) for v in sums.cpu().tolist()]

  def check_ranks_agree(self):
    """The divergence guard: every rank of the group holds the same parameter
    bits and step counter, else replicas.ReplicasDivergedError on every rank.
    Collective; nothing to do without a group."""
    if self.group is not None:
      self.group.check_same(
          self.parameter_checksum() + [int(self.global_step)],
          'parameters or step counters')

  # -- state ---------------------------------------------------------------------
  def _download(self, arena):
    return optimizer_lib.unpack(arena.cpu().numpy(), self.layout)

  def variables(self):
    """{checkpoint name: numpy array in the checkpoint's shape}."""
    return self._download(self.params)

  def gradients(self):
    """The raw (unclipped) gradients of the last step or the last contribute,
    like variables(); after apply_contributions, the aggregated gradient."""
    return self._download(self.grads)

  def slot_variables(self):
    """One dict like variables() per slot of the rule."""
    return [self._download(s) for s in self.slots]

  def state(self):
    """Everything a resumed run needs, as plain numpy and Python values."""
    return {'variables': self.variables(), 'slots': self.slot_variables(),
            'global_step': int(self.global_step),
            'beta1_power': np.float32(self.beta1_power),
            'beta2_power': np.float32(self.beta2_power),
            'config': self.config.to_dict()}

  def load_state(self, state):
    """Takes a state() of a trainer of the same model shape and optimizer."""
    config = optimizer_lib.OptimizerConfig.from_dict(state['config'])
    if config.optimizer != self.config.optimizer:
      raise ValueError('state of optimizer %r, this trainer runs %r' %
                       (config.optimizer, self.config.optimizer))
    if len(state['slots']) != len(self.slots):
      raise ValueError('state has %d slots, expected %d' %
                       (len(state['slots']), len(self.slots)))
    inits = optimizer_lib.SLOT_INIT[config.optimizer]
    # pack everything first: a state that does not fit changes nothing
    params = optimizer_lib.pack(state['variables'], self.layout)
    slots = [optimizer_lib.pack(s, self.layout, fill=init)
             for s, init in zip(state['slots'], inits)]
    self.params.copy_(self._upload(params))
    for dst, src in zip(self.slots, slots):
      dst.copy_(self._upload(src))
    self.torch.cuda.synchronize(self.device)
    self.config = config
    self._status = [None] * self.replicas  # taken under other variables
    self.global_step = int(state['global_step'])
    self.beta1_power = np.float32(state['beta1_power'])
    self.beta2_power = np.float32(state['beta2_power'])
