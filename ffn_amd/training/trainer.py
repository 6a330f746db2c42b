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
"""

from __future__ import annotations

import numpy as np

from . import gradients as gradients_lib
from . import optimizer as optimizer_lib


class InvalidLossError(ArithmeticError):
  """The loss or a gradient entry of a step is not finite (the reference's
  check_numerics, 'Invalid loss detected'); the step changed nothing."""


class ConvStackTrainer:
  """Trains `model` (a ConvStack3DFFNModel with variables; any depth >= 2, 32
  features, any FoV) on batches of up to `max_batch` FoVs on device
  `device_id`.  The model object is read once and not written."""

  def __init__(self, model, config=None, max_batch: int = 1,
               device_id: int = 0):
    config = config if config is not None else optimizer_lib.OptimizerConfig()
    if not isinstance(config, optimizer_lib.OptimizerConfig):
      raise TypeError('config must be an OptimizerConfig')
    if model.variables is None:
      raise ValueError('model has no weights (load_checkpoint / init_random)')
    self.config = config
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
      torch.cuda.synchronize(self.device)
      self.csg = gradients_lib.ConvStackGradients(model, max_batch, device_id,
                                                  storage=storage)
    except Exception:
      self.ops.close()
      raise
    self.global_step = 0
    self.beta1_power, self.beta2_power = config.initial_powers()
    self.last_stats = None

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

  # -- state ---------------------------------------------------------------------
  def _download(self, arena):
    return optimizer_lib.unpack(arena.cpu().numpy(), self.layout)

  def variables(self):
    """{checkpoint name: numpy array in the checkpoint's shape}."""
    return self._download(self.params)

  def gradients(self):
    """The raw (unclipped) gradients of the last step, like variables()."""
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
    self.global_step = int(state['global_step'])
    self.beta1_power = np.float32(state['beta1_power'])
    self.beta2_power = np.float32(state['beta2_power'])
