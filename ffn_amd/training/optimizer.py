"""The parameter update of a training step on the GPU.

`OptimizerOps` is the handle over the optimizer unit of libffn_hip.so
(include/ffn_optimizer.h): gradient statistics and the clipped update of one
of five rules over flat f32 device arrays, one launch for all elements, and
`aggregate`, the clipped mean of the gradients of n replicas in replica order.

`OptimizerConfig` mirrors the flags of reference ffn/training/optimizer.py and
model.py:127 with their defaults, and owns the learning-rate schedule
(optimizer.py:80-86: exponential decay, staircase).  sync_sgd and the replica
flags are train.py's and the trainer's (trainer.ConvStackTrainer.contribute,
apply_contributions), not this class's.

The arena layout (`arena_layout`, `pack`, `unpack`) says where each variable of
a conv stack lies in the flat arrays a trainer hands to the unit; it is plain
numpy and needs no GPU.  There is no CPU fallback: without a GPU `OptimizerOps`
raises.
"""

from __future__ import annotations

import collections
import ctypes
import threading

import numpy as np

from .. import _unit
from .._lib import check
from .models import convstack_3d

#: rule numbers of include/ffn_optimizer.h
RULES = ('sgd', 'momentum', 'adagrad', 'adam', 'rmsprop')
#: rule -> initial value of each slot it uses (ffn_optimizer.h's table)
SLOT_INIT = {'sgd': (), 'momentum': (0.0,), 'adagrad': (0.1,),
             'adam': (0.0, 0.0), 'rmsprop': (1.0, 0.0)}
#: what `last_timing` indexes
TIMED_CALLS = ('grad_stats', 'apply')
ALIGN = 4  # floats: every tensor of an arena starts 16-byte aligned


def _addr(a) -> int:
  """Address of a device array: an int, None (NULL) or an object with
  data_ptr()."""
  if a is None:
    return 0
  if hasattr(a, 'data_ptr'):
    return int(a.data_ptr())
  return int(a)


class OptimizerOps(_unit.Handle):
  """One stream + workspace for the update kernels.  Every array argument is
  the address of dense, 16-byte aligned f32 device memory (or an object with
  data_ptr()) holding `count` floats."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_optimizer_create', 'ffn_optimizer_destroy',
                     device_id)
    self.lock = threading.RLock()

  def grad_stats(self, count, grads, clip):
    """(max_abs over the finite entries, number of finite entries with
    |g| > clip, number of non-finite entries)."""
    max_abs = ctypes.c_float(0.0)
    clipped, nonfinite = ctypes.c_uint64(0), ctypes.c_uint64(0)
    with self.lock:
      check(self._lib.ffn_optimizer_grad_stats(
          self._h, int(count), _addr(grads), float(clip),
          ctypes.byref(max_abs), ctypes.byref(clipped),
          ctypes.byref(nonfinite)))
    return float(max_abs.value), int(clipped.value), int(nonfinite.value)

  def apply(self, rule, count, params, grads, slot0=None, slot1=None, lr=0.0,
            clip=0.0, c0=0.0, c1=0.0, eps=0.0):
    """One update of `params` (and the slots) in place; `rule` is a name of
    RULES or its number."""
    if isinstance(rule, str):
      rule = RULES.index(rule)
    with self.lock:
      check(self._lib.ffn_optimizer_apply(
          self._h, int(rule), int(count), _addr(params), _addr(grads),
          _addr(slot0), _addr(slot1), float(lr), float(clip), float(c0),
          float(c1), float(eps)))

  def aggregate(self, count, n, src, stride, clip, dst):
    """dst = the mean of the `n` arrays of `count` floats that lie `stride`
    floats apart in `src`, each clipped first, folded in the order they lie
    (ffn_optimizer.h's definition: the gradients of n replicas)."""
    with self.lock:
      check(self._lib.ffn_optimizer_aggregate(
          self._h, int(count), int(n), _addr(src), int(stride), float(clip),
          _addr(dst)))

  def last_timing(self):
    """{call name: HIP-event kernel ms of its last run on this handle}."""
    ms = (ctypes.c_double * len(TIMED_CALLS))()
    with self.lock:
      check(self._lib.ffn_optimizer_last_timing(self._h, ms))
    return dict(zip(TIMED_CALLS, [float(v) for v in ms]))

  def last_timing_aggregate(self) -> float:
    """HIP-event kernel ms of the last aggregate on this handle."""
    ms = ctypes.c_double(0.0)
    with self.lock:
      check(self._lib.ffn_optimizer_last_timing_aggregate(
          self._h, ctypes.byref(ms)))
    return float(ms.value)


_default = _unit.Registry(OptimizerOps)


def default_ops(device_id: int = 0) -> OptimizerOps:
  """Process-wide OptimizerOps of a device (created on first use)."""
  return _default.get(device_id)


class OptimizerConfig:
  """The optimizer flags of the reference, validated."""

  FIELDS = ('optimizer', 'learning_rate', 'momentum',
            'learning_rate_decay_factor', 'decay_steps', 'rmsprop_decay',
            'adam_beta1', 'adam_beta2', 'epsilon', 'max_gradient_entry_mag')

  def __init__(self, optimizer='sgd', learning_rate=0.001, momentum=0.9,
               learning_rate_decay_factor=None, decay_steps=None,
               rmsprop_decay=0.9, adam_beta1=0.9, adam_beta2=0.999,
               epsilon=1e-8, max_gradient_entry_mag=0.7):
    if optimizer not in RULES:
      raise ValueError('Unknown optimizer: %r (one of %s)' %
                       (optimizer, ', '.join(RULES)))
    if not (np.isfinite(learning_rate) and learning_rate > 0):
      raise ValueError('learning_rate = %r, expected > 0' % (learning_rate,))
    for name, v in (('momentum', momentum), ('rmsprop_decay', rmsprop_decay),
                    ('adam_beta1', adam_beta1), ('adam_beta2', adam_beta2)):
      if not 0 <= v < 1:
        raise ValueError('%s = %r, expected 0 <= value < 1' % (name, v))
    if learning_rate_decay_factor is not None and not (
        np.isfinite(learning_rate_decay_factor) and
        learning_rate_decay_factor > 0):
      raise ValueError('learning_rate_decay_factor = %r, expected > 0' %
                       (learning_rate_decay_factor,))
    if decay_steps is not None and (int(decay_steps) != decay_steps or
                                    decay_steps < 1):
      raise ValueError('decay_steps = %r, expected an integer >= 1' %
                       (decay_steps,))
    # > 0: a zero gradient entry (a pad of the arena, a dead channel) must not
    # become 0 / 0 under adam and rmsprop
    if not (np.isfinite(epsilon) and epsilon > 0):
      raise ValueError('epsilon = %r, expected > 0' % (epsilon,))
    if not (np.isfinite(max_gradient_entry_mag) and
            max_gradient_entry_mag >= 0):
      raise ValueError('max_gradient_entry_mag = %r, expected >= 0 (0: no '
                       'clip)' % (max_gradient_entry_mag,))
    self.optimizer = optimizer
    self.learning_rate = float(learning_rate)
    self.momentum = float(momentum)
    self.learning_rate_decay_factor = (
        None if learning_rate_decay_factor is None
        else float(learning_rate_decay_factor))
    self.decay_steps = None if decay_steps is None else int(decay_steps)
    self.rmsprop_decay = float(rmsprop_decay)
    self.adam_beta1 = float(adam_beta1)
    self.adam_beta2 = float(adam_beta2)
    self.epsilon = float(epsilon)
    self.max_gradient_entry_mag = float(max_gradient_entry_mag)

  def to_dict(self):
    return {k: getattr(self, k) for k in self.FIELDS}

  @classmethod
  def from_dict(cls, d):
    return cls(**{k: d[k] for k in cls.FIELDS if k in d})

  def __eq__(self, other):
    return (isinstance(other, OptimizerConfig) and
            self.to_dict() == other.to_dict())

  def __repr__(self):
    return 'OptimizerConfig(%s)' % ', '.join(
        '%s=%r' % kv for kv in self.to_dict().items())

  @property
  def rule(self) -> int:
    return RULES.index(self.optimizer)

  @property
  def num_slots(self) -> int:
    return len(SLOT_INIT[self.optimizer])

  def learning_rate_at(self, step: int) -> np.float32:
    """The learning rate of the update that takes global_step `step` to
    step + 1: lr0 * factor ** floor(step / decay_steps), in f32."""
    lr0 = np.float32(self.learning_rate)
    if self.learning_rate_decay_factor is None or self.decay_steps is None:
      return lr0
    k = np.float32(int(step) // self.decay_steps)
    return np.float32(lr0 * np.float32(self.learning_rate_decay_factor) ** k)

  def initial_powers(self):
    """(beta1^1, beta2^1) as f32: adam's state before its first step."""
    return np.float32(self.adam_beta1), np.float32(self.adam_beta2)

  def advance_powers(self, b1p, b2p):
    return (np.float32(np.float32(b1p) * np.float32(self.adam_beta1)),
            np.float32(np.float32(b2p) * np.float32(self.adam_beta2)))

  def coefficients(self, step: int, b1p=None, b2p=None):
    """(lr, c0, c1, eps) of ffn_optimizer_apply for the update at global_step
    `step`, every value an np.float32 computed in f32.  b1p, b2p: adam's
    beta powers before this step."""
    one = np.float32(1)
    lr = self.learning_rate_at(step)
    c0 = c1 = np.float32(0)
    eps = np.float32(self.epsilon)
    if self.optimizer == 'momentum':
      c0 = np.float32(self.momentum)
    elif self.optimizer == 'adam':
      c0 = np.float32(one - np.float32(self.adam_beta1))
      c1 = np.float32(one - np.float32(self.adam_beta2))
      lr = np.float32(np.float32(lr * np.sqrt(np.float32(one - np.float32(b2p))))
                      / np.float32(one - np.float32(b1p)))
    elif self.optimizer == 'rmsprop':
      c0 = np.float32(one - np.float32(self.rmsprop_decay))
      c1 = np.float32(self.momentum)
    return lr, c0, c1, eps


# -- arena layout ----------------------------------------------------------------

Entry = collections.namedtuple('Entry', 'name shape offset size')


class Layout(collections.namedtuple('Layout', 'entries total count')):
  """entries: one Entry per variable in arena order; total: floats in the
  arena, pads included (a multiple of 4); count: floats in variables."""


def variable_shape(scope: str, features: int = 32):
  """(weights shape, biases shape) of a scope, as in the checkpoint."""
  w = ((3, 3, 3, 2, features) if scope == 'conv0_a' else
       (1, 1, 1, features, 1) if scope == 'conv_lom' else
       (3, 3, 3, features, features))
  return w, w[-1:]


def arena_layout(depth: int, features: int = 32) -> Layout:
  """Variables in conv_scopes(depth) order, weights then biases per scope, each
  starting at a multiple of ALIGN floats; the total is rounded up likewise."""
  entries, offset, count = [], 0, 0
  for scope in convstack_3d.conv_scopes(depth):
    for kind, shape in zip(('weights', 'biases'),
                           variable_shape(scope, features)):
      size = int(np.prod(shape))
      entries.append(Entry('seed_update/%s/%s' % (scope, kind), shape, offset,
                           size))
      count += size
      offset = -(-(offset + size) // ALIGN) * ALIGN
  return Layout(tuple(entries), offset, count)


def pack(variables, layout: Layout, fill: float = 0.0) -> np.ndarray:
  """{name: array} -> the flat f32 arena; pads hold `fill`."""
  flat = np.full((layout.total,), fill, np.float32)
  for e in layout.entries:
    a = np.asarray(variables[e.name], dtype=np.float32)
    if tuple(a.shape) != tuple(e.shape):
      raise ValueError('%s: shape %r, expected %r' % (e.name, a.shape, e.shape))
    flat[e.offset:e.offset + e.size] = a.reshape(-1)
  return flat


def unpack(flat, layout: Layout):
  """The flat arena -> {name: array in the checkpoint's shape} (copies)."""
  flat = np.asarray(flat)
  if flat.shape != (layout.total,):
    raise ValueError('arena of shape %r, expected (%d,)' %
                     (flat.shape, layout.total))
  return {e.name: flat[e.offset:e.offset + e.size].reshape(e.shape).copy()
          for e in layout.entries}
