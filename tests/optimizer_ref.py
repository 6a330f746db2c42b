"""Oracle for the optimizer unit (include/ffn_optimizer.h,
ffn_amd/training/optimizer.py): the header's table and the learning-rate
schedule restated in numpy, one numpy operation per written operation.

Every function takes a dtype.  With np.float32 the arrays and every
coefficient are f32 and each numpy operation rounds once, so the result is the
definition's, bit for bit (numpy never contracts a product and a sum, and its
f32 sqrt and divide are the correctly rounded ones).  With np.float64 the same
operations are the yardstick for the f32 run.

The five forms are TensorFlow 1's documented ApplyGradientDescent,
ApplyMomentum (no Nesterov), ApplyAdagrad, ApplyAdam and ApplyRMSProp, written
from the documentation; TensorFlow is not a dependency and nothing here is
pinned to its bits.
"""

import numpy as np

RULES = ('sgd', 'momentum', 'adagrad', 'adam', 'rmsprop')
SLOT_INIT = {'sgd': (), 'momentum': (0.0,), 'adagrad': (0.1,),
             'adam': (0.0, 0.0), 'rmsprop': (1.0, 0.0)}

DEFAULTS = dict(optimizer='sgd', learning_rate=0.001, momentum=0.9,
                learning_rate_decay_factor=None, decay_steps=None,
                rmsprop_decay=0.9, adam_beta1=0.9, adam_beta2=0.999,
                epsilon=1e-8, max_gradient_entry_mag=0.7)


def clip_gradient(g, clip):
  """g < -clip -> -clip, g > clip -> clip; clip <= 0: no clip."""
  if not clip > 0:
    return g
  g = np.where(g < -clip, -clip, g)
  return np.where(g > clip, clip, g)


def apply(rule, p, g, slots, lr, clip, c0, c1, eps, dtype=np.float32):
  """One update.  p, g and the slots are arrays; returns (p, slots) as new
  arrays of `dtype`.  lr, clip, c0, c1, eps are rounded to `dtype` first."""
  t = dtype
  p, g = np.asarray(p, t), np.asarray(g, t)
  slots = [np.asarray(s, t) for s in slots]
  lr, clip, c0, c1, eps = t(lr), t(clip), t(c0), t(c1), t(eps)
  assert len(slots) == len(SLOT_INIT[rule]), rule
  with np.errstate(all='ignore'):
    g = clip_gradient(g, clip).astype(t)
    if rule == 'sgd':
      u = lr * g
      p = p - u
      out = []
    elif rule == 'momentum':
      a, = slots
      u = a * c0
      a = u + g
      u = a * lr
      p = p - u
      out = [a]
    elif rule == 'adagrad':
      a, = slots
      gg = g * g
      a = a + gg
      u = lr * g
      s = np.sqrt(a)
      u = u / s
      p = p - u
      out = [a]
    elif rule == 'adam':
      m, v = slots
      d = g - m
      d = d * c0
      m = m + d
      gg = g * g
      e = gg - v
      e = e * c1
      v = v + e
      u = m * lr
      s = np.sqrt(v)
      s = s + eps
      u = u / s
      p = p - u
      out = [m, v]
    elif rule == 'rmsprop':
      ms, mom = slots
      gg = g * g
      e = gg - ms
      e = e * c0
      ms = ms + e
      bm = mom * c1
      u = g * lr
      r = ms + eps
      s = np.sqrt(r)
      u = u / s
      mom = bm + u
      p = p - mom
      out = [ms, mom]
    else:
      raise ValueError(rule)
  assert p.dtype == t and all(s.dtype == t for s in out)
  return p, out


def learning_rate_at(cfg, step, dtype=np.float32):
  t = dtype
  lr0 = t(cfg['learning_rate'])
  if cfg['learning_rate_decay_factor'] is None or cfg['decay_steps'] is None:
    return lr0
  k = t(int(step) // int(cfg['decay_steps']))
  return t(lr0 * t(cfg['learning_rate_decay_factor']) ** k)


def coefficients(cfg, step, b1p, b2p, dtype=np.float32):
  """(lr, c0, c1, eps) of `apply` at global_step `step`; b1p, b2p are adam's
  beta powers before the step."""
  t = dtype
  one = t(1)
  lr = learning_rate_at(cfg, step, t)
  c0 = c1 = t(0)
  rule = cfg['optimizer']
  if rule == 'momentum':
    c0 = t(cfg['momentum'])
  elif rule == 'adam':
    c0 = t(one - t(cfg['adam_beta1']))
    c1 = t(one - t(cfg['adam_beta2']))
    lr = t(t(lr * np.sqrt(t(one - t(b2p)))) / t(one - t(b1p)))
  elif rule == 'rmsprop':
    c0 = t(one - t(cfg['rmsprop_decay']))
    c1 = t(cfg['momentum'])
  return lr, c0, c1, t(cfg['epsilon'])


class Optimizer:
  """The state a trainer keeps besides the variables: slots, step counter,
  adam's beta powers.  `step(p, g)` works on one array or on a dict of arrays
  (slots are then dicts too)."""

  def __init__(self, dtype=np.float32, **flags):
    unknown = set(flags) - set(DEFAULTS)
    assert not unknown, unknown
    self.cfg = dict(DEFAULTS, **flags)
    self.dtype = dtype
    self.rule = self.cfg['optimizer']
    self.global_step = 0
    self.b1p = dtype(self.cfg['adam_beta1'])
    self.b2p = dtype(self.cfg['adam_beta2'])
    self.slots = None

  def _init_slots(self, p):
    return [np.full(np.shape(p), init, self.dtype)
            for init in SLOT_INIT[self.rule]]

  def step(self, p, g):
    t = self.dtype
    lr, c0, c1, eps = coefficients(self.cfg, self.global_step, self.b1p,
                                   self.b2p, t)
    clip = self.cfg['max_gradient_entry_mag']
    if isinstance(p, dict):
      if self.slots is None:
        self.slots = {k: self._init_slots(v) for k, v in p.items()}
      new = {}
      for k in p:
        new[k], self.slots[k] = apply(self.rule, p[k], g[k], self.slots[k], lr,
                                      clip, c0, c1, eps, t)
    else:
      if self.slots is None:
        self.slots = self._init_slots(p)
      new, self.slots = apply(self.rule, p, g, self.slots, lr, clip, c0, c1,
                              eps, t)
    self.global_step += 1
    if self.rule == 'adam':
      self.b1p = t(self.b1p * t(self.cfg['adam_beta1']))
      self.b2p = t(self.b2p * t(self.cfg['adam_beta2']))
    return new
