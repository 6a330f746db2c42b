"""The optimizer's host side without a GPU: the numpy oracle
(tests/optimizer_ref.py) against independent restatements, the learning-rate
schedule, OptimizerConfig's validation and the arena layout
(ffn_amd/training/optimizer.py)."""

import numpy as np
import pytest

from ffn_amd import _lib
from ffn_amd.training import optimizer as opt
from tests import gradients_ref
from tests import optimizer_ref as ref

EPS32 = 2.0 ** -24


def f32_flags(**flags):
  """Flags whose values are f32 numbers, so that the f32 and the f64 run of
  the oracle start from the same constants and differ in arithmetic only."""
  return {k: float(np.float32(v)) if isinstance(v, float) else v
          for k, v in flags.items()}


def random_case(seed, count=4000):
  rng = np.random.RandomState(seed)
  p = rng.normal(0, 0.05, count).astype(np.float32)
  gs = [rng.normal(0, 0.5, count).astype(np.float32) for _ in range(5)]
  return p, gs


def test_the_module_agrees_with_the_oracle_on_names_and_slots():
  assert opt.RULES == ref.RULES
  assert opt.SLOT_INIT == ref.SLOT_INIT
  assert opt.OptimizerConfig().to_dict() == ref.DEFAULTS


@pytest.mark.parametrize('rule', ref.RULES)
def test_f32_oracle_stays_within_a_few_ulps_of_its_f64_run(rule):
  """Five steps at lr 0.01 on p ~ N(0, 0.05), g ~ N(0, 0.5) clipped to 0.7.
  Bound: an update |u| stays below 0.15 max|p| here; a step rounds p once
  (2^-24 max|p|) and u carries at most 32 roundings of its chain and of the
  slots' five steps (32 x 2^-24 x 0.15 max|p|): under 6 x 2^-24 max|p| a step,
  32 x 2^-24 over five.  A slot rounds at most three times a step.
  Adam adds the cancellation in its f32 beta2 power: 1 - beta2^t has a relative
  error of up to 2^-24 / (t (1 - beta2)) = 1000 / t x 2^-24 from step 2 on (step
  1 is exact), the square root halves it, and |u| is about lr = 0.05 max|p|:
  25 / t x 2^-24 max|p| a step, 25 (1/2 + 1/3 + 1/4 + 1/5) = 32 x 2^-24 more."""
  flags = f32_flags(optimizer=rule, learning_rate=0.01, momentum=0.9,
                    rmsprop_decay=0.9, adam_beta1=0.9, adam_beta2=0.999,
                    epsilon=1e-8, max_gradient_entry_mag=0.7)
  p, gs = random_case(1)
  o32, o64 = ref.Optimizer(np.float32, **flags), ref.Optimizer(np.float64,
                                                               **flags)
  p32, p64 = p, p.astype(np.float64)
  for g in gs:
    p32, p64 = o32.step(p32, g), o64.step(p64, g.astype(np.float64))
  assert p32.dtype == np.float32 and p64.dtype == np.float64
  e = float(np.max(np.abs(p32 - p64)) / np.max(np.abs(p64)))
  print('%s: max |p32 - p64| / max |p64| = %.3g = %.2f x 2^-24' %
        (rule, e, e / EPS32))
  assert e <= (64 if rule == 'adam' else 32) * EPS32
  assert np.max(np.abs(p64 - p)) > 1e-3  # and it moved
  for s32, s64 in zip(o32.slots, o64.slots):
    es = float(np.max(np.abs(s32 - s64)) / np.max(np.abs(s64)))
    print('%s: slot %.2f x 2^-24' % (rule, es / EPS32))
    assert es <= 32 * EPS32


@pytest.mark.parametrize('rule', ['sgd', 'momentum'])
def test_sgd_and_momentum_equal_torch_sgd_in_f64(rule):
  """Only these two rules have the same form in torch: torch.optim.SGD with
  momentum mu and dampening 0 keeps buf = mu buf + g and steps p -= lr buf,
  which is the table's momentum rule (and sgd with mu = 0).  torch's Adam,
  Adagrad and RMSprop place epsilon and the bias correction differently and
  start their accumulators elsewhere, so they are no oracle for the other
  three."""
  import torch
  p, gs = random_case(2, 500)
  clip = 0.7
  o = ref.Optimizer(np.float64, optimizer=rule, learning_rate=0.01,
                    momentum=0.9, max_gradient_entry_mag=clip)
  tp = torch.tensor(p.astype(np.float64), requires_grad=True)
  sgd = torch.optim.SGD([tp], lr=0.01, dampening=0,
                        momentum=0.9 if rule == 'momentum' else 0.0)
  mine = p.astype(np.float64)
  for g in gs:
    mine = o.step(mine, g.astype(np.float64))
    tp.grad = torch.tensor(np.clip(g.astype(np.float64), -clip, clip))
    sgd.step()
  # f64 rounding: torch may fuse or reorder lr * buf; 5 steps of |u| < 0.1
  assert np.max(np.abs(mine - tp.detach().numpy())) <= 5 * 0.1 * 2.0 ** -52


def scalar_loop(rule, p, gs, lr, clip, mom, decay, b1, b2, eps):
  """The rules element by element in Python floats (f64), as one would write
  them from the optimizers' documentation."""
  out = []
  for i in range(len(p)):
    x = float(p[i])
    acc, m, v, ms, mo = 0.1, 0.0, 0.0, 1.0, 0.0
    for t, garr in enumerate(gs, start=1):
      g = float(garr[i])
      if clip > 0:
        g = min(max(g, -clip), clip)
      if rule == 'adagrad':
        acc += g * g
        x -= lr * g / acc ** 0.5
      elif rule == 'adam':
        alpha = lr * (1 - b2 ** t) ** 0.5 / (1 - b1 ** t)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        x -= alpha * m / (v ** 0.5 + eps)
      else:
        ms = decay * ms + (1 - decay) * g * g
        mo = mom * mo + lr * g / (ms + eps) ** 0.5
        x -= mo
    out.append(x)
  return np.array(out)


@pytest.mark.parametrize('eps', [1e-8, 1e-3])
@pytest.mark.parametrize('rule', ['adagrad', 'adam', 'rmsprop'])
def test_adam_adagrad_rmsprop_against_scalar_loops(rule, eps):
  p, gs = random_case(3, 200)
  lr, clip, mom, decay, b1, b2 = 0.01, 0.7, 0.9, 0.9, 0.9, 0.999
  o = ref.Optimizer(np.float64, optimizer=rule, learning_rate=lr, momentum=mom,
                    rmsprop_decay=decay, adam_beta1=b1, adam_beta2=b2,
                    epsilon=eps, max_gradient_entry_mag=clip)
  mine = p.astype(np.float64)
  for g in gs:
    mine = o.step(mine, g.astype(np.float64))
  want = scalar_loop(rule, p, gs, lr, clip, mom, decay, b1, b2, eps)
  # the loops write b m + (1 - b) g where the table writes m + (g - m)(1 - b):
  # equal up to f64 rounding of a few operations a step
  assert np.max(np.abs(mine - want)) <= 1e-12
  assert np.max(np.abs(want - p)) > 1e-3


def test_adam_moves_by_about_lr_a_step_under_a_constant_gradient():
  lr = 0.001
  for dtype in (np.float32, np.float64):
    o = ref.Optimizer(dtype, optimizer='adam', learning_rate=lr)
    p = np.zeros(3, dtype)
    g = np.array([0.3, -0.3, 0.01], dtype)
    for k in range(1, 6):
      p = o.step(p, g)
      # m_hat / sqrt(v_hat) = sign(g) for a constant g, up to epsilon
      assert np.allclose(p, -np.sign(g) * lr * k, rtol=1e-4, atol=0)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_clip_at_the_bound_beyond_it_and_off(dtype):
  above = np.nextafter(np.float32(0.7), np.float32(1))  # 0.70000005
  g = np.array([0.7, -0.7, above, -above, 3.0, -3.0, 0.0, -0.0, 0.2],
               np.float32).astype(dtype)
  c = dtype(np.float32(0.7))
  got = ref.clip_gradient(g, c)
  want = np.array([c, -c, c, -c, c, -c, 0.0, -0.0, dtype(np.float32(0.2))],
                  dtype)
  assert np.array_equal(got, want)
  assert np.array_equal(np.signbit(got), np.signbit(want))
  assert ref.clip_gradient(g, dtype(0)) is g
  # through apply: sgd with lr 1 moves p = 0 to -clip(g)
  p, _ = ref.apply('sgd', np.zeros_like(g), g, [], 1.0, c, 0, 0, 0, dtype)
  assert np.array_equal(p, -want)
  p, _ = ref.apply('sgd', np.zeros_like(g), g, [], 1.0, 0.0, 0, 0, 0, dtype)
  assert np.array_equal(p, -g)


def test_learning_rate_schedule():
  cfg = opt.OptimizerConfig(learning_rate=0.003)
  for step in (0, 1, 7, 10 ** 6):
    lr = cfg.learning_rate_at(step)
    assert type(lr) is np.float32 and lr == np.float32(0.003)
  # both decay values are needed
  assert opt.OptimizerConfig(learning_rate=0.003, decay_steps=2
                             ).learning_rate_at(9) == np.float32(0.003)
  cfg = opt.OptimizerConfig(learning_rate=0.003, decay_steps=2,
                            learning_rate_decay_factor=0.5)
  lr0 = np.float32(0.003)
  want = [lr0, lr0, lr0 / 2, lr0 / 2, lr0 / 4]
  got = [cfg.learning_rate_at(s) for s in range(5)]
  assert got == want
  assert all(type(v) is np.float32 for v in got)
  flags = cfg.to_dict()
  assert [ref.learning_rate_at(flags, s) for s in range(5)] == want


@pytest.mark.parametrize('rule', ref.RULES)
def test_config_coefficients_equal_the_oracles(rule):
  cfg = opt.OptimizerConfig(optimizer=rule, learning_rate=0.002, decay_steps=3,
                            learning_rate_decay_factor=0.7, epsilon=1e-3)
  b1p, b2p = cfg.initial_powers()
  o = ref.Optimizer(np.float32, **cfg.to_dict())
  for step in range(7):
    got = cfg.coefficients(step, b1p, b2p)
    want = ref.coefficients(o.cfg, step, o.b1p, o.b2p, np.float32)
    assert all(type(v) is np.float32 for v in got)
    assert [v.tobytes() for v in got] == [v.tobytes() for v in want]
    b1p, b2p = cfg.advance_powers(b1p, b2p)
    o.b1p = np.float32(o.b1p * np.float32(o.cfg['adam_beta1']))
    o.b2p = np.float32(o.b2p * np.float32(o.cfg['adam_beta2']))


@pytest.mark.parametrize('flags', [
    dict(optimizer='lion'), dict(learning_rate=0.0), dict(learning_rate=-1.0),
    dict(learning_rate=float('nan')), dict(adam_beta1=1.0),
    dict(adam_beta2=-0.1), dict(adam_beta2=1.0), dict(momentum=1.0),
    dict(rmsprop_decay=1.5), dict(decay_steps=0), dict(decay_steps=-3),
    dict(decay_steps=2.5), dict(learning_rate_decay_factor=0.0),
    dict(epsilon=0.0), dict(max_gradient_entry_mag=-0.7)])
def test_config_refuses(flags):
  with pytest.raises(ValueError):
    opt.OptimizerConfig(**flags)


def test_config_round_trip():
  cfg = opt.OptimizerConfig(optimizer='adam', decay_steps=5,
                            learning_rate_decay_factor=0.9)
  assert opt.OptimizerConfig.from_dict(cfg.to_dict()) == cfg
  assert cfg.rule == 3 and cfg.num_slots == 2
  assert opt.OptimizerConfig().rule == 0 and opt.OptimizerConfig().num_slots == 0


@pytest.mark.parametrize('depth', [2, 3, 12])
def test_arena_layout(depth):
  from ffn_amd.training.models import convstack_3d
  layout = opt.arena_layout(depth)
  names = [e.name for e in layout.entries]
  want = []
  for scope in convstack_3d.conv_scopes(depth):
    want += ['seed_update/%s/weights' % scope, 'seed_update/%s/biases' % scope]
  assert names == want
  end = 0
  for e in layout.entries:
    assert e.offset % 4 == 0, e
    assert e.offset >= end, e           # no overlap
    assert e.offset - end < 4, e        # and no more pad than alignment needs
    assert e.size == int(np.prod(e.shape))
    end = e.offset + e.size
  assert layout.total % 4 == 0 and 0 <= layout.total - end < 4
  count = 27 * 2 * 32 + 32 + (2 * depth - 1) * (27 * 32 * 32 + 32) + 33
  assert layout.count == count == sum(e.size for e in layout.entries)
  if depth == 12:
    assert layout.count == 638433
    assert layout.count == _lib.load().ffn_engine_weight_count(12, 32)
    # only conv_lom's single bias leaves a pad
    assert layout.total == 638433 + 3
  variables = gradients_ref.random_variables(depth, seed=5)
  flat = opt.pack(variables, layout, fill=7.0)
  assert flat.dtype == np.float32 and flat.shape == (layout.total,)
  covered = np.zeros(layout.total, bool)
  for e in layout.entries:
    covered[e.offset:e.offset + e.size] = True
  assert np.all(flat[~covered] == 7.0)
  back = opt.unpack(flat, layout)
  assert sorted(back) == sorted(variables)
  for k, v in variables.items():
    assert back[k].shape == v.shape and np.array_equal(back[k], v), k
  with pytest.raises(ValueError):
    opt.unpack(flat[:-1], layout)
  bad = dict(variables)
  bad[names[0]] = bad[names[0]][..., :1]
  with pytest.raises(ValueError):
    opt.pack(bad, layout)


def test_no_cpu_fallback_without_gpu():
  import torch
  if torch.cuda.is_available():
    pytest.skip('GPU present')
  from ffn_amd.training import trainer
  from ffn_amd.training.models import convstack_3d
  with pytest.raises(_lib.FFNHipError):
    opt.OptimizerOps()
  m = convstack_3d.ConvStack3DFFNModel(fov_size=[9, 7, 5], deltas=[1, 1, 1],
                                       depth=3)
  m.set_variables(gradients_ref.random_variables(3, seed=5))
  with pytest.raises(_lib.FFNHipError):
    trainer.ConvStackTrainer(m, opt.OptimizerConfig(), max_batch=2)
