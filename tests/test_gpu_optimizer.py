"""The optimizer unit and ConvStackTrainer on the GPU (include/ffn_optimizer.h,
ffn_amd/training/optimizer.py, ffn_amd/training/trainer.py) against the numpy
oracle (tests/optimizer_ref.py).

The update is elementwise with every operation rounded on its own, so the
relation to the oracle's f32 run is equality of bits, not a tolerance.  Whether
the gradients are right is tests/test_gpu_gradients.py's business; here the
trainer's gradients are compared, for equality, with a separate
ConvStackGradients on the same variables.
"""
import ctypes

import numpy as np
import pytest

from tests import gradients_ref as gref
from tests import optimizer_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG = -1
GUARD = 64
COUNTS = [1, 3, 4, 5, 255, 1029, 638433]
ABOVE = np.nextafter(np.float32(0.7), np.float32(1))  # 0.70000005
PLANTED = np.array([0.7, -0.7, ABOVE, -ABOVE, 0.0, -0.0, 1e-41], np.float32)
F32 = np.float32
# rule -> (c0, c1) as the trainer computes them at the reference's defaults
COEF = {'sgd': (F32(0), F32(0)), 'momentum': (F32(0.9), F32(0)),
        'adagrad': (F32(0), F32(0)),
        'adam': (F32(1) - F32(0.9), F32(1) - F32(0.999)),
        'rmsprop': (F32(1) - F32(0.9), F32(0.9))}
APPLY_CASES = [(rule, eps) for rule in ref.RULES
               for eps in ((1e-8, 1e-3) if rule in ('adam', 'rmsprop')
                           else (1e-8,))]


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


def guarded(torch, values):
  """`values` on the device with GUARD NaNs behind them."""
  host = np.full(len(values) + GUARD, np.nan, np.float32)
  host[:len(values)] = values
  t = torch.from_numpy(host).to('cuda:0')
  torch.cuda.synchronize()
  assert t.data_ptr() % 16 == 0
  return t


def split(t, count):
  host = t.cpu().numpy()
  return host[:count], host[count:]


def apply_inputs(count, seed):
  """p ~ N(0, 0.05); three gradients ~ N(0, 0.5) (one entry in six beyond the
  clip) with the planted values at the front and, from the back, in the tail
  elements."""
  rng = np.random.RandomState(seed)
  p = rng.normal(0, 0.05, count).astype(np.float32)
  gs = []
  for k in range(3):
    g = rng.normal(0, 0.5, count).astype(np.float32)
    planted = np.roll(PLANTED, k)
    m = min(count, len(planted))
    g[:m] = planted[:m]
    if count > 2 * len(planted):
      g[-len(planted):] = planted[::-1]
    gs.append(g)
  return p, gs


# -- 1. apply -----------------------------------------------------------------
def run_apply(ops, torch, rule, eps, count, p, gs, lr, clip):
  c0, c1 = COEF[rule]
  pd = guarded(torch, p)
  slots_d = [guarded(torch, np.full(count, init, np.float32))
             for init in ref.SLOT_INIT[rule]]
  steps = []
  for g in gs:
    gd = guarded(torch, g)
    ops.apply(rule, count, pd, gd, *slots_d, lr=lr, clip=clip, c0=c0, c1=c1,
              eps=eps)
    got_p, guard_p = split(pd, count)
    assert np.all(np.isnan(guard_p))
    got_slots = []
    for sd in slots_d:
      s, guard_s = split(sd, count)
      assert np.all(np.isnan(guard_s))
      got_slots.append(s)
    got_g, guard_g = split(gd, count)
    assert same_bits(got_g, g) and np.all(np.isnan(guard_g))
    steps.append((got_p, got_slots))
  return steps


@pytest.mark.parametrize('count', COUNTS)
@pytest.mark.parametrize('rule,eps', APPLY_CASES)
def test_apply_equals_the_oracle_bit_for_bit(ops, torch, rule, eps, count):
  lr, clip = F32(0.01), F32(0.7)
  c0, c1 = COEF[rule]
  p, gs = apply_inputs(count, seed=count)
  first = run_apply(ops, torch, rule, eps, count, p, gs, lr, clip)
  again = run_apply(ops, torch, rule, eps, count, p, gs, lr, clip)
  want_p = p
  want_slots = [np.full(count, init, np.float32)
                for init in ref.SLOT_INIT[rule]]
  for k, g in enumerate(gs):
    want_p, want_slots = ref.apply(rule, want_p, g, want_slots, lr, clip, c0,
                                   c1, eps, np.float32)
    got_p, got_slots = first[k]
    differ = np.flatnonzero(bits(got_p) != bits(want_p))
    assert differ.size == 0, (k, differ[:8], got_p[differ[:8]],
                              want_p[differ[:8]], g[differ[:8]])
    for j, (got, want) in enumerate(zip(got_slots, want_slots)):
      differ = np.flatnonzero(bits(got) != bits(want))
      assert differ.size == 0, (k, j, differ[:8], got[differ[:8]],
                                want[differ[:8]], g[differ[:8]])
    assert same_bits(again[k][0], got_p)
    assert all(same_bits(a, b) for a, b in zip(again[k][1], got_slots))
  assert np.all(np.isfinite(want_p))
  assert not same_bits(want_p, p)


def test_apply_without_clip(ops, torch):
  count = 1029
  p, gs = apply_inputs(count, seed=7)
  got = run_apply(ops, torch, 'sgd', 1e-8, count, p, gs[:1], F32(0.01), 0.0)
  want, _ = ref.apply('sgd', p, gs[0], [], F32(0.01), 0.0, 0, 0, 0, np.float32)
  assert same_bits(got[0][0], want)
  clipped, _ = ref.apply('sgd', p, gs[0], [], F32(0.01), F32(0.7), 0, 0, 0,
                         np.float32)
  assert not same_bits(want, clipped)


# -- 2. grad_stats ------------------------------------------------------------
@pytest.mark.parametrize('clip', [0.7, 0.0])
@pytest.mark.parametrize('count', [5, 1029, 638433])
def test_grad_stats(ops, torch, count, clip):
  """Count 5 holds 3.5, NaN, +inf, -inf and 0.7; the larger ones also -0.7,
  and 3.5 in the last element (the scalar tail)."""
  rng = np.random.RandomState(count)
  g = np.clip(rng.normal(0, 0.5, count), -3, 3).astype(np.float32)
  planted = np.array([3.5, np.nan, np.inf, -np.inf, 0.7, -0.7], np.float32)
  m = min(count, len(planted))
  g[:m] = planted[:m]
  if count > 5:
    g[-1] = 3.5
    g[count // 2] = np.nan
  finite = np.isfinite(g)
  want_clipped = int(np.sum(np.abs(g[finite]) > F32(clip))) if clip > 0 else 0
  want_bad = int(np.sum(~finite))
  assert want_bad == (3 if count == 5 else 4)
  if clip > 0 and count > 5:
    # about one entry in six; +-0.7 themselves are not among them
    assert 0.1 * count < want_clipped < 0.25 * count
    assert want_clipped == int(np.sum(np.abs(g[finite]) >= F32(clip))) - 2
  gd = guarded(torch, g)
  for _ in range(2):
    max_abs, clipped, bad = ops.grad_stats(count, gd, clip)
    assert (max_abs, clipped, bad) == (3.5, want_clipped, want_bad)
  got_g, guard = split(gd, count)
  assert same_bits(got_g, g) and np.all(np.isnan(guard))
  timing = ops.last_timing()
  assert set(timing) == {'grad_stats', 'apply'} and timing['grad_stats'] > 0


def test_grad_stats_of_nothing_finite(ops, torch):
  gd = guarded(torch, np.array([np.nan, np.inf, -np.inf], np.float32))
  assert ops.grad_stats(3, gd, 0.7) == (0.0, 0, 3)


# -- 3. validation ------------------------------------------------------------
def test_bad_arguments_launch_nothing(ops, torch):
  count = 64
  nan = lambda: torch.full((count + 4,), np.nan, dtype=torch.float32,
                           device='cuda:0')
  p, g, s0, s1 = nan(), nan(), nan(), nan()
  torch.cuda.synchronize()
  lib, h = ops._lib, ops._h
  P = lambda t, off=0: ctypes.c_void_p(0 if t is None else t.data_ptr() + off)
  slots_of = {0: (None, None), 1: (s0, None), 2: (s0, None), 3: (s0, s1),
              4: (s0, s1)}

  def apply(rule=3, n=count, params=P(p), grads=P(g), slots=None):
    a, b = slots if slots is not None else [
        P(t) for t in slots_of.get(rule, (s0, s1))]
    return lib.ffn_optimizer_apply(h, rule, n, params, grads, a, b, 0.01, 0.7,
                                   0.1, 0.001, 1e-8)

  assert apply(params=P(None)) == ERR_ARG
  assert apply(grads=P(None)) == ERR_ARG
  for rule in range(5):
    a, b = slots_of[rule]
    if a is None:
      assert apply(rule, slots=(P(s0), P(None))) == ERR_ARG  # superfluous
    else:
      assert apply(rule, slots=(P(None), P(b))) == ERR_ARG   # missing
    if b is None:
      assert apply(rule, slots=(P(a), P(s1))) == ERR_ARG     # superfluous
    else:
      assert apply(rule, slots=(P(a), P(None))) == ERR_ARG   # missing
  assert apply(n=0) == ERR_ARG
  assert apply(n=-4) == ERR_ARG
  assert apply(n=2 ** 31) == ERR_ARG
  assert apply(rule=5) == ERR_ARG
  assert apply(rule=-1) == ERR_ARG
  assert apply(params=P(p, 4)) == ERR_ARG
  assert apply(grads=P(g, 4)) == ERR_ARG
  assert apply(slots=(P(s0, 4), P(s1))) == ERR_ARG
  assert apply(slots=(P(s0), P(s1, 4))) == ERR_ARG
  assert apply(grads=P(p)) == ERR_ARG       # params overlapping grads
  assert apply(grads=P(p, 16)) == ERR_ARG   # partly
  assert apply(slots=(P(s0), P(s0))) == ERR_ARG
  assert lib.ffn_optimizer_apply(None, 0, count, P(p), P(g), P(None), P(None),
                                 0.01, 0.7, 0.0, 0.0, 0.0) == ERR_ARG
  assert lib.ffn_optimizer_apply(h, 0, count, P(p), P(g), P(None), P(None),
                                 float('inf'), 0.7, 0.0, 0.0, 0.0) == ERR_ARG

  canary = -12345.0
  mx = ctypes.c_float(canary)
  n_clip, n_bad = ctypes.c_uint64(77), ctypes.c_uint64(77)

  def stats(n=count, grads=P(g), out=ctypes.byref(mx)):
    return lib.ffn_optimizer_grad_stats(h, n, grads, 0.7, out,
                                        ctypes.byref(n_clip),
                                        ctypes.byref(n_bad))

  assert stats(n=0) == ERR_ARG
  assert stats(grads=P(None)) == ERR_ARG
  assert stats(grads=P(g, 4)) == ERR_ARG
  assert stats(out=None) == ERR_ARG
  assert lib.ffn_last_error()
  assert (mx.value, n_clip.value, n_bad.value) == (canary, 77, 77)
  torch.cuda.synchronize()
  for t in (p, g, s0, s1):
    assert np.all(np.isnan(t.cpu().numpy()))
  # and the same handle still works
  assert stats() == 0 and n_bad.value == count


# -- 4. the trainer -----------------------------------------------------------
def make_model(variables, depth, zyx):
  from ffn_amd.training.models import convstack_3d
  m = convstack_3d.ConvStack3DFFNModel(fov_size=list(zyx[::-1]),
                                       deltas=[1, 1, 1], depth=depth)
  m.set_variables(variables)
  return m


ZYX = (5, 7, 9)
TRAINER_CASES = {'depth3': (3, 2, 33), 'fib25': (12, 1, 32)}


def case_variables(name, fib25_variables):
  if name == 'fib25':
    return fib25_variables
  return gref.random_variables(3, seed=21, stddev=0.05)


@pytest.fixture(scope='module')
def separate_gradients(fib25_variables):
  """name -> a ConvStackGradients of its own (the parent commit's path: own
  buffers, variables uploaded), shared by the rules."""
  from ffn_amd.training import gradients
  made = {}

  def get(name):
    if name not in made:
      depth, n, _ = TRAINER_CASES[name]
      made[name] = gradients.ConvStackGradients(
          make_model(case_variables(name, fib25_variables), depth, ZYX), n, 0)
    return made[name]
  yield get
  for csg in made.values():
    csg.close()


def assert_same_dict(got, want, what):
  assert sorted(got) == sorted(want), what
  for k in want:
    assert same_bits(got[k], want[k]), (what, k)


@pytest.mark.parametrize('rule', ref.RULES)
@pytest.mark.parametrize('name', sorted(TRAINER_CASES))
def test_trainer_composes_gradients_and_update(opt, tr, separate_gradients,
                                               fib25_variables, name, rule):
  depth, n, seed = TRAINER_CASES[name]
  variables = case_variables(name, fib25_variables)
  inputs = gref.training_inputs(n, ZYX, seed=seed)
  cfg = opt.OptimizerConfig(optimizer=rule, decay_steps=2,
                            learning_rate_decay_factor=0.5)
  trainer = tr.ConvStackTrainer(make_model(variables, depth, ZYX), cfg,
                                max_batch=n, device_id=0)
  csg = separate_gradients(name)
  oracle = ref.Optimizer(np.float32, **cfg.to_dict())
  lr0 = np.float32(0.001)
  staircase = [lr0, lr0, lr0 / 2]
  try:
    before = trainer.variables()
    assert_same_dict(before, variables, 'initial variables')
    for k in range(3):
      loss, logits, step = trainer.train_step(*inputs)
      # (a) the kernels saw the current weights
      csg.set_variables(before)
      want_loss, want_logits, want_grads = csg.loss_and_gradients(*inputs)
      grads = trainer.gradients()
      assert_same_dict(grads, want_grads, 'gradients of step %d' % k)
      assert np.float32(loss).tobytes() == np.float32(want_loss).tobytes()
      assert isinstance(logits, np.ndarray) and same_bits(logits, want_logits)
      # (b) the update
      want = oracle.step(before, grads)
      after = trainer.variables()
      assert_same_dict(after, want, 'variables after step %d' % k)
      for j, got_slot in enumerate(trainer.slot_variables()):
        assert_same_dict(got_slot, {key: s[j] for key, s in
                                    oracle.slots.items()}, 'slot %d' % j)
      assert any(not same_bits(after[key], before[key]) for key in after)
      # (c) counter and schedule
      assert step == k + 1 == trainer.global_step
      stats = trainer.last_stats
      assert type(stats['learning_rate']) is np.float32
      assert stats['learning_rate'] == staircase[k]
      assert stats['loss'] == loss
      biggest = max(float(np.max(np.abs(g))) for g in grads.values())
      assert stats['max_abs'] == biggest
      assert stats['clipped'] == sum(
          int(np.sum(np.abs(g) > np.float32(0.7))) for g in grads.values())
      before = after
  finally:
    trainer.close()


# -- 5. refusal ---------------------------------------------------------------
def assert_same_state(got, want):
  assert_same_dict(got['variables'], want['variables'], 'variables')
  assert len(got['slots']) == len(want['slots'])
  for j, (a, b) in enumerate(zip(got['slots'], want['slots'])):
    assert_same_dict(a, b, 'slot %d' % j)
  assert got['global_step'] == want['global_step']
  for key in ('beta1_power', 'beta2_power'):
    assert np.float32(got[key]).tobytes() == np.float32(want[key]).tobytes()
  assert got['config'] == want['config']


def test_a_step_that_is_not_finite_is_refused(opt, tr, torch):
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  inputs = gref.training_inputs(2, ZYX, seed=33)
  trainer = tr.ConvStackTrainer(make_model(variables, 3, ZYX),
                                opt.OptimizerConfig(optimizer='adam'),
                                max_batch=2, device_id=0)
  try:
    trainer.train_step(*inputs)  # slots and powers away from their start
    # a NaN in the gradient arena's pad: no kernel of the gradient pass writes
    # there, so it is what grad_stats meets
    assert trainer.layout.total - trainer.layout.count == 3
    held = trainer.state()
    trainer.grads[-1] = float('nan')
    torch.cuda.synchronize()
    with pytest.raises(tr.InvalidLossError, match='Invalid loss detected'):
      trainer.train_step(*inputs)
    assert_same_state(trainer.state(), held)
    trainer.grads[-1] = 0.0
    torch.cuda.synchronize()
    # a loss that overflows
    bad = dict(held)
    bad['variables'] = dict(held['variables'])
    bad['variables']['seed_update/conv_lom/weights'] = np.full(
        (1, 1, 1, 32, 1), 1e38, np.float32)
    trainer.load_state(bad)
    held = trainer.state()
    assert_same_state(held, bad)
    with pytest.raises(tr.InvalidLossError, match='Invalid loss detected'):
      trainer.train_step(*inputs)
    assert_same_state(trainer.state(), held)
    assert trainer.global_step == 1
  finally:
    trainer.close()


# -- 6. resume ----------------------------------------------------------------
def test_resume_from_state(opt, tr):
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  inputs = gref.training_inputs(2, ZYX, seed=33)
  cfg = opt.OptimizerConfig(optimizer='adam', decay_steps=2,
                            learning_rate_decay_factor=0.5)
  model = make_model(variables, 3, ZYX)
  first = tr.ConvStackTrainer(model, cfg, max_batch=2, device_id=0)
  second = None
  try:
    first.train_step(*inputs)
    first.train_step(*inputs)
    state = first.state()
    second = tr.ConvStackTrainer(model, opt.OptimizerConfig(optimizer='adam'),
                                 max_batch=2, device_id=0)
    second.load_state(state)
    assert second.config == cfg
    loss1, logits1, step1 = first.train_step(*inputs)
    loss2, logits2, step2 = second.train_step(*inputs)
    assert step1 == step2 == 3
    assert np.float32(loss1).tobytes() == np.float32(loss2).tobytes()
    assert same_bits(logits1, logits2)
    assert_same_state(second.state(), first.state())
    assert second.last_stats == first.last_stats
    sgd = tr.ConvStackTrainer(model, opt.OptimizerConfig(), max_batch=2,
                              device_id=0)
    try:
      with pytest.raises(ValueError):
        sgd.load_state(state)
    finally:
      sgd.close()
  finally:
    first.close()
    if second is not None:
      second.close()


# -- 7. it learns -------------------------------------------------------------
LEARN_SEED = 51


def learn_inputs():
  seed, image, _, weights = gref.training_inputs(2, ZYX, seed=LEARN_SEED)
  labels = np.full((2,) + ZYX, 0.05, np.float32)
  labels[:, 1:4, 2:5, 3:6] = 0.95  # a centred 3^3 box
  return seed, image, labels, weights


def oracle_losses(rule, dtype):
  """The loss before each of ten steps and after the tenth, by gradients_ref
  and optimizer_ref on the CPU in `dtype`."""
  import torch
  tdt = torch.float32 if dtype == np.float32 else torch.float64
  variables = {k: v.astype(dtype) for k, v in
               gref.random_variables(3, seed=21, stddev=0.05).items()}
  o = ref.Optimizer(dtype, optimizer=rule)
  inputs = learn_inputs()
  out = []
  for _ in range(10):
    r = gref.run(variables, 3, *inputs, dtype=tdt)
    out.append(r['loss'])
    variables = o.step(variables, {k: np.asarray(g, dtype)
                                   for k, g in r['grads'].items()})
  out.append(gref.run(variables, 3, *inputs, dtype=tdt,
                      want_grads=False)['loss'])
  return out


@pytest.mark.parametrize('rule', ref.RULES)
def test_ten_steps_lower_the_loss(opt, tr, rule):
  """One fixed batch (depth 3, FoV (5, 7, 9), n = 2, labels 0.95 in a centred
  box), ten steps at the reference's default flags (learning rate 0.001 for
  every rule, input seed 51).  The oracle on the CPU, loss before the first
  step 0.437540501 (f32 and f64 agree to 3e-8), after the tenth:
    rule      f32          f64          decrease  |f32 - f64|
    sgd       0.431345582  0.431345554  0.0062    2.8e-08
    momentum  0.414505392  0.414505435  0.023     4.3e-08
    adagrad   0.422826678  0.422826716  0.015     3.8e-08
    adam      0.260950178  0.260873940  0.18      7.6e-05
    rmsprop   0.409730256  0.409730288  0.028     3.2e-08
  so every decrease is more than 2000 times the oracle's own f32 / f64
  difference.  (The last digit of the f32 column depends on the host's torch:
  adam read 0.260950148 on another.)  The GPU's final loss must lie within 4
  times that difference of the oracle's f32 final loss; measured on the
  MI355X: 0, 1.39 (momentum: 0.414505452), 0, 0.0004 and 0 times."""
  l32, l64 = oracle_losses(rule, np.float32), oracle_losses(rule, np.float64)
  own = abs(l32[-1] - l64[-1])
  assert l32[0] - l32[-1] >= 10 * own
  inputs = learn_inputs()
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  trainer = tr.ConvStackTrainer(make_model(variables, 3, ZYX),
                                opt.OptimizerConfig(optimizer=rule),
                                max_batch=2, device_id=0)
  try:
    losses = [trainer.train_step(*inputs)[0] for _ in range(10)]
    final, _ = trainer.csg.loss_and_gradients_device(*inputs)
  finally:
    trainer.close()
  losses.append(final)
  print('%s: oracle f32 %s' % (rule, ' '.join('%.9g' % v for v in l32)))
  print('%s: GPU        %s' % (rule, ' '.join('%.9g' % v for v in losses)))
  print('%s: final GPU %.9g, oracle f32 %.9g f64 %.9g; |GPU - f32| = %.3g = '
        '%.3g x |f32 - f64| (%.3g)' % (
            rule, final, l32[-1], l64[-1], abs(final - l32[-1]),
            abs(final - l32[-1]) / own, own))
  assert final < losses[0]
  assert abs(final - l32[-1]) <= 4 * own


# -- 8. no clip ---------------------------------------------------------------
def test_max_gradient_entry_mag_zero_applies_the_raw_gradient(opt, tr):
  variables = gref.random_variables(3, seed=21, stddev=0.05)
  seed, image, labels, weights = gref.training_inputs(2, ZYX, seed=33)
  weights = weights * np.float32(1000)  # gradients far beyond 0.7
  cfg = opt.OptimizerConfig(optimizer='momentum', max_gradient_entry_mag=0)
  trainer = tr.ConvStackTrainer(make_model(variables, 3, ZYX), cfg,
                                max_batch=2, device_id=0)
  try:
    trainer.train_step(seed, image, labels, weights)
    grads, after = trainer.gradients(), trainer.variables()
    stats = trainer.last_stats
  finally:
    trainer.close()
  assert stats['max_abs'] > 0.7 and stats['clipped'] == 0
  want = ref.Optimizer(np.float32, **cfg.to_dict()).step(variables, grads)
  assert_same_dict(after, want, 'unclipped')
  flags = dict(cfg.to_dict(), max_gradient_entry_mag=0.7)
  clipped = ref.Optimizer(np.float32, **flags).step(variables, grads)
  assert any(not same_bits(after[k], clipped[k]) for k in after)
