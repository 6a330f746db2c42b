"""fp16 inference (engine option mfma_products = 1, Runner(precision='fp16')): conv32m and
conv32mt keep the hi x hi MFMA product of every fp16 operand pair and drop the two
cross products that make the default path f32-accurate.

What is asserted: the option's semantics; on operands that ARE fp16 values the mode
computes what the f32 oracle computes, at the gate of the split kernels (1e-4), in every
family and batch form; the residual of an operand is really gone (weights that are not
representable, an activation below 2^-14); on the whole FIB-25 stack the GPU stands to
the mode's f64 definition (tests/half_ref.py, h64) as an f32 CPU restatement of it (h32)
does; back on three products nothing is left behind; the fp16 range guard still voids
and repeats on the exact kernel; the three FoV loops agree bit for bit with the mode on.

The smallest engine the split-product family runs on has depth 2 (its head is fused into
the last conv_b and the family needs depth >= 2), so the exact-operand cases use
conv0_a -> conv0_b -> conv1_a -> conv1_b + head with conv0_b and conv1_a a power of two
per channel on the centre tap (exact in, exact out) and conv1_b, the conv the head and
the residual are fused into, the dense one under test."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import half_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
FFN_OK, FFN_ERR_ARG = 0, -1
GATE = 1e-4  # the existing parity tests' gate for the split kernels (they measure <= 4.8e-6)
FOV33 = ((33, 33, 33), (8, 8, 8))
FOV_PERM = ((21, 41, 41), (5, 10, 10))  # laid out with permuted axes (rows of 21)


def _set(eng, name, value):
  return eng._lib.ffn_engine_set_option(eng._h, name.encode(), int(value))


def _get(eng, name):
  value = ctypes.c_int(-12345)
  rc = eng._lib.ffn_engine_get_option(eng._h, name.encode(), ctypes.byref(value))
  return rc, value.value


def _random_engine(depth, max_batch=1, fov=FOV33):
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  eng = hip_engine.HipEngine(fov[0], fov[1], depth, max_batch=max_batch)
  variables = ffn_oracle.random_weights(depth, seed=5, stddev=0.05)
  eng.set_weights(ffn_oracle.weights_blob(variables, depth))
  return eng


def _inputs(rng, n, fov=(33, 33, 33)):
  from oracle import ffn_oracle
  img = ((rng.randint(0, 256, (n,) + fov).astype(np.float32)) - 128) / 33
  seed = np.full((n,) + fov, ffn_oracle.f32_logit(0.05), np.float32)
  seed[:, fov[0] // 2, fov[1] // 2, fov[2] // 2] = ffn_oracle.f32_logit(0.95)
  seed[:, 4:14, 6:16, 2:18] += rng.normal(0, 1.5, (n, 10, 10, 16)).astype(np.float32)
  return img, seed


# ---------------------------------------------------------------------------
# 1. option semantics
# ---------------------------------------------------------------------------


def test_option_semantics():
  eng = _random_engine(3)
  plain = _random_engine(3)
  try:
    assert _get(eng, 'mfma_products') == (FFN_OK, 3)
    assert _set(eng, 'mfma_products', 1) == FFN_OK
    assert _get(eng, 'mfma_products') == (FFN_OK, 1)
    for bad in (0, 2, 4):
      assert _set(eng, 'mfma_products', bad) == FFN_ERR_ARG, bad
      assert _get(eng, 'mfma_products') == (FFN_OK, 1), bad  # a refused set stores nothing
    # a family without a one-product form ignores the option: the exact kernel's bits
    eng.set_option('conv_variant', 2)
    plain.set_option('conv_variant', 2)
    assert eng.get_option('mfma_products') == 1
    img, seed = _inputs(np.random.RandomState(4), 1)
    a, b = eng.predict(seed, img), plain.predict(seed, img)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # ... and M / MT do not: back on the default variant the logits move
    eng.set_option('conv_variant', 9)
    plain.set_option('conv_variant', 9)
    assert not np.array_equal(eng.predict(seed, img), plain.predict(seed, img))
  finally:
    eng.close()
    plain.close()


# ---------------------------------------------------------------------------
# 2. / 3. exact operands
# ---------------------------------------------------------------------------


def exact_variables(seed=7, representable=True, shifts=((-2, 1), (-1, 2), (-1, 1)),
                    w_std=0.05, lom_std=0.05):
  """Depth-2 variables whose 32 -> 32 convs see only fp16-representable operands for an
  image of multiples of 2^-6 in [-4, 4):
    conv0_a  the centre tap of the image channel times 2^p per output channel, no bias
             (the seed channel is not read): relu(2^p image), at most 9 significant bits;
    conv0_b, conv1_a  2^p per channel on the centre tap, no bias: exact in, exact out;
    conv1_b  dense; its weights rounded to fp16 by this function (representable) or left
             as f32 values (not), none in (0, 2^-14); f32 bias;
    conv_lom dense f32.
  shifts: [lo, hi) of p for conv0_a, conv0_b, conv1_a -- the smallest activation,
  2^-6 2^(sum of the lows), stays a normal fp16 number unless a test wants it otherwise."""
  from oracle import ffn_oracle
  rng = np.random.RandomState(seed)
  v = ffn_oracle.random_weights(2, seed=seed, stddev=w_std)
  w0 = np.zeros((3, 3, 3, 2, 32), np.float32)
  w0[1, 1, 1, 0, :] = 2.0 ** rng.randint(shifts[0][0], shifts[0][1], size=32)
  v['seed_update/conv0_a/weights'] = w0
  v['seed_update/conv0_a/biases'] = np.zeros(32, np.float32)
  for name, (lo, hi) in (('conv0_b', shifts[1]), ('conv1_a', shifts[2])):
    w = np.zeros((3, 3, 3, 32, 32), np.float32)
    w[1, 1, 1, np.arange(32), np.arange(32)] = 2.0 ** rng.randint(lo, hi, size=32)
    v['seed_update/%s/weights' % name] = w
    v['seed_update/%s/biases' % name] = np.zeros(32, np.float32)
  w = v['seed_update/conv1_b/weights']
  w[(np.abs(w) < half_ref.TINY)] = 0
  if representable:
    w = half_ref.hi_np(w)
  else:
    assert not np.array_equal(half_ref.hi_np(w), w)
  v['seed_update/conv1_b/weights'] = w
  v['seed_update/conv_lom/weights'] = rng.normal(0, lom_std, (1, 1, 1, 32, 1)).astype(
      np.float32)
  return v


def exact_images(n, fov, seed=11):
  rng = np.random.RandomState(seed)
  img = (rng.randint(-256, 256, size=(n,) + tuple(fov)) / 64.0).astype(np.float32)
  logits = rng.normal(0, 1, img.shape).astype(np.float32)
  return img, logits


def _exact_engine(variables, fov, max_batch):
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  eng = hip_engine.HipEngine(fov[0], fov[1], 2, max_batch=max_batch)
  eng.set_weights(ffn_oracle.weights_blob(variables, 2))
  eng.set_option('mfma_products', 1)
  return eng


@pytest.mark.parametrize('fov,max_batch,batches', [
    (FOV33, 4, (1, 3, 4)),   # MT (main and tail workgroups; 33^3 ends in a partial chunk),
                             # then M, ragged and full
    (FOV_PERM, 2, (1, 2)),   # the permuted layout
])
def test_exact_operands_meet_the_oracle(fov, max_batch, batches):
  from oracle import ffn_oracle
  variables = exact_variables()
  blob = ffn_oracle.weights_blob(variables, 2)
  img, seed = exact_images(max(batches), fov[0])
  want = ffn_oracle.forward(img, seed, blob, 2)
  eng = _exact_engine(variables, fov, max_batch)
  try:
    assert eng.get_option('conv_variant') in (8, 9)
    for n in batches:
      got = eng.predict(seed[:n], img[:n])
      err = float(np.abs(got - want[:n]).max())
      print('fov %s n %d: max|gpu - oracle| %.3g' % (fov[0], n, err))
      assert err <= GATE, (fov, n, err)
    assert eng.get_option('conv_variant') in (8, 9)  # (no step was voided)
  finally:
    eng.close()


@pytest.mark.parametrize('fov,max_batch,batches', [(FOV33, 4, (1, 3, 4)),
                                                   (FOV_PERM, 2, (1, 2))])
def test_the_weights_residual_is_gone(fov, max_batch, batches):
  """The same inputs with conv1_b weights that are NOT fp16 values: the result is the
  oracle's on hi(w), and misses the oracle's on w by more than the gate."""
  from oracle import ffn_oracle
  variables = exact_variables(representable=False, w_std=0.2, lom_std=0.2)
  on_hi = ffn_oracle.weights_blob(half_ref.hi_variables(variables, 2), 2)
  on_w = ffn_oracle.weights_blob(variables, 2)
  img, seed = exact_images(max(batches), fov[0])
  want_hi = ffn_oracle.forward(img, seed, on_hi, 2)
  want_w = ffn_oracle.forward(img, seed, on_w, 2)
  eng = _exact_engine(variables, fov, max_batch)
  try:
    for n in batches:
      got = eng.predict(seed[:n], img[:n])
      err_hi = float(np.abs(got - want_hi[:n]).max())
      err_w = float(np.abs(got - want_w[:n]).max())
      print('fov %s n %d: max|gpu - oracle(hi w)| %.3g, max|gpu - oracle(w)| %.3g' % (
          fov[0], n, err_hi, err_w))
      assert err_hi <= GATE, (fov, n, err_hi)
      assert err_w > GATE, (fov, n, err_w)
      # the three-product path on the same engine: the oracle's on w
      eng.set_option('mfma_products', 3)
      assert np.abs(eng.predict(seed[:n], img[:n]) - want_w[:n]).max() <= GATE
      eng.set_option('mfma_products', 1)
  finally:
    eng.close()


def test_an_activation_below_the_fp16_normals_contributes_nothing():
  """Every channel carries 2^-9 image into conv1_b, so the one voxel of 2^-6 arrives
  there as 2^-15: its hi half is 0, and the result is the oracle's with that image voxel
  zeroed (conv1_b's weights are large enough for the voxel to matter: the oracle's two
  runs differ by far more than the gate at its neighbours).  At the voxel itself the f32
  residual stream, which the mode leaves alone, still carries its 2^-12 past the conv to
  the head: there the result is the mode's definition (half_ref), not the oracle's
  with the voxel zeroed."""
  from oracle import ffn_oracle
  variables = exact_variables(shifts=((-3, -2), (-3, -2), (-3, -2)), w_std=4.0, lom_std=0.5)
  blob = ffn_oracle.weights_blob(variables, 2)
  img, seed = exact_images(1, (33, 33, 33))
  img[img == 2.0 ** -6] = 2.0 ** -5  # 2^-6 is the flushed value: one voxel only
  at = (0, 14, 17, 20)
  img[at] = 2.0 ** -6
  zeroed = img.copy()
  zeroed[at] = 0
  want_kept = ffn_oracle.forward(img, seed, blob, 2)
  want_zeroed = ffn_oracle.forward(zeroed, seed, blob, 2)
  # (every operand is exact here, so the f32 restatement is the definition to ~1e-6)
  want_h64 = half_ref.forward_half(img, seed, variables, 2, acc='h32')
  others = np.ones(img.shape, bool)
  others[at] = False
  assert np.abs(want_kept - want_zeroed)[others].max() > 10 * GATE
  assert np.abs(want_h64 - want_zeroed)[others].max() <= GATE / 10
  eng = _exact_engine(variables, FOV33, 1)
  try:
    got = eng.predict(seed, img)
    print('max|gpu - oracle(zeroed)| %.3g, max|gpu - oracle(kept)| %.3g beside the voxel; '
          '|gpu - half_ref| %.3g at it' % (np.abs(got - want_zeroed)[others].max(),
                                     np.abs(got - want_kept)[others].max(),
                                     abs(got[at] - want_h64[at])))
    assert np.abs(got - want_zeroed)[others].max() <= GATE
    assert np.abs(got - want_kept)[others].max() > GATE
    assert abs(got[at] - want_h64[at]) <= GATE
    # with three products the voxel lives on in the residual half
    eng.set_option('mfma_products', 3)
    assert np.abs(eng.predict(seed, img) - want_kept).max() <= GATE
  finally:
    eng.close()


# ---------------------------------------------------------------------------
# 4. the whole stack against the mode's definition
# ---------------------------------------------------------------------------

CROPS = [(slice(4, 37), slice(5, 38), slice(6, 39)),
         (slice(8, 41), slice(3, 36), slice(10, 43)),
         (slice(2, 35), slice(9, 42), slice(1, 34))]


def _rms(d):
  return float(np.sqrt(np.mean(np.square(d.astype(np.float64)))))


@pytest.fixture(scope='module')
def stack_case(fib25_model, fib25_variables):
  """Inputs, the engine's logits in both modes and the CPU restatements h64 / h32, made
  once: (a) three crops with the pad logit everywhere and the init logit at the centre,
  (b) the first crop with the f32 logits of (a) as the seed."""
  from ffn_amd import engine as hip_engine
  from ffn_amd import synthetic
  from oracle import ffn_oracle
  vol = synthetic.normalize(synthetic.cells_volume((48, 48, 48), seed=3))
  img = np.stack([vol[c] for c in CROPS]).astype(np.float32)
  seed_a = np.full(img.shape, ffn_oracle.f32_logit(0.05), np.float32)
  seed_a[:, 16, 16, 16] = ffn_oracle.f32_logit(0.95)
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=3)
  case = dict(img=img, seed_a=seed_a)
  try:
    f32_a = eng.predict(seed_a[:1], img[:1])
    case['seed_b'] = f32_a
    eng.set_option('mfma_products', 1)
    case['gpu_a1'] = eng.predict(seed_a[:1], img[:1])
    case['gpu_a1_again'] = eng.predict(seed_a[:1], img[:1])
    case['gpu_b1'] = eng.predict(f32_a, img[:1])
    case['gpu_a3'] = eng.predict(seed_a, img)
    case['gpu_a3_again'] = eng.predict(seed_a, img)
    case['variant_batched'] = eng.get_option('conv_variant')
    eng.set_option('conv_variant', 8)
    case['gpu_a_alone8'] = np.concatenate(
        [eng.predict(seed_a[k:k + 1], img[k:k + 1]) for k in range(3)])
  finally:
    eng.close()
  for acc in ('h64', 'h32'):
    case[acc + '_a'] = half_ref.forward_half(img, seed_a, fib25_variables, 12, acc=acc)
    case[acc + '_b'] = half_ref.forward_half(img[:1], f32_a, fib25_variables, 12, acc=acc)
  return case


def _yardstick(name, gpu, h64, h32):
  """max|gpu - h64| <= 4 max|h32 - h64| (this tree's own margin)
  and rms(gpu - h64) <= 2 rms(h32 - h64) (another f32 summation order of the same
  restatement stood to h32 - h64 at rms 0.97 - 1.06 and at max 0.61 - 1.45)."""
  d_gpu, d_ref = gpu - h64, h32 - h64
  mx, mx_ref = float(np.abs(d_gpu).max()), float(np.abs(d_ref).max())
  rms, rms_ref = _rms(d_gpu), _rms(d_ref)
  print('%s: max|gpu - h64| %.3g = %.2f x max|h32 - h64| %.3g;  rms %.3g = %.2f x %.3g' % (
      name, mx, mx / mx_ref, mx_ref, rms, rms / rms_ref, rms_ref))
  assert mx <= 4 * mx_ref, (name, mx, mx_ref)
  assert rms <= 2 * rms_ref, (name, rms, rms_ref)


@pytest.mark.parametrize('which', ['a', 'b'])
def test_whole_stack_single_fov(stack_case, which):
  c = stack_case
  _yardstick('(%s) n = 1' % which, c['gpu_%s1' % which][0], c['h64_' + which][0],
             c['h32_' + which][0])


def test_whole_stack_batch_of_three(stack_case):
  c = stack_case
  for k in range(3):
    _yardstick('(a) n = 3, item %d' % k, c['gpu_a3'][k], c['h64_a'][k], c['h32_a'][k])


def test_whole_stack_bits(stack_case):
  """Two runs give equal bits; item i of a batch equals the same FoV alone under
  conv_variant 8 (conv32m's sums do not depend on the batch)."""
  c = stack_case
  assert np.array_equal(c['gpu_a1'].view(np.uint32), c['gpu_a1_again'].view(np.uint32))
  assert np.array_equal(c['gpu_a3'].view(np.uint32), c['gpu_a3_again'].view(np.uint32))
  assert np.array_equal(c['gpu_a3'].view(np.uint32), c['gpu_a_alone8'].view(np.uint32))


# ---------------------------------------------------------------------------
# 5. back to three products
# ---------------------------------------------------------------------------


def _one_step(eng, vol):
  from ffn_amd import _lib
  from oracle import ffn_oracle
  canvas = eng.create_canvas(vol)
  pos = (24, 24, 24)
  canvas.init_seed(pos, ffn_oracle.f32_logit(0.95))
  req = _lib.StepRequest()
  req.pos[:] = pos
  req.start_pos[:] = pos
  req.num_candidates = 0
  res = eng.step1(canvas, req, _lib.StepParams(ffn_oracle.f32_logit(0.05),
                                                ffn_oracle.f32_logit(0.9), 0.0))
  seed = np.array(canvas.read_seed())
  canvas.close()
  return seed, list(res.face_score), list(res.face_index)


def test_back_to_three_products(fib25_model):
  from ffn_amd import engine as hip_engine
  from ffn_amd import synthetic
  vol = synthetic.normalize(synthetic.cells_volume((48, 48, 48), seed=3))
  img, seed = _inputs(np.random.RandomState(12), 1)
  fresh = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
  try:
    eng.set_option('mfma_products', 1)
    half = eng.predict(seed, img)
    half_step = _one_step(eng, vol)
    eng.set_option('mfma_products', 3)
    want, want_step = fresh.predict(seed, img), _one_step(fresh, vol)
    got, got_step = eng.predict(seed, img), _one_step(eng, vol)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got_step[0], want_step[0], equal_nan=True)
    assert got_step[1:] == want_step[1:]
    assert not np.array_equal(half, want)
    assert not np.array_equal(half_step[0], want_step[0], equal_nan=True)
  finally:
    eng.close()
    fresh.close()


# ---------------------------------------------------------------------------
# 6. the fp16 range guard
# ---------------------------------------------------------------------------


@pytest.mark.parametrize('fast', [9, 8])
def test_range_guard_with_the_mode_on(fib25_model, fib25_blob, fast):
  """test_fp16_range_fallback's predict and canvas-step halves with mfma_products = 1: a
  value beyond 65504 voids the run (nothing pasted), the repeat runs on exact_variant --
  a family that ignores the option -- and the exact kernel's answer comes back."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
  try:
    eng.set_option('conv_variant', fast)
    eng.set_option('mfma_products', 1)
    img, seed = _inputs(np.random.RandomState(12), 1)
    eng.predict(seed, img)
    assert eng.get_option('conv_variant') == fast  # ordinary data stays on fp16
    big = (img * 3e5).astype(np.float32)  # conv0_a outputs far beyond 65504
    got = eng.predict(seed, big)
    assert eng.get_option('conv_variant') == 2 == eng.get_option('exact_variant')
    assert eng.get_option('mfma_products') == 1
    want = ffn_oracle.forward(big, seed, fib25_blob, 12)
    assert np.isfinite(got).all()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    # canvas step: the voided step leaves the canvas untouched, then repeats
    eng.set_option('conv_variant', fast)
    vol = np.zeros((40, 40, 40), np.float32)
    vol[4:37, 4:37, 4:37] = big[0]
    canvas = eng.create_canvas(vol)
    start = (20, 20, 20)
    canvas.init_seed(start, 2.9444386959)
    params = _lib.StepParams(-2.9444389343, 2.1972243786, 0.0)
    req = _lib.StepRequest()
    req.pos[:] = start
    req.start_pos[:] = start
    req.num_candidates = 0
    arr = (ctypes.c_void_p * 1)()
    arr[0] = canvas._h
    res = (_lib.StepResult * 1)()
    rc = eng._lib.ffn_canvas_step(eng._h, 1, arr, ctypes.byref(req), ctypes.byref(params),
                                  res)
    assert rc == _lib.ERR_RANGE and res[0].range_error == 1
    seed_now = canvas.read_seed()
    assert np.isnan(seed_now).sum() == seed_now.size - 1  # nothing was pasted
    eng.set_option('conv_variant', fast)
    r = eng.step1(canvas, req, params)  # the Python handle repeats on the exact kernel
    assert eng.range_fallbacks == 1 and eng.get_option('conv_variant') == 2
    assert r.range_error == 0 and np.isfinite(r.start_logit)
    pasted = np.array(canvas.read_seed((4, 4, 4), (37, 37, 37)))
    assert np.isfinite(pasted).all()
    canvas.close()
    # the exact kernel's answer: an engine on variant 2 that never saw the option
    plain = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
    try:
      plain.set_option('conv_variant', 2)
      canvas = plain.create_canvas(vol)
      canvas.init_seed(start, 2.9444386959)
      plain.step1(canvas, req, params)
      assert np.array_equal(pasted, canvas.read_seed((4, 4, 4), (37, 37, 37)))
      canvas.close()
    finally:
      plain.close()
  finally:
    eng.close()


# ---------------------------------------------------------------------------
# 7. canvas and loops
# ---------------------------------------------------------------------------


def _iou(a, b):
  union = np.logical_or(a, b).sum()
  return float(np.logical_and(a, b).sum()) / float(union) if union else 1.0


def test_the_three_loops_agree_with_the_mode_on(fib25_model):
  """One segment of cells_volume 56^3 (seed 3) through the Python loop, the library's
  ffn_canvas_segment_at and a two-canvas MultiCanvasDriver run, all on conv32m
  (conv_variant 8, the kernel every batch form shares) with one product: the same
  positions, segmentation, seed logits and counters.  On conv32mt (9, single FoVs) the
  Python loop and the library's loop agree as well.  The foreground IoU against the f32
  run of the same engine is printed, not asserted: no per-volume number can be promised
  (DESIGN.md section 3.7)."""
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.inference import seed as seed_lib
  from oracle import ffn_oracle
  import bench
  request = bench.make_request()
  image = synthetic.normalize(synthetic.cells_volume((56, 56, 56), seed=3))
  grid = ffn_oracle.grid_seeds((56, 56, 56), (16, 16, 16))

  class PythonLoop(inference.DeviceCanvas):
    NATIVE_LOOP = False

  counters = inference_utils.Counters()
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None, counters, 2)
  eng = exe.engine

  def make(cls=inference.DeviceCanvas):
    sub = counters.get_sub_counters()
    return cls(fib25_model.info, exe.get_client(sub, direct=True), image,
               request.inference_options, counters=sub, keep_history=True,
               movement_policy_fn=movement.get_policy_fn(request, fib25_model.info))

  def result(c):
    out = dict(seg=np.array(np.asarray(c.segmentation)),
               seed=np.array(c._handle.read_seed()), history=list(c.history),
               rejects=c.gate_rejects,
               counters={k: c.counters[k].value for k in (
                   'update_at-calls', 'skip_threshold', 'skip_invalid_pos',
                   'seed_got_too_weak', 'segment_at-loop-calls', 'voxels-segmented')})
    c.close()
    return out

  def same(a, b):
    assert a['history'] == b['history']
    assert a['counters'] == b['counters'] and a['rejects'] == b['rejects']
    assert np.array_equal(a['seg'], b['seg'])
    assert np.array_equal(a['seed'], b['seed'], equal_nan=True)

  # the f32 run finds where a segment starts: the origin that took the most steps
  eng.set_option('conv_variant', 8)
  c = make()
  c.segment_all(seed_policy=functools.partial(seed_lib.PolicyFixed, coords=grid))
  assert c.origins
  start = max(c.origins.values(), key=lambda o: o.iters).start_zyx
  c.close()
  one = functools.partial(seed_lib.PolicyFixed, coords=[start])
  c = make()
  c.segment_all(seed_policy=one)
  f32 = result(c)
  assert f32['counters']['update_at-calls'] > 1 and (f32['seg'] > 0).any()

  eng.set_option('mfma_products', 1)
  runs = {}
  for name, cls in (('python', PythonLoop), ('library', inference.DeviceCanvas)):
    c = make(cls)
    assert c._native_loop_ok() == (cls is inference.DeviceCanvas)
    c.segment_all(seed_policy=one)
    runs[name] = result(c)
  pair = [make(), make()]
  drv = inference.MultiCanvasDriver(eng, batch_size=2, native=True)
  drv.run((c, one) for c in pair)
  assert eng.get_option('conv_variant') == 8 and eng.get_option('mfma_products') == 1
  runs['driver0'], runs['driver1'] = result(pair[0]), result(pair[1])
  for name in ('library', 'driver0', 'driver1'):
    same(runs[name], runs['python'])
  assert runs['python']['counters']['update_at-calls'] > 1
  print('conv32m, one segment from %s: %d steps with one product, %d with three; '
        'foreground IoU against the f32 run %.5f' % (
            tuple(start), runs['python']['counters']['update_at-calls'],
            f32['counters']['update_at-calls'],
            _iou(runs['python']['seg'] > 0, f32['seg'] > 0)))

  # single FoVs on conv32mt: per-layer launches, main and tail workgroups
  eng.set_option('conv_variant', 9)
  mt = {}
  for name, cls in (('python', PythonLoop), ('library', inference.DeviceCanvas)):
    c = make(cls)
    c.segment_all(seed_policy=one)
    mt[name] = result(c)
  same(mt['library'], mt['python'])
  assert mt['python']['counters']['update_at-calls'] > 1
  exe.stop_server()


def _request(vol_path, out_dir, fov):
  from ffn_amd.inference import request as req_lib
  return req_lib.request_from_text('''
    image { npy: "%s" }
    image_mean: 128
    image_stddev: 33
    seed_policy: "PolicyPeaks"
    model_checkpoint_path: "%s"
    model_name: "convstack_3d.ConvStack3DFFNModel"
    model_args: "{\\"depth\\": 12, \\"fov_size\\": [%d, %d, %d], \\"deltas\\": [%d, %d, %d]}"
    segmentation_output_dir: "%s"
    inference_options {
      init_activation: 0.95
      pad_value: 0.05
      move_threshold: 0.9
      min_boundary_dist { x: 1 y: 1 z: 1}
      segment_threshold: 0.6
      min_segment_size: 500
    }''' % ((vol_path, os.path.join(GOLDEN, 'fib25_weights.npz')) + tuple(fov[0]) +
            tuple(fov[1]) + (out_dir,)))


def test_runner_fp16_run_many_writes_the_files(tmp_path):
  from ffn_amd import synthetic
  from ffn_amd.inference import runner as runner_lib
  from ffn_amd.inference import storage
  vol = synthetic.cells_volume((56, 56, 112), seed=3)
  vol_path = str(tmp_path / 'vol.npy')
  np.save(vol_path, vol)
  out_dir = str(tmp_path / 'out')
  runner = runner_lib.Runner(precision='fp16')
  runner.start(_request(vol_path, out_dir, FOV33), batch_size=2, direct=True)
  try:
    assert runner.executor.engine.get_option('mfma_products') == 1
    boxes = [((0, 0, 0), (56, 56, 56)), ((0, 0, 56), (56, 56, 56))]
    canvases = runner.run_many(boxes, batch_size=2)
    assert len(canvases) == 2 and all(c is not None for c in canvases)
    assert runner.executor.engine.get_option('mfma_products') == 1
    steps = 0
    for corner, size in boxes:
      assert os.path.exists(storage.segmentation_path(out_dir, corner))
      seg, _ = storage.load_segmentation(out_dir, corner, split_cc=False)
      assert seg.shape == size
      steps += int(seg.max() > 0)
    assert steps > 0  # something was segmented
  finally:
    runner.stop_executor()
  with pytest.raises(ValueError):
    runner_lib.Runner(precision='bf16')


def test_runner_fp16_needs_conv32m(tmp_path):
  """A FoV of 5^3 has a single 128-voxel chunk: neither conv32m nor conv32mt takes it,
  the engine's default is its exact kernel, and precision='fp16' is refused."""
  from ffn_amd import synthetic
  from ffn_amd.inference import runner as runner_lib
  vol_path = str(tmp_path / 'vol.npy')
  np.save(vol_path, synthetic.cells_volume((24, 24, 24), seed=3))
  small = ((5, 5, 5), (1, 1, 1))
  runner = runner_lib.Runner(precision='fp16')
  with pytest.raises(ValueError, match='conv32m'):
    runner.start(_request(vol_path, str(tmp_path / 'out'), small))
  runner.stop_executor()
  # the f32 path takes the same request
  runner = runner_lib.Runner()
  runner.start(_request(vol_path, str(tmp_path / 'out32'), small))
  assert runner.executor.engine.default_variant not in (8, 9)
  runner.stop_executor()
