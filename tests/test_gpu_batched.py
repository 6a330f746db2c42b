"""GPU tests of batched inference: 5 .. 32 FoVs per engine call against the
double-precision oracle (oracle.ffn_oracle.forward_f64c) and the f32 C oracle.

Batch size changes the shape of the code, not only its size:
- the split-product convs (conv32d / conv32m) deal n * nchunks chunks
  round-robin over a grid of 8 * ceil(n * nchunks / 8) slots, find the FoV of a
  chunk by a magic division and address its activations at item * item_bytes;
- conv32mt_kernel<..., 3> (engine option tail_batched) runs only when n > 1;
- the fused head's move counts land in head_count[] per workgroup and are summed
  per item (sum_block_counts), which decides disco per canvas;
- a step of several canvases reads its StepItems from d_items (item_view with
  use_inline = 0) and launches paste_kernel / faces_kernel / conv0a / the head
  on one grid row per item; two steps in flight sit at slot * max_batch;
- one FoV beyond the fp16 range voids the whole batch (range_flag: one word
  per step).

The engine states that conv32m's arithmetic does not depend on the batch
(engine.pin_batched_arithmetic), so most checks here are bit for bit: a FoV in
a batch of 32 against the same FoV run alone.  TOL (1e-4 absolute on logits of
order 10) is the contract bound against both oracles.
"""

import ctypes
import functools
import os

import numpy as np
import pytest

from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 1e-4
FP16_MAX = 65504.0
NS = (5, 8, 16, 32)
# the FoVs of the 33^3 batch that are not plain random inputs
PAD, NEAR16, NANFOV = 1, 2, 3
# conv_variant of a single FoV that runs the same arithmetic as `variant` does
# for a batch: variant 9 is conv32m at n > 1 (= variant 8) and conv32mt at n = 1
COUNTERPART = {0: 0, 2: 2, 6: 6, 7: 7, 8: 8, 9: 8}


def _pad_logit():
  from oracle import ffn_oracle
  return np.float32(ffn_oracle.f32_logit(0.05))


def _same_bits(a, b):
  return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


# ---------------------------------------------------------------------------
# 1. stateless predict at n in {5, 8, 16, 32}
# ---------------------------------------------------------------------------


@pytest.fixture(scope='module')
def eng32(fib25_model):
  from ffn_amd import engine as hip_engine
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=32, device_id=0)
  yield eng
  eng.close()


def _max_activation(img, seed, blob, depth):
  """max over every conv output of what the next conv consumes (ReLU'd): the
  operands the split-product kernels convert to fp16 pairs."""
  from oracle import ffn_oracle
  return max(float(np.maximum(ffn_oracle.forward(img, seed, blob, depth,
                                                 stop_after=k), 0).max())
             for k in range(2 * depth))


@pytest.fixture(scope='module')
def batch33(fib25_blob):
  """32 distinct 33^3 FoVs (random images, seeds of different amplitudes) with
  their f64 and f32 oracle logits.  Item PAD is all pad (zero image, seed at
  logit(0.05)); item NEAR16 is scaled so that its largest fp16 operand is about
  0.85 x 65504 (conv0_a's outputs above 0.4 x 65504); item NANFOV has NaN and
  large finite values on its boundary planes and corners, the voxels whose
  halo reads would cross into a neighbouring item."""
  from oracle import ffn_oracle
  rng = np.random.RandomState(2026)
  n = 32
  img = ((rng.randint(0, 256, (n, 33, 33, 33)).astype(np.float32)) - 128) / 33
  seed = np.full((n, 33, 33, 33), _pad_logit(), np.float32)
  seed[:, 16, 16, 16] = ffn_oracle.f32_logit(0.95)
  for k in range(n):
    amp = 0.25 + 3.0 * k / n
    z0, y0, x0 = rng.randint(2, 12, 3)
    seed[k, z0:z0 + 18, y0:y0 + 18, x0:x0 + 18] += rng.normal(
        0, amp, (18, 18, 18)).astype(np.float32)
  img[PAD] = 0.0
  seed[PAD] = _pad_logit()
  # near the fp16 limit: at large scales the stack is close to positively
  # homogeneous in the image, so one probe of every layer fixes the scale
  base = img[NEAR16].copy()
  c0a = float(ffn_oracle.forward(base, seed[NEAR16], fib25_blob, 12,
                                 stop_after=0).max())
  scale = 0.45 * FP16_MAX / c0a
  probe = _max_activation(base * np.float32(scale), seed[NEAR16], fib25_blob, 12)
  img[NEAR16] = base * np.float32(scale * 0.85 * FP16_MAX / probe)
  near_max = _max_activation(img[NEAR16], seed[NEAR16], fib25_blob, 12)
  c0a_max = float(ffn_oracle.forward(img[NEAR16], seed[NEAR16], fib25_blob, 12,
                                     stop_after=0).max())
  assert 0.6 * FP16_MAX < near_max < 0.95 * FP16_MAX, near_max
  assert 0.4 * FP16_MAX < c0a_max < FP16_MAX, c0a_max
  # NaN / large finite values on the boundary
  q = NANFOV
  img[q, 0] = 900.0
  img[q, :, :, 32] = -700.0
  img[q, :, 32, :] = np.nan
  seed[q, :, 0, :] = 40.0
  for c in ((0, 0, 0), (0, 0, 32), (32, 32, 32), (32, 0, 32), (0, 32, 0)):
    img[(q,) + c] = np.nan
    seed[(q,) + c] = np.nan
  seed[q, 32, :, 0] = np.nan
  want64 = ffn_oracle.forward_f64c(img, seed, fib25_blob, 12)
  want32 = ffn_oracle.forward(img, seed, fib25_blob, 12)
  print('near-fp16 FoV: largest fp16 operand %.0f, conv0_a %.0f' % (near_max, c0a_max))
  return img, seed, want64, want32


def _check_rows(got, want64, want32, idx, label):
  """Rows of `got` (FoVs idx) against the oracles; returns max |err| vs f64."""
  worst = 0.0
  for r, k in enumerate(idx):
    if k == NANFOV:
      continue  # NaN in the inputs: compared with its own n = 1 run only
    w64 = want64[k].astype(np.float64)
    if k == NEAR16:
      # logits of order 1e5: the f32 bound of test_fp16_range_fallback
      bound = 1e-5 * np.abs(w64).max()
    else:
      bound = TOL
    err64 = float(np.abs(got[r] - w64).max())
    err32 = float(np.abs(got[r] - want32[k]).max())
    assert np.isfinite(got[r]).all(), (label, k)
    assert err64 <= bound and err32 <= bound, (label, k, err64, err32, bound)
    if k != NEAR16:
      worst = max(worst, err64)
  return worst


def _set_variant(eng, variant, tail_batched):
  eng.set_option('conv_variant', variant)
  eng.set_option('tail_batched', tail_batched)


@pytest.mark.parametrize('variant,tail_batched', [
    (0, 0), (2, 0), (6, 0), (7, 0), (8, 0), (9, 0), (9, 1)])
def test_predict_batches_match_f64_and_run_alone_bits(eng32, batch33, variant,
                                                      tail_batched):
  """ffn_predict at n = 5, 8, 16, 32 on every conv kernel the 33^3 engine takes:
  conv_variant 0 / 2 (exact f32), 6 / 7 (conv32d), 8 (conv32m), 9 (conv32m at
  n > 1) and 9 + tail_batched (conv32mt_kernel<..., 3>: the K-split tail of a
  batch).  n = 5 and 16 leave n * nchunks off a multiple of 8, so the last
  grid slots are empty.  Every FoV is within TOL of the f64 and f32 oracles, and
  equals -- bit for bit -- its logits when run alone with the same arithmetic
  (9 at n > 1 against 8 at n = 1; 9 + tail_batched against itself), wherever it
  sits in the batch and whatever ran before (slot and stale-data invariance:
  32, reversed 32, items 15..31 as a ragged 17, then 5).  The near-fp16 FoV
  voids nothing; the FoVs next to the NaN FoV give the same bits without it."""
  img, seed, want64, want32 = batch33
  eng = eng32
  try:
    _set_variant(eng, COUNTERPART[variant] if not tail_batched else variant,
                 tail_batched)
    single_variant = eng.get_option('conv_variant')
    alone = np.stack([eng.predict(seed[k:k + 1], img[k:k + 1])[0]
                      for k in range(32)])
    assert eng.get_option('conv_variant') == single_variant  # no void
    _check_rows(alone, want64, want32, range(32), (variant, tail_batched, 1))
    _set_variant(eng, variant, tail_batched)
    errs = []
    full = None
    for n in NS:
      got = eng.predict(seed[:n], img[:n])
      assert eng.get_option('conv_variant') == variant  # no void
      errs.append(_check_rows(got, want64, want32, range(n),
                              (variant, tail_batched, n)))
      for k in range(n):
        assert _same_bits(got[k], alone[k]), (variant, tail_batched, n, k)
      full = got
    # slot / stale-data invariance
    rev = eng.predict(seed[::-1], img[::-1])[::-1]
    assert _same_bits(rev, full)
    rag = eng.predict(seed[15:], img[15:])
    assert _same_bits(rag, full[15:])
    five = eng.predict(seed[:5], img[:5])
    assert _same_bits(five, full[:5])
    # isolation: the NaN FoV's neighbours, with a plain FoV in its place
    s2, i2 = seed[:8].copy(), img[:8].copy()
    s2[NANFOV], i2[NANFOV] = seed[20], img[20]
    clean = eng.predict(s2, i2)
    for k in range(8):
      if k != NANFOV:
        assert _same_bits(clean[k], full[k]), k
    assert _same_bits(clean[NANFOV], full[20])
    assert eng.get_option('conv_variant') == variant
    print('33^3 variant %d tail_batched %d: max |err| vs f64 %s at n = %s '
          '(n = 1 alone: same bits)' % (variant, tail_batched,
                                        ' '.join('%.3g' % e for e in errs), NS))
  finally:
    eng.set_option('tail_batched', 0)
    eng.restore_default_variant()


@pytest.mark.parametrize('fast', [9, 8, 6])
def test_range_void_in_a_batch_of_16(fib25_model, batch33, fib25_blob, fast):
  """One FoV of 16 beyond 65504 (the `big` input of test_fp16_range_fallback):
  the range flag, one word per step, voids the whole batch; ffn_predict repeats
  it with the exact-f32 kernel, every row matches the oracle and the engine
  stays on exact_variant."""
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  img, seed, want64, _ = batch33
  idx = [k for k in range(4, 20)]
  bad = 7
  im, sd = img[idx].copy(), seed[idx].copy()
  im[bad] = (im[bad] * 3e5).astype(np.float32)
  want_big = ffn_oracle.forward_f64c(im[bad], sd[bad], fib25_blob, 12)
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=16)
  try:
    eng.set_option('conv_variant', fast)
    got = eng.predict(sd, im)
    assert eng.get_option('conv_variant') == eng.get_option('exact_variant') == 2
    for r, k in enumerate(idx):
      if r == bad:
        assert np.isfinite(got[r]).all()
        assert np.abs(got[r] - want_big).max() <= 1e-5 * np.abs(want_big).max()
      else:
        assert np.abs(got[r] - want64[k]).max() <= TOL, (r, k)
  finally:
    eng.close()


@pytest.mark.parametrize('fov_xyz,deltas_xyz,depth,n', [
    ([41, 41, 21], [10, 10, 5], 3, 16),  # permuted layout (BASELINE configs[4])
    ([25, 25, 25], [6, 6, 6], 3, 8),     # conv32mt does not take these
    ([29, 21, 17], [7, 5, 4], 3, 8)])
def test_other_geometries_at_batch(fov_xyz, deltas_xyz, depth, n):
  """Chunking, magic divisions and item strides of other FoVs at batch: every
  variant the engine accepts (a refusal is FFNHipError) against f64 within TOL,
  and the FoVs run alone (9 -> 8 at n = 1) give the same bits."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  from ffn_amd.training.models import convstack_3d
  from oracle import ffn_oracle
  variables = ffn_oracle.random_weights(depth, seed=33, stddev=0.06)
  m = convstack_3d.ConvStack3DFFNModel(fov_size=fov_xyz, deltas=deltas_xyz,
                                       depth=depth)
  m.set_variables(variables)
  blob = ffn_oracle.weights_blob(variables, depth)
  zyx = fov_xyz[::-1]
  rng = np.random.RandomState(17)
  amp = np.linspace(0.3, 3.0, n).astype(np.float32)[:, None, None, None]
  img = rng.normal(0, 1, [n] + zyx).astype(np.float32)
  seed = (rng.normal(0, 1, [n] + zyx).astype(np.float32) * amp).astype(np.float32)
  img[1] = 0.0
  seed[1] = _pad_logit()
  want = ffn_oracle.forward_f64c(img, seed, blob, depth)
  eng = hip_engine.HipEngine.from_model(m, max_batch=n)
  ran = []
  try:
    default = eng.get_option('conv_variant')
    for variant in (0, 2, 6, 7, 8, 9):
      try:
        eng.set_option('conv_variant', variant)
      except _lib.FFNHipError:
        continue  # this kernel does not take this FoV
      got = eng.predict(seed, img)
      err = float(np.abs(got - want).max())
      assert err <= TOL, (variant, err)
      alone_variant = COUNTERPART[variant] if variant in COUNTERPART else variant
      try:
        eng.set_option('conv_variant', alone_variant)
      except _lib.FFNHipError:
        alone_variant = None
      if alone_variant is not None:
        for k in range(n):
          assert _same_bits(eng.predict(seed[k:k + 1], img[k:k + 1])[0], got[k]), (
              variant, k)
      eng.set_option('conv_variant', variant)
      assert _same_bits(eng.predict(seed[::-1], img[::-1])[::-1], got), variant
      ran.append(variant)
      print('fov %s n %d variant %d: max |err| vs f64 %.3g' % (fov_xyz, n, variant,
                                                              err))
    assert 0 in ran and default in ran and len(ran) >= 3, ran
  finally:
    eng.close()


# ---------------------------------------------------------------------------
# 2. batched canvas steps
# ---------------------------------------------------------------------------

# (shape zyx, u8 canvas, start position): from just over one FoV to 128^3,
# elongated boxes, FoVs touching canvas faces (16 / s - 17), f32 and u8 mixed
CANVASES = [
    ((34, 35, 36), False, (17, 17, 18)),
    ((33, 40, 48), True, (16, 16, 16)),
    ((40, 40, 120), False, (23, 20, 103)),
    ((128, 36, 40), True, (111, 18, 23)),
    ((48, 128, 34), False, (24, 60, 17)),
    ((36, 50, 100), True, (19, 33, 50)),
    ((64, 64, 64), False, (32, 32, 32)),
    ((128, 128, 128), True, (64, 70, 58)),
    ((33, 33, 33), False, (16, 16, 16)),
    ((60, 44, 80), True, (43, 27, 40)),
    ((100, 40, 40), False, (50, 17, 22)),
    ((45, 90, 45), True, (28, 45, 16)),
    ((70, 70, 34), False, (35, 53, 17)),
    ((38, 38, 76), True, (21, 21, 59)),
    ((52, 52, 52), False, (17, 35, 26)),
    ((34, 66, 98), True, (17, 33, 81)),
]
MOVE = (8, 8, 8)


def _params_probs():
  from oracle import ffn_oracle
  return (ffn_oracle.f32_logit(0.05), ffn_oracle.f32_logit(0.9),
          float(np.float32(ffn_oracle.logit(0.8))))


class _Case:
  """One canvas of the batch: its image, its prepared seed and its oracle."""

  def __init__(self, k, shape, u8, start, blob, scale=None):
    from ffn_amd import synthetic
    from ffn_amd.inference import inference
    from oracle import ffn_oracle
    self.shape, self.u8, self.start = shape, u8, tuple(start)
    raw = synthetic.cells_volume(shape, seed=300 + k)
    self.raw = raw
    image = synthetic.normalize(raw)
    if scale is not None:  # a FoV beyond fp16 range (f32 canvases only)
      lo = [p - 16 for p in start]
      sel = tuple(slice(l, l + 33) for l in lo)
      image[sel] *= np.float32(scale)
    self.image = image
    self.make_image = (lambda: inference.NormalizedU8Image(raw, 128.0, 33.0)) if u8 \
        else (lambda: image)
    self.oc = ffn_oracle.OracleCanvas(image, blob, 12, (33, 33, 33), MOVE,
                                      ffn_oracle.Options())
    # a prepared seed around the start: some canvases mostly above the move
    # threshold, some mostly below, a fifth NaN (never predicted)
    rng = np.random.RandomState(500 + k)
    lo = [max(p - 20, 0) for p in start]
    hi = [min(p + 21, s) for p, s in zip(start, shape)]
    box = tuple(h - l for l, h in zip(lo, hi))
    mu = (-4.0, 3.5, -1.0, 2.0)[k % 4]
    s = (rng.normal(mu, 2.0, box)).astype(np.float32)
    s[rng.rand(*box) < 0.2] = np.nan
    self.box = (lo, hi, s)
    sel = tuple(slice(l, h) for l, h in zip(lo, hi))
    self.oc.seed[sel] = s
    self.oc.seed[self.start] = self.oc.init_activation
    self.pos = self.start
    rng_c = np.random.RandomState(700 + k)
    nc = (k * 5) % 17
    self.cands = [tuple(int(rng_c.randint(0, d)) for d in shape) for _ in range(nc)]
    if nc:
      self.cands[0] = self.start

  def canvas(self, eng):
    c = eng.create_canvas(self.make_image())
    lo, hi, s = self.box
    c.write_seed(lo, hi, s)
    c.write_seed(self.start, [p + 1 for p in self.start],
                 np.float32(self.oc.init_activation))
    return c

  def request(self):
    from ffn_amd import _lib
    r = _lib.StepRequest()
    r.pos[:] = self.pos
    r.start_pos[:] = self.start
    r.num_candidates = len(self.cands)
    for j, c in enumerate(self.cands):
      r.candidates[j][:] = c
    return r

  def fov_inputs(self):
    sel = tuple(slice(p - 16, p + 17) for p in self.pos)
    s = np.array(self.oc.seed[sel])
    s[np.isnan(s)] = np.float32(self.oc.pad_value)
    return self.image[sel], s

  def valid(self, p):
    return all(16 <= v <= s - 17 for v, s in zip(p, self.shape))

  def next_pos(self, logits):
    """The best face (oracle scores) whose position a step can take."""
    from oracle import ffn_oracle
    scores, _ = ffn_oracle.face_maxima(MOVE, logits)
    order = np.argsort(-scores, kind='stable')
    for f in order:
      axis, sign = f // 2, (-1, 1)[f % 2]
      p = list(self.pos)
      p[axis] += sign * MOVE[axis]
      if self.valid(p):
        return tuple(p)
    return self.pos


def _disco_threshold(fracs, voxels):
  """A threshold between the per-canvas fractions of logits >= move_threshold
  that leaves at least 3 canvases on each side, in the widest such gap."""
  f = np.sort(np.asarray(fracs))
  best, thr = -1.0, None
  for j in range(3, len(f) - 2):
    gap = f[j] - f[j - 1]
    if gap > best:
      best, thr = gap, 0.5 * (f[j] + f[j - 1])
  assert best * voxels >= 20, ('fractions too close for a clean disco split', f)
  return float(np.float32(thr))


def _res_tuple(r, nc):
  return (tuple(np.float32(v).view(np.uint32) for v in r.face_score),
          tuple(r.face_index), np.float32(r.start_logit).view(np.uint32),
          r.num_above_move, r.disco_applied, r.num_deleted,
          tuple(np.float32(r.cand_seed[j]).view(np.uint32) for j in range(nc)),
          tuple(r.cand_seg[j] for j in range(nc)), r.range_error)


def _oracle_round(cases, params_fn, blob):
  """Oracle logits for every case at its current position; returns the step
  params with a disco threshold that splits the batch."""
  from oracle import ffn_oracle
  ins = [c.fov_inputs() for c in cases]
  raw = ffn_oracle.forward(np.stack([a for a, _ in ins]),
                           np.stack([b for _, b in ins]), blob, 12)
  pad, move, deleted = _params_probs()
  fracs = [float(np.mean(r >= np.float32(move))) for r in raw]
  thr = _disco_threshold(fracs, raw[0].size)
  return raw, fracs, params_fn(pad, move, thr, deleted)


def _check_step(case, res, logits, disco, seg=None):
  from oracle import ffn_oracle
  oc = case.oc
  scores, idx = ffn_oracle.face_maxima(MOVE, logits)
  assert np.allclose(list(res.face_score), scores, atol=TOL, rtol=0)
  assert list(res.face_index) == [int(i) for i in idx]
  assert abs(res.start_logit - oc.seed[case.start]) <= TOL
  assert bool(res.disco_applied) == disco
  assert abs(int(res.num_deleted) - oc.last_deleted) <= oc.last_deleted_ties
  for j, c in enumerate(case.cands):
    a, b = res.cand_seed[j], oc.seed[c]
    assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= TOL, (j, a, b)
    assert res.cand_seg[j] == (0 if seg is None else seg[c])


def test_batched_canvas_steps_match_oracle_and_single_steps(eng32, fib25_model,
                                                           fib25_blob):
  """ffn_canvas_step with 16 canvases per call (d_items, paste_kernel on
  dim3(71, n), faces_kernel on dim3(n), conv0a on dim3(tiles, n), the head on
  dim3(kHeadBlocks, n), per-item move counts -> disco): canvases of different
  sizes (34^3 .. 128^3, elongated), f32 and u8 images in one call, FoVs touching
  canvas faces, different candidate lists, and a disco threshold that is passed
  by some canvases and not by others.  Three rounds, each moving every canvas
  to a face its oracle scores.  Checked per canvas against an OracleCanvas:
  face scores within TOL and indices exact, disco decision exact, num_deleted
  within the oracle's ties, candidate seeds, the whole seed array within TOL
  with the same NaN pattern.  A twin set stepped ONE canvas at a time on a
  variant-8 engine (the fused faces + paste + next conv0_a launch, with
  speculation) and a twin set batched in another order end bit for bit equal."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  cases = [_Case(k, *spec, blob=fib25_blob) for k, spec in enumerate(CANVASES)]
  n = len(cases)
  eng1 = hip_engine.HipEngine.from_model(fib25_model, max_batch=1)
  try:
    eng1.set_option('conv_variant', 8)
    assert eng32.get_option('conv_variant') == 9 and not eng32.variant_is_explicit
    main = [c.canvas(eng32) for c in cases]
    single = [c.canvas(eng1) for c in cases]
    perm = np.random.RandomState(3).permutation(n)
    permuted = [cases[j].canvas(eng32) for j in perm]
    both = []
    for rnd in range(3):
      raw, fracs, params = _oracle_round(cases, _lib.StepParams, fib25_blob)
      reqs = [c.request() for c in cases]
      got = eng32.step(main, reqs, params)
      got_single = [_res_tuple(eng1.step1(sc, r, params), len(c.cands))
                    for sc, r, c in zip(single, reqs, cases)]
      got_perm = eng32.step(permuted, [reqs[j] for j in perm], params)
      discos = []
      for k, c in enumerate(cases):
        c.oc.disco_seed_threshold = params.disco_seed_threshold
        c.oc.forward_fn = (lambda a, b, out=raw[k]: out.copy())
        logits = c.oc.update_at(c.pos)
        disco = fracs[k] > params.disco_seed_threshold
        discos.append(disco)
        _check_step(c, got[k], logits, disco)
        seed_now = main[k].read_seed()
        assert np.array_equal(np.isnan(seed_now), np.isnan(c.oc.seed)), (rnd, k)
        assert np.nanmax(np.abs(seed_now - c.oc.seed)) <= TOL, (rnd, k)
        mine = _res_tuple(got[k], len(c.cands))
        assert got_single[k] == mine, (rnd, k)
        assert _res_tuple(got_perm[int(np.where(perm == k)[0][0])],
                          len(c.cands)) == mine, (rnd, k)
        c.pos = c.next_pos(logits)
      assert any(discos) and not all(discos), discos
      both.append(sum(discos))
    for k in range(n):
      want = main[k].read_seed()
      assert _same_bits(single[k].read_seed(), want), k
      assert _same_bits(permuted[int(np.where(perm == k)[0][0])].read_seed(), want), k
    print('16 canvases x 3 rounds: disco on for %s of 16 per round; bit-equal to '
          'single steps and to a permuted batch' % both)
    for c in main + permuted:
      c.close()
  finally:
    eng1.close()


def test_two_full_steps_in_flight(eng32):
  """ffn_canvas_step_submit twice with n = max_batch = 32 (both slots of
  h_items / d_items / h_pub full, at slot * max_batch), then
  ffn_canvas_step_wait on both: every result and canvas equals the blocking
  run, bit for bit.  Canvas sizes and f32 / u8 kinds mixed."""
  from ffn_amd import _lib
  from ffn_amd import synthetic
  from ffn_amd.inference import inference
  pad, move, deleted = _params_probs()
  params = _lib.StepParams(pad, move, 0.0, deleted)
  shapes = [(44, 44, 44), (48, 44, 46), (44, 52, 44), (46, 46, 60)]
  rng = np.random.RandomState(900)
  specs = []
  for k in range(64):
    shape = shapes[k % 4]
    raw = rng.randint(0, 256, shape).astype(np.uint8)
    specs.append((raw, k % 3 == 1, tuple(s // 2 for s in shape)))

  def make():
    cs = []
    for raw, u8, start in specs:
      image = (inference.NormalizedU8Image(raw, 128.0, 33.0) if u8
               else synthetic.normalize(raw))
      c = eng32.create_canvas(image)
      c.init_seed(start, 2.9444386959)
      cs.append(c)
    return cs

  def req(k, pos):
    r = _lib.StepRequest()
    r.pos[:] = pos
    r.start_pos[:] = specs[k][2]
    r.num_candidates = 1
    r.candidates[0][:] = specs[k][2]
    return r

  moves = [(0, 0, 0), (0, 0, 4), (3, -4, 0)]
  a = make()
  want = []
  for mv in moves:
    for g in (0, 1):
      ks = range(32 * g, 32 * g + 32)
      rq = [req(k, [p + d for p, d in zip(specs[k][2], mv)]) for k in ks]
      want += [_res_tuple(r, 1) for r in eng32.step([a[k] for k in ks], rq, params)]
  seeds_want = [c.read_seed() for c in a]
  for c in a:
    c.close()
  b = make()
  got = []
  for mv in moves:
    tickets = []
    for g in (0, 1):
      ks = range(32 * g, 32 * g + 32)
      rq = [req(k, [p + d for p, d in zip(specs[k][2], mv)]) for k in ks]
      tickets.append(eng32.step_submit([b[k] for k in ks], rq, params))
    for t in tickets:
      res = eng32.step_wait(t)
      got += [_res_tuple(res[j], 1) for j in range(32)]
  assert got == want
  for k, c in enumerate(b):
    assert _same_bits(c.read_seed(), seeds_want[k]), k
    c.close()


def test_range_void_in_a_batch_of_16_canvases(fib25_model, fib25_blob):
  """One canvas of 16 holds an image beyond fp16 range at its FoV: the raw
  ffn_canvas_step returns FFN_ERR_RANGE and EVERY canvas's seed and
  segmentation are what they were before the call; the retry through
  engine.step (exact-f32 kernel) then matches the oracle for all 16."""
  from ffn_amd import _lib
  from ffn_amd import engine as hip_engine
  bad = 6  # an f32 canvas
  cases = [_Case(k, *spec, blob=fib25_blob, scale=3e5 if k == bad else None)
           for k, spec in enumerate(CANVASES)]
  assert not cases[bad].u8
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=16)
  try:
    assert eng.get_option('conv_variant') == 9
    canvases = [c.canvas(eng) for c in cases]
    rng = np.random.RandomState(8)
    segs = []
    for c in canvases:  # something to keep in the segmentations (-1 markers)
      seg = np.where(rng.rand(*c.shape) < 0.1, -1, 0).astype(np.int32)
      c.write_segmentation((0, 0, 0), c.shape, seg)
      segs.append(seg)
    before = [(c.read_seed(), c.read_segmentation()) for c in canvases]
    raw, fracs, params = _oracle_round(cases, _lib.StepParams, fib25_blob)
    reqs = (_lib.StepRequest * 16)()
    arr = (ctypes.c_void_p * 16)()
    for k, c in enumerate(cases):
      ctypes.pointer(reqs[k])[0] = c.request()
      arr[k] = canvases[k]._h
    res = (_lib.StepResult * 16)()
    lib = _lib.load()
    rc = lib.ffn_canvas_step(eng._h, 16, arr, reqs, ctypes.byref(params), res)
    assert rc == _lib.ERR_RANGE
    for k, c in enumerate(canvases):
      assert _same_bits(c.read_seed(), before[k][0]), k
      assert np.array_equal(c.read_segmentation(), before[k][1]), k
    got = eng.step(canvases, [reqs[k] for k in range(16)], params)
    assert eng.range_fallbacks == 1
    assert eng.get_option('conv_variant') == eng.get_option('exact_variant')
    for k, c in enumerate(cases):
      c.oc.disco_seed_threshold = params.disco_seed_threshold
      c.oc.forward_fn = (lambda a, b, out=raw[k]: out.copy())
      logits = c.oc.update_at(c.pos)
      seed_now = canvases[k].read_seed()
      assert np.array_equal(np.isnan(seed_now), np.isnan(c.oc.seed)), k
      if k == bad:
        scale = np.nanmax(np.abs(c.oc.seed))
        assert np.nanmax(np.abs(seed_now - c.oc.seed)) <= 1e-5 * scale
        assert got[k].range_error == 0
      else:
        _check_step(c, got[k], logits, fracs[k] > params.disco_seed_threshold,
                    segs[k])
        assert np.nanmax(np.abs(seed_now - c.oc.seed)) <= TOL, k
  finally:
    eng.close()


# ---------------------------------------------------------------------------
# 3. whole runs at the benchmark's batched shape
# ---------------------------------------------------------------------------


@pytest.mark.parametrize('carry', [True, False])
def test_fixture_runs_at_batch_16_in_two_groups(fib25_model, carry):
  """bench.py's batched leg (BASELINE configs[2]): HipBatchExecutor(batch 16) +
  MultiCanvasDriver(batch_size=16, groups=2, native=True): the library's segment
  loops (ffn_canvas_segment_many[_carry]) over 34 canvases of the reference-
  minted cells56 / cells72 runs, half of them u8 canvases.  Each canvas equals
  its reference run, the driver counted every step once, and full batches of
  16 really ran (stat_hist_16)."""
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.inference import seed as seed_lib
  import bench
  names = ['cells72', 'cells56'] * 17
  gold = {n: np.load(os.path.join(GOLDEN, 'ref_canvas_%s.npz' % n))
          for n in set(names)}
  request = bench.make_request()
  counters = inference_utils.Counters()
  exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                  fib25_model.info, None, counters, 16)
  canvases = []
  results = {}
  try:

    def jobs():
      for j, n in enumerate(names):
        sub = counters.get_sub_counters()
        raw = gold[n]['volume']
        image = (inference.NormalizedU8Image(raw, 128.0, 33.0) if (j // 2) % 2
                 else synthetic.normalize(raw))
        c = inference.DeviceCanvas(
            fib25_model.info, exe.get_client(sub, direct=True), image,
            request.inference_options, counters=sub,
            movement_policy_fn=movement.get_policy_fn(request, fib25_model.info))
        canvases.append((c, n))
        yield c, functools.partial(seed_lib.PolicyFixed, coords=gold[n]['seeds'])

    def on_done(c):
      results[id(c)] = (np.array(np.asarray(c.segmentation)),
                        c.counters['update_at-calls'].value)
      c.close()

    drv = inference.MultiCanvasDriver(exe.engine, batch_size=16, native=True,
                                      groups=2, carry=carry)
    assert drv.groups == 2
    drv.run(jobs(), on_done=on_done)
    assert len(canvases) == len(names) == len(results)
    total = 0
    for c, n in canvases:
      seg, calls = results[id(c)]
      assert np.array_equal(seg, gold[n]['segmentation']), n
      assert calls == len(gold[n]['steps']), n
      total += calls
    assert drv.steps == total
    assert exe.engine.get_option('stat_hist_16') > 0
    print('34 canvases, batch 16, 2 groups, carry %s: %d steps, %d full batches' % (
        carry, total, exe.engine.get_option('stat_hist_16')))
  finally:
    exe.engine.close()


def test_phantom_ensemble_batched_equals_alone(fib25_model):
  """Six 128^3 phantoms (ref_canvas_phantoms128.npz) segmented together at batch
  16 under the native driver, and each alone on a variant-8 engine: the same
  segmentation, seed logits, per-segment origins and step counts, bit for bit --
  batching changes nothing, whatever the trajectory.  The foreground IoU
  against the fixture is printed (not asserted; see test_phantom_ensemble)."""
  from ffn_amd import synthetic
  from ffn_amd.inference import executor
  from ffn_amd.inference import inference
  from ffn_amd.inference import inference_utils
  from ffn_amd.inference import movement
  from ffn_amd.inference import seed as seed_lib
  import bench
  g = np.load(os.path.join(GOLDEN, 'ref_canvas_phantoms128.npz'))
  size = int(g['size'])
  vol_seeds = [int(v) for v in g['vol_seeds'].tolist()[:6]]
  request = bench.make_request()

  def run(batch):
    counters = inference_utils.Counters()
    exe = executor.HipBatchExecutor(executor.ExecutorInterface(), fib25_model,
                                    fib25_model.info, None, counters, batch)
    out = []
    try:
      if batch == 1:
        exe.engine.set_option('conv_variant', 8)
      canvases = []
      for vs in vol_seeds:
        sub = counters.get_sub_counters()
        canvases.append(inference.DeviceCanvas(
            fib25_model.info, exe.get_client(sub, direct=True),
            synthetic.normalize(synthetic.cells_volume((size,) * 3, seed=vs)),
            request.inference_options, counters=sub,
            movement_policy_fn=movement.get_policy_fn(request, fib25_model.info)))
      policies = [functools.partial(seed_lib.PolicyFixed,
                                    coords=g['s%d/seeds' % vs].astype(np.int32))
                  for vs in vol_seeds]
      if batch == 1:
        for c, p in zip(canvases, policies):
          c.segment_all(seed_policy=p)
      else:
        drv = inference.MultiCanvasDriver(exe.engine, batch_size=batch, native=True)
        drv.run(zip(canvases, policies))
        assert exe.engine.get_option('conv_variant') == 8  # pinned
      for c in canvases:
        out.append(dict(
            seg=np.array(np.asarray(c.segmentation)),
            seed=np.array(c._handle.read_seed()),
            steps=c.counters['update_at-calls'].value,
            origins={int(k): (tuple(int(v) for v in o.start_zyx), o.iters)
                     for k, o in c.origins.items()}))
        c.close()
      assert exe.engine.range_fallbacks == 0
    finally:
      exe.engine.close()
    return out

  together = run(16)
  alone = run(1)
  for vs, a, b in zip(vol_seeds, together, alone):
    agree = bench.segmentation_agreement(a['seg'], g['s%d/segmentation' % vs])
    print('phantom %d^3 seed %d: %d steps, %d segments; IoU foreground vs fixture '
          '%.6f' % (size, vs, a['steps'], len(a['origins']), agree['iou_foreground']))
    assert a['steps'] == b['steps'], vs
    assert a['origins'] == b['origins'], vs
    assert np.array_equal(a['seg'], b['seg']), vs
    assert _same_bits(a['seed'], b['seed']), vs
