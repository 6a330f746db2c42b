"""Forward-only evaluation on the GPU (include/ffn_evaluation.h,
ffn_amd/training/evaluation.py, evaluate_checkpoint.py): every kernel of the
unit against the numpy restatement (tests/evaluation_ref.py) at the smallest
shapes that reach its paths, ffn_predict_device against ffn_predict, and
CheckpointEvaluator with the FIB-25 weights against the reference's recorded
runs (tests/golden/ref_evaluation.npz).

End-to-end figures (MI355X; S is the fixture's f32-against-f64 spread of the
final seeds, the GPU column the largest |GPU - fixture| over the sampled
seeds, in logit units; the bound on it is M / 4 = 2.5e-4): see DESIGN.md
10.4."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import evaluation_ref
from tests import test_evaluation as cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def ev():
  from ffn_amd.training import evaluation
  return evaluation


@pytest.fixture(scope='module')
def ops(ev):
  return ev.default_ops(0)


@pytest.fixture(scope='module')
def torch():
  import torch as torch_module
  return torch_module


def make_geometry(ev, seed, pred, deltas, moves, slots, extra=0, image=None):
  """zyx sizes -> Geometry; `extra` more moves in the arrays than in the eval
  box (1 = what 'max_pred_moves' has); `image`: input_image where it is not
  input_seed."""
  grow = lambda size, m: tuple(s + 2 * m * d for s, d in zip(size, deltas))
  image = seed if image is None else image
  return ev.Geometry(input_seed=seed, input_image=image, pred_mask=pred,
                     deltas=deltas, canvas=grow(seed, moves + extra),
                     image_patch=grow(image, moves + extra),
                     label_patch=grow(pred, moves + extra),
                     eval=grow(pred, moves), slots=slots)


def geom_dict(g):
  return {k: tuple(getattr(g, k)) for k in (
      'input_seed', 'input_image', 'pred_mask', 'deltas', 'canvas',
      'image_patch', 'label_patch', 'eval')}


#: name -> (input_seed, pred_mask, deltas (all zyx), fov_moves, slots)
SHAPES = {
    'anisotropic_1': ((9, 13, 17), (7, 11, 15), (1, 2, 3), 1, 5),
    'anisotropic_2': ((9, 13, 17), (7, 11, 15), (1, 2, 3), 2, 32),
    'wide_x': ((5, 7, 67), (5, 7, 67), (1, 1, 4), 1, 5),
    'below_a_wave': ((3, 3, 5), (3, 3, 5), (1, 1, 1), 1, 1),
}


def all_offsets(deltas_zyx, moves):
  """model.shifts scaled by 1 .. moves: every shift, and the extreme offsets
  +/- moves * deltas on each axis; (0, 0, 0) first."""
  shifts = evaluation_ref.model_shifts(deltas_zyx[::-1])
  out = [(0, 0, 0)]
  for m in range(1, moves + 1):
    out += [tuple(m * v for v in s) for s in shifts]
  return out


def labelled_volume(shape, label_dtype, image_dtype, seed):
  """An image and a label volume of four slabs along x and two along z whose
  ids, as uint64, differ only above bit 32; a band of background."""
  rng = np.random.RandomState(seed)
  if image_dtype == np.uint8:
    image = rng.randint(0, 256, shape).astype(np.uint8)
  else:
    image = rng.normal(100, 50, shape).astype(np.float32)
  ids = np.zeros(shape, np.uint64)
  quarter = shape[2] // 4
  for k in range(4):
    high = np.uint64(k) << np.uint64(32) if label_dtype == np.uint64 else k
    ids[:, :, k * quarter:(k + 1) * quarter] = np.uint64(7) + np.uint64(high)
  ids[shape[0] // 2:] += np.uint64(100)
  ids[:, shape[1] // 2 - 1:shape[1] // 2 + 1] = 0
  return image, ids.astype(label_dtype)


def torch_io(torch, g, n):
  """Caller-made device arrays for n FoVs: seed, image, logits."""
  make = lambda dims: torch.empty((n,) + tuple(dims), dtype=torch.float32,
                                  device='cuda:0')
  return make(g.input_seed), make(g.input_image), make(g.input_seed)


def device_array(torch, array):
  t = torch.from_numpy(np.ascontiguousarray(array)).to('cuda:0')
  torch.cuda.synchronize()
  return t


# ---- load --------------------------------------------------------------------------


@pytest.mark.parametrize('shape_name', sorted(SHAPES))
@pytest.mark.parametrize('image_dtype,label_dtype', [
    (np.uint8, np.uint64), (np.float32, np.uint32), (np.uint8, np.int64)])
def test_load_is_bit_equal_to_numpy(ev, ops, shape_name, image_dtype,
                                    label_dtype):
  seed, pred, deltas, moves, slots = SHAPES[shape_name]
  g = make_geometry(ev, seed, pred, deltas, moves, slots)
  gd = geom_dict(g)
  ops.configure(g)
  ops.reset()
  # three different extents, room for a few centres
  shape = tuple(s + e for s, e in zip(g.image_patch, (5, 9, 13)))
  image, labels = labelled_volume(shape, label_dtype, image_dtype, 3)
  other = labelled_volume(tuple(s + 2 for s in shape), label_dtype,
                          image_dtype, 4)
  vols = [ops.add_volume(image, labels), ops.add_volume(*other)]
  data = [(image, labels), other]
  lo = [(s - 1) // 2 for s in g.image_patch]              # first centre, zyx
  hi = [n - s + (s - 1) // 2 for n, s in zip(shape, g.image_patch)]  # last
  rng = np.random.RandomState(5)
  centres_zyx = [tuple(lo), tuple(hi),
                 (lo[0] + 1, shape[1] // 2 - 1, lo[2] + 2)]  # centre label 0
  while len(centres_zyx) < min(slots, 6):
    centres_zyx.append(tuple(int(rng.randint(l, h + 1))
                             for l, h in zip(lo, hi)))
  centres_zyx = centres_zyx[:slots]
  n = len(centres_zyx)
  which = [k % 2 for k in range(n)]
  for k in range(n):  # the second volume is larger: keep its centres inside
    assert all(c <= h for c, h in zip(centres_zyx[k], hi))
  centres = [c[::-1] for c in centres_zyx]
  offsets = [100.0 + k for k in range(n)]
  scales = [33.0 - 0.5 * k for k in range(n)]
  slot_ids = list(range(n))[::-1]
  ops.load(slot_ids, [vols[w] for w in which], centres, offsets, scales, 0.05)
  for k, s in enumerate(slot_ids):
    want = evaluation_ref.load(*data[which[k]], centres[k], offsets[k],
                               scales[k], gd, 0.05)
    assert np.array_equal(ops.read_image(s), want[0]), k
    assert np.array_equal(ops.read_labels(s), want[1]), k
    assert np.array_equal(ops.read_seed(s), want[2]), k
  if n > 2:
    assert (ops.read_labels(slot_ids[2]) == np.float32(0.05)).all()
  # one past the last position that fits, on each axis: refused, slot untouched
  before = [ops.read_image(0), ops.read_labels(0), ops.read_seed(0)]
  for axis in range(3):
    for past in (hi[axis] + 1, lo[axis] - 1):
      c = list(centres_zyx[0])
      c[axis] = past
      with pytest.raises(Exception, match='leave volume'):
        ops.load([0], [vols[0]], [c[::-1]], [0.0], [1.0], 0.05)
  after = [ops.read_image(0), ops.read_labels(0), ops.read_seed(0)]
  assert all(np.array_equal(a, b) for a, b in zip(before, after))


def test_load_compares_labels_on_all_64_bits(ev, ops):
  g = make_geometry(ev, (3, 3, 5), (3, 3, 5), (1, 1, 1), 1, 1)
  ops.configure(g)
  ops.reset()
  shape = (5, 5, 7)
  labels = np.full(shape, 9, np.uint64)
  labels[:, :, 4:] = 9 + (1 << 32)   # same low word
  labels[:, :, 0] = 9 + (1 << 63)
  vol = ops.add_volume(np.zeros(shape, np.uint8), labels)
  ops.load([0], [vol], [(3, 2, 2)], [0.0], [1.0], 0.05)
  want = evaluation_ref.load(np.zeros(shape, np.uint8), labels, (3, 2, 2), 0.0,
                             1.0, geom_dict(g))[1]
  got = ops.read_labels(0)
  assert np.array_equal(got, want)
  assert (got[:, :, 1:4] == np.float32(0.95)).all()
  assert (got[:, :, 4:] == np.float32(0.05)).all()
  assert (got[:, :, 0] == np.float32(0.05)).all()


# ---- gather / paste ----------------------------------------------------------------


def filled_slots(ev, ops, g, seed):
  """Every slot loaded from one random volume and given a random seed canvas;
  returns the per-slot [image, labels, seed] restatement arrays."""
  ops.configure(g)
  ops.reset()
  rng = np.random.RandomState(seed)
  shape = tuple(s + 4 for s in g.image_patch)
  image, labels = labelled_volume(shape, np.uint64, np.uint8, seed)
  vol = ops.add_volume(image, labels)
  lo = [(s - 1) // 2 for s in g.image_patch]
  centres = [tuple(int(l + rng.randint(0, 5)) for l in lo)[::-1]
             for _ in range(g.slots)]
  ops.load(list(range(g.slots)), [vol] * g.slots, centres, [128.0] * g.slots,
           [33.0] * g.slots, 0.05)
  state = []
  for s in range(g.slots):
    arrays = list(evaluation_ref.load(image, labels, centres[s], 128.0, 33.0,
                                      geom_dict(g)))
    arrays[2] = rng.permutation(arrays[2].size).astype(np.float32).reshape(
        g.canvas) * np.float32(0.37) - np.float32(50)
    ops.write_seed(s, arrays[2])
    state.append(arrays)
  return state


@pytest.mark.parametrize('shape_name', sorted(SHAPES))
def test_gather_and_paste_at_every_shift(ev, ops, torch, shape_name):
  seed, pred, deltas, moves, slots = SHAPES[shape_name]
  g = make_geometry(ev, seed, pred, deltas, moves, slots)
  gd = geom_dict(g)
  state = filled_slots(ev, ops, g, 11)
  offsets = all_offsets(deltas, moves)
  rng = np.random.RandomState(12)
  seed_io, image_io, _ = torch_io(torch, g, slots)
  lo = [(a - p) // 2 for a, p in zip(seed, pred)]
  box = tuple(slice(l, l + p) for l, p in zip(lo, pred))
  for start in range(0, len(offsets), slots):
    # different offsets for the slots of one call, the slots in a shuffled order
    chunk = offsets[start:start + slots]
    slot_ids = [int(s) for s in rng.permutation(slots)[:len(chunk)]]
    n = len(chunk)
    seed_io.fill_(-1.0)
    image_io.fill_(-1.0)
    torch.cuda.synchronize()
    ops.gather(slot_ids, chunk, seed_io, image_io)
    got_seed = seed_io.cpu().numpy()
    got_image = image_io.cpu().numpy()
    for k, (s, off) in enumerate(zip(slot_ids, chunk)):
      assert np.array_equal(got_seed[k],
                            evaluation_ref.crop(state[s][2], off, seed)), off
      assert np.array_equal(got_image[k],
                            evaluation_ref.crop(state[s][0], off, seed)), off
    assert (got_seed[n:] == -1.0).all() and (got_image[n:] == -1.0).all()
    # caller-made logits, distinct per voxel, in both layouts; the canvases are
    # compared after each paste: the window, and everything outside it unchanged
    for layout in (ev.EvaluationOps.LOGITS_PRED, ev.EvaluationOps.LOGITS_FOV):
      dims = pred if layout == ev.EvaluationOps.LOGITS_PRED else seed
      logits = (rng.permutation(n * int(np.prod(dims))).astype(np.float32)
                .reshape((n,) + dims) * np.float32(0.01) +
                np.float32(start + 1000 * layout))
      ops.paste(slot_ids, chunk, device_array(torch, logits), layout)
      for k, (s, off) in enumerate(zip(slot_ids, chunk)):
        evaluation_ref.paste(
            state[s][2], off,
            logits[k] if layout == ev.EvaluationOps.LOGITS_PRED
            else logits[k][box], gd)
      for s in range(slots):
        assert np.array_equal(ops.read_seed(s), state[s][2]), (start, s, layout)
  # one step past the extreme offset leaves the canvas: refused
  past = (0, 0, -(moves + 1) * deltas[0])
  with pytest.raises(Exception, match='out of its array'):
    ops.gather([0], [past], seed_io, image_io)
  with pytest.raises(Exception, match='out of its array'):
    ops.paste([0], [past], seed_io, ev.EvaluationOps.LOGITS_FOV)
  if slots > 1:
    with pytest.raises(Exception, match='twice'):
      ops.paste([0, 0], [(0, 0, 0)] * 2, seed_io, ev.EvaluationOps.LOGITS_FOV)
  assert np.array_equal(ops.read_seed(0), state[0][2])


def test_gather_with_an_image_box_that_is_not_the_seed_box(ev, ops, torch):
  seed, image, pred, deltas, moves, slots = (
      (5, 7, 9), (7, 11, 15), (5, 7, 9), (1, 2, 3), 2, 5)
  g = make_geometry(ev, seed, pred, deltas, moves, slots, image=image)
  assert g.image_patch != g.canvas
  state = filled_slots(ev, ops, g, 13)
  for s in range(slots):  # load with two patch sizes
    assert np.array_equal(ops.read_image(s), state[s][0])
    assert np.array_equal(ops.read_labels(s), state[s][1])
  offsets = all_offsets(deltas, moves)
  seed_io, image_io, _ = torch_io(torch, g, slots)
  assert tuple(image_io.shape[1:]) == image and tuple(seed_io.shape[1:]) == seed
  for start in range(0, len(offsets), slots):
    chunk = offsets[start:start + slots]
    slot_ids = list(range(len(chunk)))[::-1]
    ops.gather(slot_ids, chunk, seed_io, image_io)
    got_seed = seed_io.cpu().numpy()
    got_image = image_io.cpu().numpy()
    for k, (s, off) in enumerate(zip(slot_ids, chunk)):
      assert np.array_equal(got_seed[k],
                            evaluation_ref.crop(state[s][2], off, seed)), off
      assert np.array_equal(got_image[k],
                            evaluation_ref.crop(state[s][0], off, image)), off


# ---- probe_moves -------------------------------------------------------------------


@pytest.mark.parametrize('shape_name', ['anisotropic_2', 'wide_x',
                                        'below_a_wave'])
def test_probe_moves_at_and_below_the_thresholds(ev, ops, shape_name):
  seed, pred, deltas, moves, slots = SHAPES[shape_name]
  g = make_geometry(ev, seed, pred, deltas, moves, slots)
  state = filled_slots(ev, ops, g, 21)
  offsets = all_offsets(deltas, moves)
  thr = ev.logit(0.9)
  label_thr = ev.expit(thr)
  at = ev.ceil_f32(thr)
  below = np.nextafter(at, np.float32(-np.inf))
  rng = np.random.RandomState(22)
  for s in range(slots):
    canvas = state[s][2]
    for k, off in enumerate(offsets):
      pos = tuple(c // 2 + o for c, o in zip(g.canvas, off[::-1]))
      canvas[pos] = (at, below, np.float32(3.0), np.float32(-3.0))[
          (k + s + int(rng.randint(2))) % 4]
    ops.write_seed(s, canvas)
  pairs = [(s, off) for s in range(slots) for off in offsets]
  if slots == 32:
    assert len(pairs) > 256  # more than one workgroup
  valid, wanted = ops.probe_moves([s for s, _ in pairs], [o for _, o in pairs],
                                  thr, label_thr)
  want = [evaluation_ref.probe(state[s][2], state[s][1], off, thr, label_thr)
          for s, off in pairs]
  assert valid.tolist() == [v for v, _ in want]
  assert wanted.tolist() == [w for _, w in want]
  values = np.array([state[s][2][tuple(c // 2 + o for c, o in
                                       zip(g.canvas, off[::-1]))]
                     for s, off in pairs])
  assert valid[values == at].all() and not valid[values == below].any()
  assert (values == at).any() and (values == below).any()
  assert wanted.any() and not wanted.all()
  # the soft label itself as the threshold: >= holds at equality
  _, w2 = ops.probe_moves([0], [(0, 0, 0)], float(at),
                          float(np.float32(0.95)))
  centre = state[0][1][tuple(s // 2 for s in g.label_patch)]
  assert bool(w2[0]) == bool(centre == np.float32(0.95))
  with pytest.raises(Exception, match='out of its array'):
    ops.probe_moves([0], [(g.canvas[2], 0, 0)], thr, label_thr)


# ---- score_faces -------------------------------------------------------------------


@pytest.mark.parametrize('shape_name', sorted(SHAPES))
def test_score_faces_ties_and_scores(ev, ops, shape_name):
  seed, pred, deltas, moves, slots = SHAPES[shape_name]
  g = make_geometry(ev, seed, pred, deltas, moves, slots)
  state = filled_slots(ev, ops, g, 31)
  rng = np.random.RandomState(32)
  n = min(slots, 4)
  offsets = [all_offsets(deltas, moves)[-1 - k] for k in range(n)]
  # slot 0: random distinct values (from filled_slots); slot 1: few distinct
  # values, many ties per face; slot 2: one constant (every face all tied, the
  # first position wins); slot 3: everything below the threshold
  if n > 1:
    state[1][2] = rng.randint(0, 3, g.canvas).astype(np.float32)
  if n > 2:
    state[2][2] = np.full(g.canvas, 4.5, np.float32)
  if n > 3:
    state[3][2] = (rng.permutation(int(np.prod(g.canvas))).reshape(g.canvas)
                   .astype(np.float32) * np.float32(-0.01) - np.float32(3))
  if n == 1:
    state[0][2] = rng.randint(0, 2, g.canvas).astype(np.float32)
  for s in range(n):
    ops.write_seed(s, state[s][2])
  scores, positions = ops.score_faces(list(range(n)), offsets)
  for s in range(n):
    want_s, want_p = evaluation_ref.face_scores(
        evaluation_ref.crop(state[s][2], offsets[s], pred), deltas)
    assert np.array_equal(scores[s], want_s), s
    assert np.array_equal(positions[s], want_p), s
  if n > 2:
    first = [[-d if a != f // 2 else (d if f % 2 else -d)
              for a, d in enumerate(deltas)] for f in range(6)]
    assert positions[2].tolist() == first
  if n > 3:  # nothing reaches the threshold: the policy queues nothing
    assert (scores[3] < ev.ceil_f32(ev.logit(0.9))).all()


# ---- finish ------------------------------------------------------------------------

FINISH_SHAPES = {
    # (seed, pred, deltas, moves, slots, extra): extra = 1 makes the eval box
    # smaller than the label patch and the canvas
    'anisotropic_eval_inside': ((9, 13, 17), (7, 11, 15), (1, 2, 3), 1, 5, 1),
    'wide_x': ((5, 7, 67), (5, 7, 67), (1, 1, 4), 1, 5, 0),
    'below_a_wave': ((3, 3, 5), (3, 3, 5), (1, 1, 1), 1, 1, 0),
    # 49^3 eval voxels inside 65^3 arrays: many workgroups
    'fib25_max_pred': ((33, 33, 33), (33, 33, 33), (8, 8, 8), 1, 1, 1),
}


@pytest.mark.parametrize('shape_name', sorted(FINISH_SHAPES))
def test_finish_counts_exactly_and_sums_the_loss(ev, ops, shape_name):
  seed, pred, deltas, moves, slots, extra = FINISH_SHAPES[shape_name]
  g = make_geometry(ev, seed, pred, deltas, moves, slots, extra)
  gd = geom_dict(g)
  if extra:
    assert all(e < l for e, l in zip(g.eval, g.label_patch))
  state = filled_slots(ev, ops, g, 41)
  rng = np.random.RandomState(42)
  at = ev.ceil_f32(ev.logit(0.9))
  below = np.nextafter(at, np.float32(-np.inf))
  special_values = np.array([at, below, 80.0, -80.0, 0.0], np.float32)
  voxels = int(np.prod(g.eval))
  for s in range(slots):
    canvas = rng.normal(0, 4, g.canvas).astype(np.float32)
    pick = rng.rand(*g.canvas) < 0.3
    canvas[pick] = special_values[rng.randint(0, 5, int(pick.sum()))]
    state[s][2] = canvas
    ops.write_seed(s, canvas)
    loss, counts, masked = ops.finish(s)
    want_loss, want_counts, _ = evaluation_ref.finish(canvas, state[s][1], gd)
    assert counts == want_counts, s
    assert sum(counts) == voxels and masked == 0
    assert np.isfinite(loss)
    # N <= 2^18 positive terms, a tree reduction and ~2-ulp exp / log1p:
    # (log2 N + 8) 2^-24 ~ 1.5e-6; x6 leaves room
    assert abs(loss - want_loss) <= 1e-5 * want_loss, (loss, want_loss)
    assert ops.finish(s)[0] == loss  # the same tree every time
  labels = state[0][1]
  assert set(np.unique(labels)) <= {np.float32(0.05), np.float32(0.95)}
  box = evaluation_ref.crop(state[0][2], (0, 0, 0), g.eval)
  assert (box == at).any() and (box == below).any() and (box == 80.0).any()


# ---- ffn_predict_device ------------------------------------------------------------


def test_predict_device_is_bit_equal_to_predict(torch):
  from ffn_amd import engine as hip_engine
  from ffn_amd.training.models import convstack_3d
  model = convstack_3d.ConvStack3DFFNModel(fov_size=[33, 33, 33],
                                           deltas=[8, 8, 8], depth=2)
  model.init_random(seed=3, stddev=0.05)
  eng = hip_engine.HipEngine.from_model(model, max_batch=16, device_id=0)
  try:
    rng = np.random.RandomState(4)
    seed = rng.normal(0, 2, (16, 33, 33, 33)).astype(np.float32)
    image = rng.normal(0, 1, (16, 33, 33, 33)).astype(np.float32)
    d_seed = device_array(torch, seed)
    d_image = device_array(torch, image)
    d_logits = torch.full((16, 33, 33, 33), -7.0, dtype=torch.float32,
                          device='cuda:0')
    torch.cuda.synchronize()
    for n in (1, 3, 16):
      want = eng.predict(seed[:n], image[:n])
      eng.predict_device(n, d_seed, d_image, d_logits)
      got = d_logits.cpu().numpy()
      assert np.array_equal(got[:n], want), n
      assert (got[n:] == -7.0).all()
      # the outputs of a call as the next call's seed, written in place
      again = eng.predict(want, image[:n])
      eng.predict_device(n, d_logits, d_image, d_logits)
      assert np.array_equal(d_logits.cpu().numpy()[:n], again), n
      d_logits.fill_(-7.0)
      torch.cuda.synchronize()
    with pytest.raises(Exception):
      eng.predict_device(17, d_seed, d_image, d_logits)
  finally:
    eng.close()


# ---- end to end --------------------------------------------------------------------

_engines = {}


def fib25_engine(fib25_model, batch_size):
  from ffn_amd import engine as hip_engine
  if batch_size not in _engines:
    _engines[batch_size] = hip_engine.HipEngine.from_model(
        fib25_model, max_batch=batch_size, device_id=0)
  return _engines[batch_size]


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
  yield
  for eng in _engines.values():
    eng.close()
  _engines.clear()


@pytest.mark.parametrize('batch_size', [1, 4, 16])
@pytest.mark.parametrize('name', cpu.CASES)
def test_evaluator_reproduces_the_reference_run(ev, ops, fib25_model, name,
                                                batch_size):
  case = cpu.FIXTURE['cases'][name]
  M = cpu.FIXTURE['M']
  evaluator = ev.CheckpointEvaluator(
      fib25_model, fib25_engine(fib25_model, batch_size), ops, case['policy'],
      case['fov_moves'], batch_size=batch_size)
  for vol_name, v in cpu.fixture_volumes().items():
    evaluator.add_volume(vol_name, *v)
  seeds = {}
  finish = ops.finish

  def keeping(slot, *args):  # the final seed of the example the slot holds
    seeds[len(seeds)] = (ops.read_seed(slot), ops.read_image(slot).tobytes())
    return finish(slot, *args)

  ops.finish = keeping
  try:
    result = evaluator.evaluate(case['coordinates'])
  finally:
    del ops.finish
  assert result.skipped == 0
  assert result.offsets == case['offsets']
  assert result.records == case['records']
  assert result.moves == case['moves'].tolist()
  assert list(result.moves_by_r) == case['radii'].tolist()
  for k, r in enumerate(case['radii']):
    assert result.moves_by_r[int(r)] == case['moves_by_r'][k].tolist()
  assert result.num_patches == int(case['num_patches'][0])
  assert result.num_voxels == case['num_voxels'].tolist()
  assert result.fov_stats == [float(v) for v in case['fov_stats']]
  assert sum(result.prediction_counts) == int(case['num_voxels'][0])
  for got, want in zip(result.prediction_counts, case['prediction_counts']):
    print('%s batch %d: count %d, fixture %d, n_near %d' % (
        name, batch_size, got, want, case['n_near']))
    assert abs(got - int(want)) <= case['n_near']
  # examples finish in another order than they start when the batch holds
  # several: match each final seed to its example by the image it was cut from
  volumes = cpu.fixture_volumes()
  geom = cpu.case_geometry(case)
  images = [evaluation_ref.load(*volumes[n][:2], c, volumes[n][2],
                                volumes[n][3], geom)[0].tobytes()
            for c, n in case['coordinates']]
  assert len(set(images)) == len(images)
  worst = 0.0
  for seed, image in seeds.values():
    k = images.index(image)
    worst = max(worst, float(np.abs(
        evaluation_ref.sample_seed(seed).astype(np.float64) -
        case['seeds'][k]).max()))
  assert len(seeds) == len(case['coordinates'])
  loss_rel = abs(result.loss - float(case['loss'][0])) / float(case['loss'][0])
  print('%s batch %d: S %.3g, GPU distance %.3g (bound %.3g), loss rel %.3g' % (
      name, batch_size, case['S'], worst, M / 4, loss_rel))
  assert worst <= M / 4
  assert loss_rel <= 1e-3


def test_script_end_to_end_equals_the_evaluator(ev, ops, fib25_model, tmp_path):
  """evaluate_checkpoint.py on .npy volumes and a TFRecord file written by
  build_coordinates.py."""

  def script(name):
    spec = importlib.util.spec_from_file_location(
        name + '_script', os.path.join(ROOT, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod

  volumes = cpu.fixture_volumes()
  image, labels, offset, scale = volumes['a']
  np.save(tmp_path / 'image.npy', image)
  np.save(tmp_path / 'labels.npy', labels)
  partitions = np.where(labels > 0, 1, 0).astype(np.uint8)
  partitions[:45] = partitions[48:] = 255  # a thin slab: a small file
  coords = str(tmp_path / 'coords')
  script('build_coordinates').build_coordinates(
      [('a', partitions)], (30, 30, 30), coords, seed=5)
  out = str(tmp_path / 'out.json')
  weights = os.path.join(ROOT, 'tests', 'golden', 'fib25_weights.npz')
  argv = ['--train_coords', coords,
          '--data_volumes', 'a:%s' % (tmp_path / 'image.npy'),
          '--label_volumes', 'a:%s' % (tmp_path / 'labels.npy'),
          '--model_args',
          '{"depth": 12, "fov_size": [33, 33, 33], "deltas": [8, 8, 8]}',
          '--checkpoint', weights, '--image_mean', str(offset),
          '--image_stddev', str(scale), '--batch_size', '4',
          '--max_examples', '5', '--output', out]
  result = script('evaluate_checkpoint').main(argv)
  with open(out) as f:
    written = json.load(f)
  assert written['examples'] == 5 and result.num_patches == 5
  from ffn_amd import coordinates
  centres, names = coordinates.read_tfrecord(coords)
  evaluator = ev.CheckpointEvaluator(
      fib25_model, fib25_engine(fib25_model, 4), ops, 'fixed', 1, batch_size=4)
  evaluator.add_volume('a', image, labels, offset, scale)
  direct = evaluator.evaluate(zip(centres.tolist(), names), max_examples=5)
  assert written['accumulators'] == json.loads(json.dumps(
      direct.accumulators()))
  assert written['summaries'] == json.loads(json.dumps(direct.summaries()))
  assert written['skipped'] == direct.skipped
  assert direct.offsets == result.offsets and sum(direct.moves) > 5
