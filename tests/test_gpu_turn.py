"""The between-segment turn on the device (ffn_canvas_segment_turn,
ffn_canvas_commit_count; ffn_amd/csrc/ffn_canvas_kernels.h) at the sizes where its
kernels take another path: rows of the commit box dealt to waves (x extents around
a wave's 64 lanes, boxes at the canvas faces, one voxel thick), the overlap
histogram in LDS up to kTurnHistLds = 4096 bins and in global memory above, the
partial sums instead of atomics, pick + clear + seed in one launch (box and linear
clear, the chosen voxel inside / outside / without a dirty box), the record polled
from pinned memory, and the scratch that has to be clean from one turn to the next.

Expected values: the numpy statement of the turn (tests/emulated_device.py; with a
restrictor, the handle of tests/restriction_ref.py).  Integer work and comparisons:
every returned field and the whole seed and segmentation volumes afterwards are
compared exactly.  No canvas has more voxels than 48 x 40 x 52; the canvases for the
x extents are 12 x 20 x 70, because a row of 65 voxels has to fit."""
import ctypes

import numpy as np
import pytest

from ffn_amd import _lib
from tests import restriction_ref
from tests.emulated_device import EmulatedHandle

pytestmark = pytest.mark.gpu

THR = 0.4054652154
INIT = 2.9444387
HIST_LDS = 4096  # kTurnHistLds: max_existing_id + 1 <= this counts in LDS


@pytest.fixture(scope='module')
def engine(fib25_model):
  from ffn_amd import engine as hip_engine
  eng = hip_engine.HipEngine.from_model(fib25_model, max_batch=1, device_id=0)
  yield eng
  eng.close()


class _RestrictRef(restriction_ref.RestrictShimHandle):
  """The reference turn with a restrictor (flag 4), without the host-loop shim
  the class otherwise drives: only its segment_turn is used here."""

  def __init__(self, image):  # pylint:disable=super-init-not-called
    EmulatedHandle.__init__(self, image)
    self.bits = None
    self.flag4 = 0


def _volumes(rng, shape, ids, density=0.3):
  """seed with NaNs and values on both sides of THR; seg with 0, -1 and `ids`."""
  seed = rng.normal(0, 2, shape).astype(np.float32)
  seed[rng.rand(*shape) < 0.3] = np.nan
  seg = np.zeros(shape, np.int32)
  m = rng.rand(*shape) < density
  seg[m] = rng.choice(np.asarray(ids, np.int32), int(m.sum()))
  seg[rng.rand(*shape) < 0.02] = -1
  return seed, seg


def _pair(engine, shape, seed, seg, dirty='all', ref_cls=EmulatedHandle):
  """A device canvas and its numpy double in the same state.  dirty: 'all' (the seed
  written everywhere: the linear clear), a (lo, hi) box (init_seed, then the seed
  written in the box only: the box clear), or None (untouched: no dirty box)."""
  image = np.zeros(shape, np.float32)
  canvas = engine.create_canvas(image)
  emu = ref_cls(image)
  if dirty == 'all':
    canvas.write_seed((0, 0, 0), shape, seed)
    emu.seed[...] = seed
  elif dirty is not None:
    lo, hi = dirty
    sel = tuple(slice(l, h) for l, h in zip(lo, hi))
    canvas.init_seed(lo, 0.5)
    emu.init_seed(lo, 0.5)
    canvas.write_seed(lo, hi, seed[sel])
    emu.seed[sel] = seed[sel]
  canvas.write_segmentation((0, 0, 0), shape, seg)
  emu.seg[...] = seg
  return canvas, emu


def _check_turn(canvas, emu, commit, mark, cands, mbd, init, tag=''):
  got = canvas.segment_turn(commit, mark, cands, mbd, init)
  want = emu.segment_turn(commit, mark, cands, mbd, init)
  assert got[0] == want[0] and got[1] == want[1], (tag, got[:2], want[:2])
  assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), tag
  assert got[2].dtype == np.int32 and got[3].dtype == np.int64
  assert got[4] == want[4] and got[5] == want[5], (tag, got[4:6], want[4:6])
  assert np.array_equal(got[6], want[6]), (tag, got[6], want[6])
  assert np.array_equal(got[7], want[7], equal_nan=True), tag
  assert np.array_equal(got[8], want[8]), tag
  assert np.array_equal(canvas.read_segmentation(), emu.seg), tag
  assert np.array_equal(canvas.read_seed(), emu.seed, equal_nan=True), tag
  return want


def _cands(rng, shape, n, lo=None, hi=None):
  lo = lo or (0, 0, 0)
  hi = hi or shape
  return np.stack([rng.randint(l, h, n) for l, h in zip(lo, hi)],
                  axis=1).astype(np.int32).reshape(-1, 3)


XSHAPE = (12, 20, 70)


def _commit_boxes():
  z, y, x = XSHAPE
  boxes = [('x%d' % w, (1, 2, 3), (11, 19, 3 + w)) for w in (1, 3, 63, 64, 65)]
  boxes += [('face_z0', (0, 3, 5), (7, 17, 40)), ('face_z1', (4, 3, 5), (z, 17, 40)),
            ('face_y0', (2, 0, 5), (9, 11, 40)), ('face_y1', (2, 6, 5), (9, y, 40)),
            ('face_x0', (2, 3, 0), (9, 17, 33)), ('face_x1', (2, 3, 30), (9, 17, x)),
            ('thin_z', (5, 1, 2), (6, 19, 69)), ('thin_y', (1, 7, 2), (11, 8, 69)),
            ('thin_x', (1, 1, 37), (11, 19, 38)), ('whole', (0, 0, 0), XSHAPE)]
  return boxes


@pytest.mark.parametrize('name,lo,hi', _commit_boxes(),
                         ids=[b[0] for b in _commit_boxes()])
def test_commit_boxes(engine, name, lo, hi):
  """Count, overlaps and assignment over boxes of every row shape: the count
  alone (ffn_canvas_commit_count), then the turn that assigns."""
  rng = np.random.RandomState(len(name) * 131 + sum(hi))
  seed, seg = _volumes(rng, XSHAPE, [1, 2, 3, 9, 40, 41])
  canvas, emu = _pair(engine, XSHAPE, seed, seg)
  raw, actual, ids, counts = canvas.commit_count(lo, hi, THR, 40)
  wraw, wactual, wids, wcounts = emu.commit_count(lo, hi, THR, 40)
  keep = wids <= 40
  assert (raw, actual) == (wraw, wactual)
  assert np.array_equal(ids, wids[keep]) and np.array_equal(counts, wcounts[keep])
  cands = _cands(rng, XSHAPE, 5)
  want = _check_turn(canvas, emu, (lo, hi, THR, 0, 77, 40), None, cands, (1, 1, 1),
                     INIT, name)
  assert want[4]  # committed
  assert want[1] == 0 or np.any(emu.seg == 77)
  canvas.close()


SHAPE = (48, 40, 52)


@pytest.mark.parametrize('max_id', [HIST_LDS - 2, HIST_LDS - 1, HIST_LDS, 20000])
def test_overlap_histogram_bounds(engine, max_id):
  """max_existing_id below the LDS table's bound, at it (max_id + 1 = 4096) and
  above it (per-voxel global atomics), ids spread over the whole range and some
  above max_id (counted as raw, not as overlaps)."""
  rng = np.random.RandomState(max_id)
  ids = np.concatenate([[1, 2, max_id - 1, max_id, max_id + 1, max_id + 7],
                        rng.randint(1, max_id + 1, 3000)])
  seed, seg = _volumes(rng, SHAPE, ids)
  # both ends of the range, and an id just past it, above the threshold in the box
  seed[5, 5, 5:8] = 3.0
  seg[5, 5, 5:8] = (1, max_id, max_id + 1)
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  lo, hi = (1, 0, 2), (47, 40, 51)
  raw, actual, got_ids, counts = canvas.commit_count(lo, hi, THR, max_id)
  wraw, wactual, wids, wcounts = emu.commit_count(lo, hi, THR, max_id)
  keep = wids <= max_id
  assert (raw, actual) == (wraw, wactual)
  assert np.array_equal(got_ids, wids[keep]) and np.array_equal(counts, wcounts[keep])
  assert got_ids[0] == 1 and got_ids[-1] == max_id and len(got_ids) > 1000
  want = _check_turn(canvas, emu, (lo, hi, THR, 0, max_id + 100, max_id), None,
                     _cands(rng, SHAPE, 3), (0, 0, 0), INIT, max_id)
  assert np.array_equal(want[2], wids[keep])
  canvas.close()


def test_more_overlaps_than_the_caller_takes(engine):
  """max_overlaps below the number of overlapped ids: the count stays exact, the
  list is the first max_overlaps pairs in ascending id order; both entry points."""
  rng = np.random.RandomState(3)
  seed, seg = _volumes(rng, SHAPE, np.arange(1, 400))
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  lo, hi = (0, 0, 0), SHAPE
  _, _, wids, wcounts = emu.commit_count(lo, hi, THR, 399)
  assert len(wids) > 300
  i3 = lambda v: (ctypes.c_int32 * 3)(*[int(x) for x in v])
  for cap in (0, 1, 7, 64):
    ids = np.full(cap + 2, -5, np.int32)
    cnts = np.full(cap + 2, -5, np.int64)
    cc = _lib.CommitCounts()
    assert canvas._lib.ffn_canvas_commit_count(
        canvas._h, i3(lo), i3(hi), THR, 399, ctypes.byref(cc), cap, ids.ctypes.data,
        cnts.ctypes.data) == 0
    assert cc.num_overlapped_ids == len(wids)
    assert np.array_equal(ids[:cap], wids[:cap]) and np.all(ids[cap:] == -5)
    assert np.array_equal(cnts[:cap], wcounts[:cap]) and np.all(cnts[cap:] == -5)
    rq = _lib.TurnRequest()
    rq.do_commit = 1
    rq.lo[:] = lo
    rq.hi[:] = hi
    rq.segment_threshold = THR
    rq.min_segment_size = 10 ** 9  # (nothing assigned: the canvas stays as it is)
    rq.segment_id = 500
    rq.max_existing_id = 399
    ids[:] = -5
    cnts[:] = -5
    res = _lib.TurnResult()
    assert canvas._lib.ffn_canvas_segment_turn(
        canvas._h, ctypes.byref(rq), None, ctypes.byref(res), cap, ids.ctypes.data,
        cnts.ctypes.data, None, None, None) == 0
    assert res.counts.num_overlapped_ids == len(wids)
    assert res.committed == 0 and res.chosen == -1
    assert np.array_equal(ids[:cap], wids[:cap]) and np.all(ids[cap:] == -5)
    assert np.array_equal(cnts[:cap], wcounts[:cap]) and np.all(cnts[cap:] == -5)
  assert np.array_equal(canvas.read_segmentation(), emu.seg)
  canvas.close()


@pytest.mark.parametrize('above', [0, 1])
def test_min_segment_size_at_the_count(engine, above):
  """min_segment_size equal to the actual count commits; one above it does not,
  and the too-small marker (mode 2) lands."""
  rng = np.random.RandomState(11 + above)
  seed, seg = _volumes(rng, SHAPE, [1, 2, 3])
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  lo, hi = (3, 5, 7), (45, 33, 50)
  actual = emu.commit_count(lo, hi, THR, 3)[1]
  assert actual > 1000
  free = np.argwhere(seg == 0)
  mark_pos = tuple(int(v) for v in free[rng.randint(len(free))])
  want = _check_turn(canvas, emu, (lo, hi, THR, actual + above, 9, 3), (mark_pos, 2),
                     _cands(rng, SHAPE, 4), (1, 1, 1), INIT, above)
  assert want[4] == (above == 0) and want[1] == actual
  if above:
    assert emu.seg[mark_pos] == -1 and not np.any(emu.seg == 9)
  canvas.close()


def test_marker_on_a_voxel_the_commit_assigns(engine):
  """Mode 1 at a free voxel above the threshold inside the box: the commit comes
  first, so the voxel carries the id and no marker."""
  rng = np.random.RandomState(21)
  seed, seg = _volumes(rng, SHAPE, [1, 2])
  pos = (20, 20, 20)
  seed[pos], seg[pos] = 3.0, 0
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  _check_turn(canvas, emu, ((2, 2, 2), (40, 38, 50), THR, 0, 9, 2), (pos, 1), (),
              (0, 0, 0), None)
  assert emu.seg[pos] == 9
  canvas.close()


@pytest.mark.parametrize('n', [0, 1, 64, 65, 200])
def test_candidate_counts(engine, n):
  """0, 1, 64, 65 and 200 candidates on a canvas where most are segmented or too
  close, so that the chosen one lies deep in the list (or there is none)."""
  rng = np.random.RandomState(40 + n)
  seed, seg = _volumes(rng, SHAPE, [1, 2, 3], density=(0.02 if n > 1 else 0.0005))
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  cands = _cands(rng, SHAPE, n)
  want = _check_turn(canvas, emu, ((3, 5, 7), (45, 33, 50), THR, 0, 77, 3), None, cands,
                     (1, 1, 1), INIT, n)
  if n == 0:
    assert want[5] == -1
  # the canvas goes on as after init_seed: one more (plain) init elsewhere
  canvas.init_seed((20, 20, 20), 1.0)
  out = canvas.read_seed()
  assert np.isnan(out).sum() == out.size - 1 and out[20, 20, 20] == 1.0
  canvas.close()


def test_last_of_many_candidates_is_chosen(engine):
  """The only candidate that passes sits at index 64 / 199: the second ballot."""
  rng = np.random.RandomState(7)
  for n in (65, 200):
    seed, seg = _volumes(rng, SHAPE, [1, 2, 3], density=0.0)
    seg[:, :, :26] = 5  # candidates in there are segmented, the ones next to it close
    canvas, emu = _pair(engine, SHAPE, seed, seg)
    cands = _cands(rng, SHAPE, n, hi=(48, 40, 27))
    cands[-1] = (30, 30, 40)
    want = _check_turn(canvas, emu, None, None, cands, (1, 1, 1), INIT, n)
    assert want[5] == n - 1 and set(want[6][:-1]) <= {1, 2}
    canvas.close()


def test_no_candidate_passes(engine):
  """Every candidate segmented or too close: chosen -1, too-close ones marked,
  nothing cleared although a seed value was given."""
  rng = np.random.RandomState(8)
  seed, seg = _volumes(rng, SHAPE, [1, 2, 3], density=0.5)
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  want = _check_turn(canvas, emu, None, None, _cands(rng, SHAPE, 70), (2, 2, 2), INIT)
  assert want[5] == -1 and 3 not in want[6] and 2 in want[6]
  assert np.array_equal(emu.seed, seed, equal_nan=True)
  canvas.close()


@pytest.mark.parametrize('where', ['inside', 'outside', 'no_dirty_box', 'linear',
                                   'no_init'])
def test_clear_and_seed(engine, where):
  """init_seed at the chosen candidate in the pick's launch: the chosen voxel
  inside the dirty box, outside it, without a dirty box, the linear clear (dirty
  box of at least half the volume), and no init at all."""
  rng = np.random.RandomState(len(where))
  seed, seg = _volumes(rng, SHAPE, [1, 2, 3], density=0.0)
  box = ((4, 6, 8), (30, 31, 40))
  dirty = {'no_dirty_box': None, 'linear': 'all'}.get(where, box)
  canvas, emu = _pair(engine, SHAPE, seed, seg, dirty=dirty)
  if where == 'outside':
    cands = _cands(rng, SHAPE, 3, lo=(32, 0, 0))
  else:
    cands = _cands(rng, SHAPE, 3, lo=(6, 8, 10), hi=(28, 29, 38))
  init = None if where == 'no_init' else INIT
  want = _check_turn(canvas, emu, None, None, cands, (1, 1, 1), init, where)
  assert want[5] == 0
  if init is not None:
    assert np.isnan(emu.seed).sum() == emu.seed.size - 1
    assert emu.seed[tuple(cands[0])] == np.float32(INIT)
    canvas.init_seed((20, 20, 20), 1.0)  # the dirty box now is the seed point alone
    out = canvas.read_seed()
    assert np.isnan(out).sum() == out.size - 1 and out[20, 20, 20] == 1.0
  canvas.close()


def test_back_to_back_turns(engine):
  """Two turns on one canvas with nothing between them (the second histogram must
  not see the first), the single count between turns, then a turn with a larger
  max_existing_id than any before, so that the scratch grows; then a small one."""
  rng = np.random.RandomState(13)
  seed, seg = _volumes(rng, SHAPE, np.arange(1, 60))
  canvas, emu = _pair(engine, SHAPE, seed, seg)
  w1 = _check_turn(canvas, emu, ((0, 0, 0), (30, 40, 52), THR, 10 ** 9, 77, 59), None,
                   _cands(rng, SHAPE, 9), (1, 1, 1), None, 'first')
  w2 = _check_turn(canvas, emu, ((20, 5, 3), (48, 35, 50), THR, 10 ** 9, 78, 59), None,
                   _cands(rng, SHAPE, 70), (1, 1, 1), None, 'second')
  assert len(w1[2]) == 59 and len(w2[2]) == 59 and not np.array_equal(w1[3], w2[3])
  got = canvas.commit_count((20, 5, 3), (48, 35, 50), THR, 59)
  assert np.array_equal(got[3], w2[3])
  # ids up to 150000: the scratch allocated so far is too small
  big = 150000
  far = np.argwhere(seg > 0)
  pick = far[rng.choice(len(far), 500, replace=False)]
  newids = rng.randint(60, big + 1, 500).astype(np.int32)
  newids[:2] = (big, big - 1)
  canvas.write_seg_points(pick, newids)
  emu.write_seg_points(pick, newids)
  w3 = _check_turn(canvas, emu, ((0, 0, 0), SHAPE, THR, 10 ** 9, 79, big), None,
                   _cands(rng, SHAPE, 300), (0, 0, 0), None, 'grown')
  assert w3[2][-1] == big and len(w3[2]) > 59
  w4 = _check_turn(canvas, emu, ((0, 0, 0), SHAPE, THR, 0, 80, 59), None,
                   _cands(rng, SHAPE, 2), (0, 0, 0), INIT, 'small again')
  assert len(w4[2]) == 59 and w4[4]
  canvas.close()


def test_restricted_canvas(engine):
  """A canvas with a restrictor: candidates that are not segmented but vetoed get
  flag 4, are skipped and not marked (tests/restriction_ref.py's turn)."""
  rng = np.random.RandomState(17)
  seed, seg = _volumes(rng, SHAPE, [1, 2, 3], density=0.01)
  mask = rng.rand(*SHAPE) < 0.4
  seed_mask = rng.rand(*SHAPE) < 0.3
  canvas, emu = _pair(engine, SHAPE, seed, seg, dirty=((4, 6, 8), (30, 31, 40)),
                      ref_cls=_RestrictRef)
  canvas.set_restrictor(mask=mask, seed_mask=seed_mask)
  emu.bits = restriction_ref.restriction(SHAPE, mask, seed_mask)
  want = _check_turn(canvas, emu, ((3, 5, 7), (45, 33, 50), THR, 0, 77, 3),
                     ((1, 2, 3), 2), _cands(rng, SHAPE, 100), (1, 1, 1), INIT)
  assert emu.flag4 > 0 and 4 in want[6]
  canvas.close()
