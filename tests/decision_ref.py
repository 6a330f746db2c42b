"""numpy restatement of the decision point specification (include/ffn_decision.h,
DESIGN.md "Decision points"): the yardstick of tests/test_decision_points.py
and tests/test_gpu_decision_points.py.  numpy only; slow and obvious on purpose.

  expand_spec            nearest-segment expansion, ties to the smallest id
  brute_force_expand     the same by definition (all labelled voxels), small
                         volumes only
  candidates_spec        the contact candidates in the reference's row order
  minimising_spec        those at the minimum distance of their pair
  decision_points_spec   the whole function
  synthetic_segmentation seeded blocky label volumes with unlabelled gaps
"""

import numpy as np

OFFSETS = ((0, 0, -1), (0, -1, 0), (0, -1, -1), (-1, 0, 0), (-1, 0, -1),
           (-1, -1, 0), (-1, -1, -1))

_PACK_INF = np.int64(1) << np.int64(62)
_PACK_LIMIT = 1 << 29  # largest d2 the packed path may meet


def _pass_packed(state, axis, w):
  """state: int64 d2 << 32 | id (or _PACK_INF); exhaustive minimum along axis."""
  f = np.moveaxis(state, axis, 0)
  length = f.shape[0]
  flat = f.reshape(length, -1)
  best = np.full_like(flat, _PACK_INF)
  q = np.arange(length, dtype=np.int64)
  for p in range(length):
    t = (q - p) * np.int64(w)
    cand = flat[p][None, :] + ((t * t) << np.int64(32))[:, None]
    np.minimum(best, cand, out=best)
  np.minimum(best, _PACK_INF, out=best)
  return np.moveaxis(best.reshape(f.shape), 0, axis)


def _pass_float(d2, ids, axis, w):
  """Exhaustive lexicographic minimum of (d2 + ((q - p) * w)**2, id) along axis."""
  f = np.moveaxis(d2, axis, 0)
  g = np.moveaxis(ids, axis, 0)
  length = f.shape[0]
  ff = f.reshape(length, -1)
  gg = g.reshape(length, -1)
  best = np.full_like(ff, np.inf)
  best_id = np.zeros_like(gg)
  q = np.arange(length, dtype=np.float64)
  for p in range(length):
    t = (q - p) * w
    cand = ff[p][None, :] + (t * t)[:, None]
    cid = np.broadcast_to(gg[p][None, :], cand.shape)
    take = (cand < best) | ((cand == best) & (cid < best_id))
    best = np.where(take, cand, best)
    best_id = np.where(take, cid, best_id)
  best_id[np.isinf(best)] = 0
  return (np.moveaxis(best.reshape(f.shape), 0, axis),
          np.moveaxis(best_id.reshape(g.shape), 0, axis))


def expand_spec(seg, voxel_size, max_distance=None):
  """(expanded, edt): see the module docstring.  voxel_size is xyz, seg is zyx;
  the passes run x, then y, then z, so that d2 = ((x + y) + z)."""
  seg = np.asarray(seg)
  if seg.ndim != 3:
    raise ValueError('expand_spec expects a 3d array')
  values, inverse = np.unique(seg, return_inverse=True)
  if values[0] != 0:
    values = np.concatenate([np.zeros(1, values.dtype), values])
    inverse = inverse + 1
  ranks = inverse.reshape(seg.shape).astype(np.int64)  # order-preserving ids
  sampling = [float(v) for v in voxel_size][::-1]  # z, y, x
  integral = all(s == int(s) for s in sampling)
  bound = sum(((n - 1) * s) ** 2 for n, s in zip(seg.shape, sampling))
  if integral and bound < _PACK_LIMIT and len(values) < (1 << 31):
    state = np.where(ranks > 0, ranks, _PACK_INF)
    for axis in (2, 1, 0):
      state = _pass_packed(state, axis, int(sampling[axis]))
    inf = state >= _PACK_INF
    d2 = (state >> np.int64(32)).astype(np.float64)
    d2[inf] = np.inf
    ids = state & np.int64(0xffffffff)
    ids[inf] = 0
  else:
    d2 = np.where(ranks > 0, 0.0, np.inf)
    ids = ranks
    for axis in (2, 1, 0):
      d2, ids = _pass_float(d2, ids, axis, sampling[axis])
  edt = np.sqrt(d2)
  expanded = values[ids].astype(seg.dtype)
  if max_distance is not None:
    expanded[edt > max_distance] = 0
  return expanded, edt


def brute_force_expand(seg, voxel_size):
  """By definition: (edt, d2, tied) with tied[v] = sorted ids of ALL labelled
  voxels at the minimum d2 of v.  O(voxels * labelled voxels)."""
  seg = np.asarray(seg)
  sx, sy, sz = [float(v) for v in voxel_size]
  lab = np.argwhere(seg > 0)
  lab_ids = seg[seg > 0]
  d2 = np.full(seg.shape, np.inf)
  tied = np.empty(seg.shape, object)
  for v in np.ndindex(*seg.shape):
    if not len(lab):
      tied[v] = []
      continue
    tx = (lab[:, 2] - v[2]) * sx
    ty = (lab[:, 1] - v[1]) * sy
    tz = (lab[:, 0] - v[0]) * sz
    dd = (tx * tx + ty * ty) + tz * tz
    m = dd.min()
    d2[v] = m
    tied[v] = sorted(set(int(i) for i in lab_ids[dd == m]))
  return np.sqrt(d2), d2, tied


def candidates_spec(expanded, edt):
  """All contact candidates as a dict of arrays (a, b, dist, off, z, y, x) in
  the row order of the reference (offset number, then z, y, x)."""
  cols = {k: [] for k in ('a', 'b', 'dist', 'off', 'z', 'y', 'x')}
  for number, off in enumerate(OFFSETS):
    here = tuple(slice(0, -1) if o else slice(None) for o in off)
    there = tuple(slice(1, None) if o else slice(None) for o in off)
    a, b = expanded[here], expanded[there]
    touching = (a > 0) & (b > 0) & (a != b)
    z, y, x = np.nonzero(touching)
    av = a[touching].astype(np.uint64)
    bv = b[touching].astype(np.uint64)
    cols['a'].append(np.minimum(av, bv))
    cols['b'].append(np.maximum(av, bv))
    cols['dist'].append((edt[here][touching] + edt[there][touching]) / 2)
    cols['off'].append(np.full(len(z), number, np.int32))
    cols['z'].append(z.astype(np.int32))
    cols['y'].append(y.astype(np.int32))
    cols['x'].append(x.astype(np.int32))
  return {k: np.concatenate(v) for k, v in cols.items()}


def _groups(c):
  """(order, starts): rows sorted by pair, keeping row order inside a pair."""
  order = np.lexsort((np.arange(len(c['a'])), c['b'], c['a']))
  a, b = c['a'][order], c['b'][order]
  new = np.ones(len(order), bool)
  new[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
  return order, np.nonzero(new)[0]


def minimising_spec(c):
  """The candidates whose distance is the minimum of their pair (row order kept)."""
  if not len(c['a']):
    return c
  order, starts = _groups(c)
  dist = c['dist'][order]
  mins = np.minimum.reduceat(dist, starts)
  counts = np.diff(np.append(starts, len(order)))
  keep = np.zeros(len(order), bool)
  keep[order] = dist == np.repeat(mins, counts)
  return {k: v[keep] for k, v in c.items()}


def select_spec(c):
  """{(a, b): (dist, xyz)}: per pair the first minimising candidate (row order)
  closest to the mean coordinate of that pair's minimising candidates."""
  ret = {}
  if not len(c['a']):
    return ret
  order, starts = _groups(c)
  ends = np.append(starts[1:], len(order))
  for s, e in zip(starts, ends):
    rows = order[s:e]
    points = np.stack([c['x'][rows], c['y'][rows], c['z'][rows]],
                      axis=1).astype(np.int64)
    offset = points - points.mean(axis=0)
    spread = (offset * offset).sum(axis=1)
    ret[(int(c['a'][rows[0]]), int(c['b'][rows[0]]))] = (
        c['dist'][rows[0]], points[int(spread.argmin())])
  return ret


def decision_points_spec(seg, voxel_size, max_distance=None, slice3d=None):
  expanded, edt = expand_spec(seg, voxel_size, max_distance)
  if slice3d is not None:
    expanded, edt = expanded[slice3d], edt[slice3d]
  return select_spec(minimising_spec(candidates_spec(expanded, edt)))


def synthetic_segmentation(shape, seed, gap=2, drop=0.15, dtype=np.uint64,
                           id_base=1, id_step=7, block=(5, 14)):
  """Blocky label volume: boxes between random cuts, each with an id of its own
  (id_base + k * id_step, shuffled) and an edge of block[0] <= n < block[1]
  voxels, separated by `gap` unlabelled voxels; a fraction `drop` of the boxes
  is left out entirely."""
  rng = np.random.RandomState(seed)
  axes = []
  for n in shape:
    cuts, pos = [0], 0
    while True:
      pos += int(rng.randint(*block))
      if pos >= n:
        break
      cuts.append(pos)
    axes.append(np.searchsorted(np.array(cuts), np.arange(n), side='right') - 1)
  nb = [int(a.max()) + 1 for a in axes]
  ids = (np.asarray(id_base, dtype) +
         rng.permutation(nb[0] * nb[1] * nb[2]).astype(dtype) *
         np.asarray(id_step, dtype)).reshape(nb)
  ids[rng.rand(*nb) < drop] = 0
  seg = ids[np.ix_(*axes)].copy()
  for axis, a in enumerate(axes):
    if len(a) <= gap:  # (an axis this short is one box without a gap)
      continue
    first = np.ones(len(a), bool)
    first[gap:] = a[gap:] != a[:-gap]
    sel = [slice(None)] * 3
    sel[axis] = first
    seg[tuple(sel)] = 0
  return seg


def touching_parabola_volume(axis):
  """The 1 x 5 x 9 arrangement of the specification (ids 7, 9, 3, 5 at distance
  2 from the centre, id 3 reachable only through a parabola that merely touches
  the lower envelope), laid out so that the last separable pass runs along
  `axis` (1 = y, 0 = z).  Returns (seg, centre index)."""
  seg = np.zeros((1, 5, 9), np.uint64)
  seg[0, 0, 4] = 7
  seg[0, 4, 4] = 9
  seg[0, 2, 2] = 3
  seg[0, 2, 6] = 5
  if axis == 1:
    return seg, (0, 2, 4)
  return np.ascontiguousarray(seg.transpose(1, 0, 2)), (2, 0, 4)
