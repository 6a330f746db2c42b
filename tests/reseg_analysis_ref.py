"""numpy / scipy restatement of resegmentation analysis: the definitions behind
include/ffn_analysis.h and ffn_amd/inference/resegmentation_analysis.py, for
inputs beyond the reference-minted fixture (tests/golden/ref_reseg_analysis.npz,
tools/make_golden_reseg_analysis.py), and the helpers that turn the fixture's
cases back into the .npz files `resegmentation.process_point` writes.

Nothing here shares code with the product: the masks are formed from the
dequantised probabilities, the distances come from scipy.
"""
import json
import os

import numpy as np
from scipy import ndimage

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
FIXTURE = os.path.join(GOLDEN, 'ref_reseg_analysis.npz')

PAIR_FLOATS = ('iou', 'max_edt_a', 'max_edt_b', 'from_a_max_edt',
               'from_b_max_edt', 'from_a_segment_a_consistency',
               'from_a_segment_b_consistency', 'from_b_segment_a_consistency',
               'from_b_segment_b_consistency')
PAIR_INTS = ('num_voxels_a', 'num_voxels_b', 'from_a_num_voxels',
             'from_b_num_voxels', 'from_a_deleted_voxels',
             'from_b_deleted_voxels', 'from_a_has_deleted_voxels',
             'from_b_has_deleted_voxels')
PAIR_VECTORS = ('point', 'segmentation_radius', 'radius', 'from_a_origin',
                'from_b_origin')  # xyz


# ---- definitions ----------------------------------------------------------------

def dequantize(q):
  """storage.dequantize_probability + nan_to_num, restated: byte 0 = never
  visited = probability 0, byte q = f32((q - 0.5) / 255)."""
  q = np.asarray(q)
  prob = ((q - 0.5) * (1.0 / 255)).astype(np.float32)
  prob[q == 0] = 0
  return prob


def object_mask(q, threshold):
  return dequantize(q) >= threshold


def max_edt(mask, voxel_size_zyx):
  """max of scipy's EDT; 0 for an empty mask, +inf for a mask without a 0 voxel
  (scipy's own answer there is arbitrary)."""
  mask = np.asarray(mask, bool)
  if not mask.any():
    return 0.0
  if mask.all():
    return float('inf')
  return float(ndimage.distance_transform_edt(
      mask, sampling=[float(v) for v in voxel_size_zyx]).max())


def pair_stats(probs, seg, offset_zyx, id_a, id_b, table, voxel_size_zyx):
  """(ten counts, four maxima) of one pair point, table-driven like the
  kernel's contract."""
  sel = tuple(slice(int(o), int(o) + s) for o, s in zip(offset_zyx, seg.shape))
  table = np.asarray(table).astype(bool)
  a = table[probs[0][sel]]
  b = table[probs[1][sel]]
  s1 = seg == np.uint64(id_a)
  s2 = seg == np.uint64(id_b)
  counts = [a.sum(), b.sum(), (a & b).sum(), (a | b).sum(), s1.sum(), s2.sum(),
            (a & s1).sum(), (a & s2).sum(), (b & s1).sum(), (b & s2).sum()]
  return (np.array(counts, np.uint64),
          np.array([max_edt(m, voxel_size_zyx) for m in (a, b, s1, s2)]))


def endpoint_overlaps(probs, seg, table, keep_id=None):
  """(|new|, {old: (num_overlapping, num_original)}) with every old id the new
  mask overlaps, and keep_id if it occurs in seg."""
  new = np.asarray(table).astype(bool)[probs]
  out = {}
  for old in np.unique(seg):
    sel = seg == old
    ov = int((sel & new).sum())
    if ov or (keep_id is not None and int(old) == int(keep_id)):
      out[int(old)] = (ov, int(sel.sum()))
  return int(new.sum()), out


class NumpyAnalyzer:
  """Stand-in for ffn_amd.analysis.Analyzer on the CPU (tests of the host
  plumbing): same calls, the restatement underneath."""

  def __init__(self):
    self.pair_batches, self.endpoint_batches = [], []

  def pair_stats(self, batch, table, voxel_size_zyx=(1, 1, 1)):
    self.pair_batches.append(len(batch))
    rows = [pair_stats(np.asarray(p.probs), np.asarray(p.seg, np.uint64),
                       p.offset_zyx, p.id_a, p.id_b, table, voxel_size_zyx)
            for p in batch]
    return (np.array([r[0] for r in rows], np.uint64).reshape(-1, 10),
            np.array([r[1] for r in rows], np.float64).reshape(-1, 4))

  def endpoint_overlaps(self, batch, table):
    self.endpoint_batches.append(len(batch))
    return [endpoint_overlaps(np.asarray(p.probs), np.asarray(p.seg, np.uint64),
                              table, p.id) for p in batch]


def f32(v):
  return np.float32(v)


def evaluate_pair(case, seg_volume=None):
  """The populated fields of evaluate_pair_resegmentation for a fixture case
  (dict as `load_cases` returns), or the name of the exception it raises."""
  probs = case['probs']
  if probs.shape[0] != 2:
    return 'IncompleteResegmentationError'
  seg_volume = case['seg'] if seg_volume is None else seg_volume
  z, y, x = (int(v) for v in case['point_zyx'])
  rad = np.array(case['radius_zyx'])
  ar = np.array(case['analysis_radius_zyx'])
  seg = seg_volume[z - ar[0]:z + ar[0] + 1, y - ar[1]:y + ar[1] + 1,
                   x - ar[2]:x + ar[2] + 1]
  s1, s2 = seg == case['id_a'], seg == case['id_b']
  out = {'num_voxels_a': int(s1.sum()), 'num_voxels_b': int(s2.sum())}
  if not out['num_voxels_a'] or not out['num_voxels_b']:
    return 'InvalidBaseSegmentatonError'
  delta = rad - ar
  sel = tuple(slice(d, d + 2 * r + 1) for d, r in zip(delta, ar))
  voxel = case['voxel_size_zyx']
  masks = [object_mask(probs[k][sel], case['threshold']) for k in range(2)]
  out['point'] = [x, y, z]
  out['segmentation_radius'] = list(rad[::-1])
  out['radius'] = list(ar[::-1])
  out['max_edt_a'] = max_edt(s1, voxel)
  out['max_edt_b'] = max_edt(s2, voxel)
  with np.errstate(invalid='ignore', divide='ignore'):
    out['iou'] = float(np.float64((masks[0] & masks[1]).sum()) /
                       np.float64((masks[0] | masks[1]).sum()))
  corner = np.array([x - rad[2], y - rad[1], z - rad[0]])
  for k, name in enumerate(('from_a', 'from_b')):
    m = masks[k]
    out[name + '_origin'] = list(np.array(case['start_points'][k][-1]) + corner)
    out[name + '_max_edt'] = max_edt(m, voxel)
    out[name + '_num_voxels'] = int(m.sum())
    out[name + '_segment_a_consistency'] = (m & s1).sum() / s1.sum()
    out[name + '_segment_b_consistency'] = (m & s2).sum() / s2.sum()
    moves = np.asarray(case['histories'][k])
    dels = np.asarray(case['deletes'][k])
    out[name + '_has_deleted_voxels'] = int(moves.size > 0)
    total = 0
    for mv, d in zip(moves.reshape(-1, 3), dels):
      if np.all(mv >= delta) and np.all(mv <= delta + 2 * ar):
        total += int(d)
    out[name + '_deleted_voxels'] = total
  return out


def evaluate_endpoint(case, seg_volume=None):
  seg_volume = case['seg'] if seg_volume is None else seg_volume
  z, y, x = (int(v) for v in case['point_zyx'])
  rad = np.array(case['radius_zyx'])
  seg = seg_volume[z - rad[0]:z + rad[0] + 1, y - rad[1]:y + rad[1] + 1,
                   x - rad[2]:x + rad[2] + 1]
  if not (seg == case['id_a']).any():
    return 'InvalidBaseSegmentatonError'
  new = object_mask(case['probs'][0], case['threshold'])
  overlaps = {}
  for old in np.unique(seg[new]):
    sel = seg == old
    overlaps[int(old)] = (int((sel & new).sum()), int(sel.sum()))
  return {'id': int(case['id_a']), 'start': [x, y, z],
          'segmentation_radius': list(rad[::-1]),
          'num_voxels': int(new.sum()), 'overlaps': overlaps,
          'source': overlaps.get(int(case['id_a']))}


# ---- fixture cases ----------------------------------------------------------------

def ragged(items):
  out = np.empty(len(items), dtype=object)
  for k, v in enumerate(items):
    out[k] = v
  return out


def file_name(case):
  z, y, x = (int(v) for v in case['point_zyx'])
  return '%d-%d_at_%d_%d_%d.npz' % (case['id_a'], case['id_b'], x, y, z)


def write_case_file(case, directory):
  """The .npz resegmentation.process_point leaves for the case (the arrays the
  analysis reads)."""
  path = os.path.join(str(directory), file_name(case))
  np.savez_compressed(
      path, probs=case['probs'],
      deletes=ragged([np.asarray(d) for d in case['deletes']]),
      histories=ragged([np.asarray(h).reshape(-1, 3)
                        for h in case['histories']]),
      start_points=ragged([[tuple(int(v) for v in p) for p in sp]
                           for sp in case['start_points']]))
  return path


def _reseg_cases():
  """Both points of ref_reseg.npz as cases (inputs only)."""
  g = np.load(os.path.join(GOLDEN, 'ref_reseg.npz'), allow_pickle=True)
  ids = [int(v) for v in g['ids']]
  common = dict(seg=g['init_seg'], point_zyx=[int(v) for v in g['point']],
                radius_zyx=[24, 24, 24], analysis_radius_zyx=[8, 8, 8],
                voxel_size_zyx=[1, 1, 1])
  pair = dict(common, kind='pair', id_a=ids[0], id_b=ids[1], threshold=0.6,
              probs=g['p0_probs'], deletes=list(g['p0_deletes']),
              histories=list(g['p0_histories']),
              start_points=[g['p0_start_points_a'], g['p0_start_points_b']])
  end = dict(common, kind='endpoint', id_a=ids[1], id_b=0, threshold=0.5,
             probs=g['p1_probs'], deletes=list(g['p1_deletes']),
             histories=list(g['p1_histories']),
             start_points=[g['p1_start_points_a'],
                           np.zeros((0, 3), np.int64)])
  return {'reseg_pair': pair, 'reseg_endpoint': end}


def load_cases():
  """name -> case dict: inputs as above plus 'want' (flat result fields or the
  name of the exception)."""
  f = np.load(FIXTURE, allow_pickle=False)
  cases = _reseg_cases()
  for name in [str(n) for n in f['names']]:
    pre = name + '/'
    meta = json.loads(str(f[pre + 'meta']))
    if name not in cases:
      case = {k: meta[k] for k in (
          'kind', 'point_zyx', 'radius_zyx', 'analysis_radius_zyx',
          'voxel_size_zyx', 'threshold', 'id_a', 'id_b')}
      case['seg'] = f[pre + 'seg']
      case['probs'] = f[pre + 'probs']
      case['deletes'] = [np.array(v, np.int64) for v in meta['deletes']]
      case['histories'] = [np.array(v, np.int64).reshape(-1, 3)
                           for v in meta['histories']]
      case['start_points'] = [np.array(v, np.int64).reshape(-1, 3)
                              for v in meta['start_points']]
      cases[name] = case
    cases[name]['want'] = meta['raises'] if 'raises' in meta else meta['want']
  return cases


def assert_pair_fields(got, want, name=''):
  """`got`: dict of flat fields (restatement) compared with a fixture `want`."""
  for key in PAIR_INTS:
    assert int(got[key]) == int(want[key]), (name, key, got[key], want[key])
  for key in PAIR_VECTORS:
    assert [int(v) for v in got[key]] == [int(v) for v in want[key]], (name, key)
  for key in PAIR_FLOATS:
    a, b = f32(got[key]), f32(want[key])
    assert a == b or (np.isnan(a) and np.isnan(b)), (name, key, got[key],
                                                     want[key])


def pair_result_fields(result):
  """Flat fields of a PairResegmentationResult message."""
  ev = result.eval
  out = {'point': [result.point.x, result.point.y, result.point.z],
         'segmentation_radius': [result.segmentation_radius.x,
                                 result.segmentation_radius.y,
                                 result.segmentation_radius.z],
         'radius': [ev.radius.x, ev.radius.y, ev.radius.z],
         'iou': ev.iou, 'max_edt_a': ev.max_edt_a, 'max_edt_b': ev.max_edt_b,
         'num_voxels_a': ev.num_voxels_a, 'num_voxels_b': ev.num_voxels_b}
  for name, sr in (('from_a', ev.from_a), ('from_b', ev.from_b)):
    out[name + '_origin'] = [sr.origin.x, sr.origin.y, sr.origin.z]
    out[name + '_num_voxels'] = sr.num_voxels
    out[name + '_has_deleted_voxels'] = int(sr.HasField('deleted_voxels'))
    out[name + '_deleted_voxels'] = sr.deleted_voxels
    out[name + '_segment_a_consistency'] = sr.segment_a_consistency
    out[name + '_segment_b_consistency'] = sr.segment_b_consistency
    out[name + '_max_edt'] = sr.max_edt
  return out


def assert_endpoint_fields(got, want, name=''):
  """`got`: dict as evaluate_endpoint returns; `want`: fixture fields."""
  assert int(got['id']) == int(want['id']), name
  assert [int(v) for v in got['start']] == [int(v) for v in want['start']], name
  assert ([int(v) for v in got['segmentation_radius']] ==
          [int(v) for v in want['segmentation_radius']]), name
  assert int(got['num_voxels']) == int(want['num_voxels']), name
  rows = {int(r[0]): (int(r[1]), int(r[2])) for r in want['overlaps']}
  assert got['overlaps'] == rows, (name, got['overlaps'], rows)
  src = want['source']
  if int(src[0]):
    assert got['source'] == (int(src[1]), int(src[2])), name
  else:
    assert got['source'] is None, name


def endpoint_result_fields(result):
  """The same dict from an EndpointResegmentationResult message."""
  return {
      'id': result.id,
      'start': [result.start.x, result.start.y, result.start.z],
      'segmentation_radius': [result.segmentation_radius.x,
                              result.segmentation_radius.y,
                              result.segmentation_radius.z],
      'num_voxels': result.num_voxels,
      'overlaps': {int(k): (v.num_overlapping, v.num_original)
                   for k, v in result.overlaps.items()},
      'source': ((result.source.num_overlapping, result.source.num_original)
                 if result.HasField('source') else None)}


class Volume4d:
  """[c, z, y, x] view of a 3d array whose slices keep the leading axis, like
  the volume objects the reference indexes (`vol[0, z, y, x][0, ...]`)."""

  def __init__(self, seg):
    self.seg = seg
    self.shape = (1,) + tuple(seg.shape)

  def __getitem__(self, index):
    assert index[0] == 0
    return self.seg[index[1:]][np.newaxis]


def random_pair_point(rng, box, crop, offset, n_ids=6, fill=0.45):
  """A random pair point of the given box / crop shapes (inputs of
  `pair_stats`): smooth random probabilities with unvisited (0) voxels, a
  blocky base segmentation holding ids a, b and others."""
  field = ndimage.gaussian_filter(rng.random((2,) + tuple(box)), (0, 1.5, 2, 2))
  field = (field - field.mean()) / (field.std() + 1e-9)
  prob = 1.0 / (1.0 + np.exp(-(field * 2.5 + (fill - 0.5) * 4)))
  q = np.digitize(prob, np.linspace(0.0, 1.0, 255)).astype(np.uint8)
  q[rng.random(q.shape) < 0.1] = 0
  labels = ndimage.gaussian_filter(rng.random(tuple(crop)), 2.0)
  ranks = np.digitize(labels, np.quantile(labels, np.linspace(0, 1, n_ids + 1)[1:-1]))
  ids = np.array([0, 7, 2**40 + 5, 3, 2**63 + 11, 9, 12, 15][:n_ids], np.uint64)
  seg = ids[ranks]
  return q, seg, tuple(offset), int(ids[1]), int(ids[2])
