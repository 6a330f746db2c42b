#!/usr/bin/env python3
"""Mints tests/golden/ref_reseg_analysis.npz with the reference's own
resegmentation_analysis (ffn/inference/resegmentation_analysis.py).

Runs in the build container only.  The reference module is imported UNMODIFIED;
what keeps it from running at HEAD is worked around HERE (documented in
DESIGN.md, and the product makes the same fixes):
  * it imports `google3.pyglib.{gfile, logging}` and
    `google3.research.neuromancer.segmentation.ffn.{resegmentation_pb2,
    storage}`: `sys.modules` entries map these names to `open`, the standard
    logging module and the reference's own ffn/inference/resegmentation_pb2.py
    (which imports `utils.vector_pb2`: the reference's ffn/ is put on the path)
    and storage.py;
  * it builds `resegmentation_pb2.EndpointSegmentationResult`, a message the
    proto does not define: aliased to `EndpointResegmentationResult`;
  * the shipped resegmentation_pb2.py is pre-3.20 generated code in which
    current protobuf does not see `overlaps` as a map: the message classes are
    rebuilt from that module's own serialized descriptor (same schema);
  * it uses `np.int` (removed in numpy 1.24): set to `int`;
  * it reads the ragged `deletes` / `histories` / `start_points` object arrays
    with a bare `np.load(f)`, which numpy >= 1.16.3 refuses: the module's `np`
    is wrapped so that `load` passes allow_pickle=True;
  * it indexes a VolumeStore (`vol[0, z, y, x][0, ...]`): the volumes here are
    numpy arrays behind a wrapper whose slices keep the channel axis;
  * it calls the closed `pywrapsegment_util.ComputeOverlapCounts`.  THE
    ORIGINAL IS NOT AVAILABLE: the stand-in below returns
    `{(old, new): count}` over the two flattened label arrays, which is what the
    caller's loop (`for k, v in overlaps.items(): old, new = k`) consumes.  The
    endpoint overlaps of the fixture therefore rest on this restatement, not on
    the original routine.
Everything else -- thresholds, crops, distance transforms, the deleted-voxel
window, origins, the divisions, the proto fields -- is the reference's code.

Cases: both points of tests/golden/ref_reseg.npz as the files process_point
wrote, synthetic pair and endpoint files (blob objects, quantised
probabilities with never-visited zeros, radii differing per axis, analysis
radius below and at the radius, voxel sizes (1, 1, 1) and (33, 8, 8),
thresholds 0.5 / 0.6 / 0.9, multi-attempt start points, empty and non-empty
histories), and cases that raise.  The file holds, per case, the inputs of a
synthetic case (`probs`, `seg`, the rest in the json `meta`) and every
populated result field, flat, under meta['want'] -- or meta['raises'].
"""
import json
import os
import sys
import tempfile
import types

os.environ['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('FFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
# resegmentation_pb2 imports its dependency as `utils.vector_pb2`
sys.path.insert(0, os.path.join(REF, 'ffn'))
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, ROOT)

import logging  # noqa: E402

import numpy as np  # noqa: E402
from scipy import ndimage  # noqa: E402

from ffn.inference import resegmentation_pb2  # noqa: E402
from ffn.inference import storage as ref_storage  # noqa: E402

from tests import reseg_analysis_ref as ra  # noqa: E402


def compute_overlap_counts(old, new):
  """Stand-in for pywrapsegment_util.ComputeOverlapCounts (see above)."""
  old = np.asarray(old, np.uint64)
  new = np.asarray(new, np.uint64)
  out = {}
  for o in np.unique(old):
    sel = old == o
    for n in np.unique(new[sel]):
      out[(int(o), int(n))] = int(np.sum(new[sel] == n))
  return out


class _LegacyNumpy:
  """numpy whose `load` still reads object arrays, and with `np.int`."""
  int = int

  def __getattr__(self, name):
    return getattr(np, name)

  @staticmethod
  def load(f, *args, **kwargs):
    kwargs.setdefault('allow_pickle', True)
    return np.load(f, *args, **kwargs)


def message_classes():
  """The reference's result messages, from the serialized descriptors its
  generated modules carry."""
  from google.protobuf import descriptor_pb2
  from google.protobuf import descriptor_pool
  from google.protobuf import message_factory
  from utils import vector_pb2
  pool = descriptor_pool.DescriptorPool()
  for mod in (vector_pb2, resegmentation_pb2):
    pool.Add(descriptor_pb2.FileDescriptorProto.FromString(
        mod.DESCRIPTOR.serialized_pb))
  get = lambda name: message_factory.GetMessageClass(
      pool.FindMessageTypeByName('ffn.' + name))
  pair, end = get('PairResegmentationResult'), get('EndpointResegmentationResult')
  return types.SimpleNamespace(PairResegmentationResult=pair,
                               EndpointResegmentationResult=end,
                               EndpointSegmentationResult=end)


def import_reference():
  pb2 = message_classes()

  def module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m

  module('google3')
  module('google3.pyglib', gfile=module('google3.pyglib.gfile', Open=open),
         logging=logging)
  sys.modules['google3.pyglib.logging'] = logging
  for name in ('google3.research', 'google3.research.neuromancer',
               'google3.research.neuromancer.segmentation'):
    module(name)
  module('google3.research.neuromancer.segmentation.ffn',
         resegmentation_pb2=pb2, storage=ref_storage)
  sys.modules['google3.research.neuromancer.segmentation.ffn.'
              'resegmentation_pb2'] = pb2
  sys.modules['google3.research.neuromancer.segmentation.ffn.storage'] = (
      ref_storage)
  module('google3.research.neuromancer.segmentation.python',
         pywrapsegment_util=module(
             'google3.research.neuromancer.segmentation.python.'
             'pywrapsegment_util', ComputeOverlapCounts=compute_overlap_counts))
  from ffn.inference import resegmentation_analysis  # noqa: E402
  resegmentation_analysis.np = _LegacyNumpy()
  return resegmentation_analysis


def blobs(rng, shape, n, radius):
  """Union of n random balls: a blob mask."""
  zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
  mask = np.zeros(shape, bool)
  centre = np.array(shape) / 2.0
  for _ in range(n):
    c = centre + rng.normal(0, radius * 0.8, 3)
    r = rng.uniform(0.6, 1.2) * radius
    mask |= (zz - c[0])**2 + (yy - c[1])**2 + (xx - c[2])**2 <= r * r
  return mask


def synthetic_case(rng, kind, radius, analysis_radius, voxel, threshold,
                   attempts=(1, 1), history=(5, 7), drop_b=False,
                   one_object=False, drop_a=False):
  radius = np.array(radius)
  box = 2 * radius + 1
  margin_lo, margin_hi = rng.integers(1, 4, 3), rng.integers(1, 4, 3)
  vol_shape = box + margin_lo + margin_hi
  point = margin_lo + radius
  id_a, id_b = 2**33 + 17, 42
  # base segmentation: two blob segments meeting near the point, a third one,
  # background 0
  seg = np.zeros(vol_shape, np.uint64)
  grid = np.indices(vol_shape)
  half = grid[2] + 0.3 * grid[1] < point[2] + 0.3 * point[1]
  body = blobs(rng, vol_shape, 6, radius.min() * 0.7)
  seg[blobs(rng, vol_shape, 3, radius.min() * 0.5)] = 99
  seg[body & half] = id_a
  seg[body & ~half] = 0 if drop_b else id_b
  if drop_a:
    seg[seg == id_a] = 0
  seg[ndimage.binary_dilation(half) & ~half & (rng.random(vol_shape) < 0.7)] = 0
  # object maps: smoothed blob masks + noise, never-visited voxels as NaN
  n_obj = 1 if (kind == 'endpoint' or one_object) else 2
  probs = []
  inner = tuple(slice(int(l), int(l + b)) for l, b in zip(margin_lo, box))
  shared = blobs(rng, tuple(box), 2, radius.min() * 0.35)
  for k in range(n_obj):
    target = (seg == (id_a if k == 0 else id_b))[inner].astype(float)
    if kind == 'endpoint':
      target = np.maximum(target, blobs(rng, tuple(box), 2, radius.min() * 0.5))
    else:  # a region both objects claim
      target = np.maximum(target, shared)
    p = ndimage.gaussian_filter(target, 1.2) * 1.3 + rng.normal(0, 0.05, box)
    p = np.clip(p, 0.001, 0.999)
    visited = blobs(rng, tuple(box), 8, radius.min() * 0.9)
    p[~visited] = np.nan
    probs.append(ref_storage.quantize_probability(p))
  probs = np.array(probs)
  assert (probs == 0).any()
  delta = radius - np.array(analysis_radius)
  histories, deletes, starts = [], [], [[], []]
  for k in range(n_obj):
    n_hist = history[k] if kind == 'pair' else history[0]
    h = rng.integers(0, box, (n_hist, 3))
    if n_hist >= 3:  # on the corners of the analysis box: both ends inclusive
      h[0] = delta
      h[1] = delta + 2 * np.array(analysis_radius)
      h[2] = np.maximum(delta - 1, 0)
    histories.append(h.astype(np.int64).reshape(-1, 3))
    deletes.append(rng.integers(0, 3000, n_hist).astype(np.int64))
    for _ in range(attempts[k]):
      zyx = rng.integers(0, box, 3)
      starts[k].append((int(zyx[2]), int(zyx[1]), int(zyx[0])))
  return {
      'kind': kind, 'seg': seg, 'probs': probs,
      'point_zyx': [int(v) for v in point],
      'radius_zyx': [int(v) for v in radius],
      'analysis_radius_zyx': [int(v) for v in analysis_radius],
      'voxel_size_zyx': [float(v) for v in voxel], 'threshold': threshold,
      'id_a': id_a, 'id_b': id_b if kind == 'pair' else 0,
      'deletes': deletes, 'histories': histories,
      'start_points': [np.array(s, np.int64).reshape(-1, 3) for s in starts]}


def check_masks_have_a_zero(case):
  """Every mask the reference takes a distance transform of must have a 0 voxel
  in its box (scipy's answer is arbitrary otherwise)."""
  if case['kind'] != 'pair' or case['probs'].shape[0] != 2:
    return
  z, y, x = case['point_zyx']
  ar = np.array(case['analysis_radius_zyx'])
  rad = np.array(case['radius_zyx'])
  seg = case['seg'][z - ar[0]:z + ar[0] + 1, y - ar[1]:y + ar[1] + 1,
                    x - ar[2]:x + ar[2] + 1]
  sel = tuple(slice(d, d + 2 * r + 1) for d, r in zip(rad - ar, ar))
  prob = np.nan_to_num(ref_storage.dequantize_probability(case['probs']))
  for mask in (seg == case['id_a'], seg == case['id_b'],
               prob[0][sel] >= case['threshold'],
               prob[1][sel] >= case['threshold']):
    assert not mask.all(), 'a mask without a 0 voxel'


def pair_fields(result):
  """Every populated field of a PairResegmentationResult proto, flat."""
  ev = result.eval
  out = {'point': [result.point.x, result.point.y, result.point.z],
         'id_a': np.uint64(result.id_a), 'id_b': np.uint64(result.id_b),
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


def endpoint_fields(result):
  rows = sorted((int(k), v.num_overlapping, v.num_original)
                for k, v in result.overlaps.items())
  src = result.source
  return {'id': np.uint64(result.id),
          'start': [result.start.x, result.start.y, result.start.z],
          'segmentation_radius': [result.segmentation_radius.x,
                                  result.segmentation_radius.y,
                                  result.segmentation_radius.z],
          'num_voxels': result.num_voxels,
          'overlaps': np.array(rows, np.uint64).reshape(-1, 3),
          'source': np.array([int(result.HasField('source')),
                              src.num_overlapping, src.num_original], np.int64)}


def main():
  ref = import_reference()
  rng = np.random.default_rng(20240917)
  cases = ra._reseg_cases()  # pylint:disable=protected-access
  synthetic = {}
  pair_specs = [
      # radius zyx, analysis radius, voxel zyx, threshold, attempts, history
      ((9, 11, 13), (6, 8, 9), (1, 1, 1), 0.5, (1, 1), (5, 7)),
      ((9, 11, 13), (9, 11, 13), (1, 1, 1), 0.6, (2, 1), (4, 0)),
      ((8, 13, 11), (5, 13, 7), (33, 8, 8), 0.5, (1, 3), (0, 0)),
      ((8, 13, 11), (8, 13, 11), (33, 8, 8), 0.9, (1, 1), (6, 6)),
      ((12, 9, 10), (7, 4, 10), (33, 8, 8), 0.6, (2, 2), (3, 9)),
      ((12, 9, 10), (3, 3, 3), (1, 1, 1), 0.9, (1, 1), (8, 2)),
      ((7, 16, 9), (7, 10, 5), (1, 1, 1), 0.6, (1, 2), (12, 1)),
      ((8, 8, 15), (4, 8, 12), (33, 8, 8), 0.5, (3, 1), (5, 5)),
      ((10, 10, 10), (10, 10, 10), (33, 8, 8), 0.6, (1, 1), (1, 4)),
      ((6, 13, 11), (2, 11, 6), (1, 1, 1), 0.5, (1, 1), (7, 3)),
  ]
  for k, (rad, ar, voxel, thr, attempts, hist) in enumerate(pair_specs):
    synthetic['pair%02d' % k] = synthetic_case(rng, 'pair', rad, ar, voxel, thr,
                                               attempts, hist)
  end_specs = [((9, 11, 13), 0.5), ((8, 13, 11), 0.6), ((12, 9, 10), 0.9),
               ((7, 15, 9), 0.5)]
  for k, (rad, thr) in enumerate(end_specs):
    synthetic['endpoint%02d' % k] = synthetic_case(rng, 'endpoint', rad, rad,
                                                   (1, 1, 1), thr)
  synthetic['raises_incomplete'] = synthetic_case(
      rng, 'pair', (9, 10, 11), (5, 5, 5), (1, 1, 1), 0.5, one_object=True)
  synthetic['raises_invalid_base'] = synthetic_case(
      rng, 'pair', (9, 10, 11), (5, 5, 5), (1, 1, 1), 0.5, drop_b=True)
  synthetic['raises_invalid_base_endpoint'] = synthetic_case(
      rng, 'endpoint', (9, 10, 11), (9, 10, 11), (1, 1, 1), 0.5, drop_a=True)
  cases.update(synthetic)

  out = {'names': np.array(list(cases))}
  with tempfile.TemporaryDirectory() as tmp:
    for name, case in cases.items():
      pre = name + '/'
      check_masks_have_a_zero(case)
      path = ra.write_case_file(case, tmp)
      volume = ra.Volume4d(case['seg'])
      meta = {}
      if name in synthetic:
        out[pre + 'probs'] = case['probs']
        out[pre + 'seg'] = case['seg']
        for key in ('kind', 'point_zyx', 'radius_zyx', 'analysis_radius_zyx',
                    'voxel_size_zyx', 'threshold', 'id_a', 'id_b'):
          meta[key] = case[key]
        for key in ('deletes', 'histories', 'start_points'):
          meta[key] = [np.asarray(v).tolist() for v in case[key]]
      try:
        if case['kind'] == 'pair':
          fields = pair_fields(ref.evaluate_pair_resegmentation(
              path, volume, case['radius_zyx'], case['analysis_radius_zyx'],
              case['voxel_size_zyx'], case['threshold']))
        else:
          fields = endpoint_fields(ref.evaluate_endpoint_resegmentation(
              path, volume, case['radius_zyx'], case['threshold']))
      except (ref.IncompleteResegmentationError,
              ref.InvalidBaseSegmentatonError) as e:
        assert name.startswith('raises'), name
        meta['raises'] = type(e).__name__
        print(name, 'raises', type(e).__name__)
      else:
        assert not name.startswith('raises'), name
        meta['want'] = {k: np.asarray(v).tolist() for k, v in fields.items()}
        print(name, {k: v for k, v in fields.items() if np.size(v) <= 3})
      # floats survive json exactly (repr round trip; NaN / Infinity literals)
      out[pre + 'meta'] = json.dumps(meta)
  dst = ra.FIXTURE
  np.savez_compressed(dst, **out)
  print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
  main()
