#!/usr/bin/env python3
"""Mints tests/golden/ref_decision_points.npz with the reference's own
ffn.utils.decision_point.find_decision_points.

Runs in the build container only (needs the reference checkout, pandas and,
for the tie statistics, scipy).  The reference modules are imported through
tools/ref_shims; `connectomics.segmentation.labels.watershed_expand` is the
shim that calls the specification (tests/decision_ref.expand_spec: nearest
labelled voxel, ties to the smallest id).  Everything after the expansion is
the reference's unmodified code.

Per case the file holds the input volume, the parameters, the reference's
result (sorted pairs, distances, points) and the specification's list of
minimising candidates (what the device's contact scan returns).  `<case>_scipy`
records, for documentation only, how the same run comes out when the expansion
takes scipy's own choice among equally near voxels: [pairs with the tie rule,
pairs with scipy, pairs in common, identical entries among those].
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('FFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from connectomics.common import bounding_box  # noqa: E402
from connectomics.segmentation import labels as shim_labels  # noqa: E402
from ffn.utils import decision_point as ref_dp  # noqa: E402

import decision_ref  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')

# name -> (shape, seed, dtype, id_base, id_step, voxel_size xyz, max_distance,
#          subvol (start xyz, size xyz), optimize_sparse, noise threshold)
CASES = {
    'iso': ((40, 48, 56), 1, np.uint64, 1, 7, (1, 1, 1), None, None, False, 0),
    'iso_max': ((40, 48, 56), 2, np.uint64, 1, 7, (1, 1, 1), 40.0, None,
                False, 0),
    'aniso': ((36, 50, 44), 3, np.uint64, 5, 3, (8, 8, 33), None, None,
              False, 0),
    'aniso_max': ((36, 50, 44), 4, np.uint64, 5, 3, (8, 8, 33), 40.0, None,
                  False, 0),
    'subvol': ((40, 48, 56), 5, np.uint64, 1, 7, (8, 8, 33), None,
               ((5, 7, 3), (37, 29, 31)), False, 0),
    'big_ids': ((30, 34, 38), 6, np.uint64, 2**32 + 11, 2**20 + 1, (8, 8, 33),
                None, None, False, 0),
    'sparse_one': ((20, 22, 24), 7, np.uint64, 1, 7, (1, 1, 1), None, None,
                   True, 0),
    'sparse_dust': ((30, 34, 38), 8, np.uint64, 1, 7, (8, 8, 33), None, None,
                    True, 400),
}


def case_volume(name):
  shape, seed, dtype, base, step = CASES[name][:5]
  seg = decision_ref.synthetic_segmentation(shape, seed, dtype=dtype,
                                            id_base=base, id_step=step)
  if name == 'sparse_one':  # one segment and a few voxels of noise of that id
    seg[seg != seg.max()] = 0
  return seg


def scipy_expand(seg, voxel_size, max_distance=None):
  from scipy import ndimage
  edt, idx = ndimage.distance_transform_edt(
      seg == 0, sampling=tuple(voxel_size)[::-1], return_indices=True)
  expanded = seg[tuple(idx)]
  if max_distance is not None:
    expanded[edt > max_distance] = 0
  return expanded, edt


def run_reference(seg, params):
  voxel, maxd, subvol, sparse, noise = params
  box = None
  if subvol is not None:
    box = bounding_box.BoundingBox(start=subvol[0], size=subvol[1])
  return ref_dp.find_decision_points(
      seg.copy(), voxel, max_distance=maxd, subvol_box=box,
      optimize_sparse=sparse, sparse_noise_threshold=noise)


def main():
  out = {'cases': np.array(sorted(CASES))}
  for name in sorted(CASES):
    params = CASES[name][5:]
    voxel, maxd, subvol, sparse, noise = params
    seg = case_volume(name)
    shim_labels.WATERSHED_EXPAND = None
    ref = run_reference(seg, params)
    keys = sorted(ref)
    out[name + '_seg'] = seg
    out[name + '_voxel_size'] = np.array(voxel, np.float64)
    out[name + '_max_distance'] = np.array(np.nan if maxd is None else maxd)
    out[name + '_subvol'] = (np.array(subvol, np.int64) if subvol is not None
                             else np.zeros((0, 3), np.int64))
    out[name + '_sparse'] = np.array([int(sparse), noise], np.int64)
    out[name + '_pairs'] = np.array(keys, np.uint64).reshape(-1, 2)
    out[name + '_dist'] = np.array([ref[k][0] for k in keys], np.float64)
    out[name + '_points'] = np.array([ref[k][1] for k in keys],
                                     np.int64).reshape(-1, 3)
    # what the contact scan of the device returns for this case
    work = seg.copy()
    if sparse and noise:
      ids, counts = np.unique(work, return_counts=True)
      work[np.isin(work, ids[counts < noise])] = 0
    expanded, edt = decision_ref.expand_spec(work, voxel, maxd)
    if subvol is not None:
      sl = bounding_box.BoundingBox(start=subvol[0], size=subvol[1]).to_slice3d()
      expanded, edt = expanded[sl], edt[sl]
    cands = decision_ref.minimising_spec(
        decision_ref.candidates_spec(expanded, edt))
    if sparse and not ref:
      cands = {k: v[:0] for k, v in cands.items()}
    for k, v in cands.items():
      out['%s_cand_%s' % (name, k)] = v
    stats = np.zeros(4, np.int64)
    try:
      shim_labels.WATERSHED_EXPAND = scipy_expand
      alt = run_reference(seg, params)
      common = [k for k in keys if k in alt]
      same = [k for k in common if alt[k][0] == ref[k][0] and
              np.array_equal(alt[k][1], ref[k][1])]
      stats[:] = len(keys), len(alt), len(common), len(same)
    except ImportError:
      pass
    finally:
      shim_labels.WATERSHED_EXPAND = None
    out[name + '_scipy'] = stats
    print('%-12s shape %s  labelled %.0f%%  pairs %d  candidates %d  scipy %s'
          % (name, seg.shape, 100.0 * np.mean(seg > 0), len(keys),
             len(cands['a']), stats.tolist()))
  dst = os.path.join(GOLD, 'ref_decision_points.npz')
  np.savez_compressed(dst, **out)
  print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
  main()
