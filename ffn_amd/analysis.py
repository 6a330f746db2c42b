"""Python handle over the resegmentation analysis kernels of libffn_hip.so
(include/ffn_analysis.h): mask counts and maximum distance transforms of pair
points, overlap tables of endpoint points -- a batch of points per call.

The only floating-point decision, "is this quantised probability at or above
the threshold", is taken HERE with numpy (`object_table`) and handed to the
device as a 256-entry table.  No CPU fallback: without the library / a GPU
every call raises.
"""

from __future__ import annotations

import collections
import ctypes
import threading

import numpy as np

from . import _lib
from . import _unit
from ._lib import check
from .inference import storage

#: one pair point: probs u8 [2, Z, Y, X] over the resegmentation box, seg u64
#: [z, y, x] over the analysis crop, which starts at offset_zyx inside the box
PairInput = collections.namedtuple(
    'PairInput', ['probs', 'seg', 'offset_zyx', 'id_a', 'id_b'])
#: one endpoint point: probs u8 [Z, Y, X], seg u64 [Z, Y, X]; id: the seeding
#: segment, reported even without an overlap (None: overlapping ids only)
EndpointInput = collections.namedtuple('EndpointInput', ['probs', 'seg', 'id'],
                                       defaults=(None,))

#: order of the columns `pair_stats` returns
COUNT_NAMES = ('a', 'b', 'a_and_b', 'a_or_b', 's1', 's2', 'a_and_s1',
               'a_and_s2', 'b_and_s1', 'b_and_s2')
MASK_NAMES = ('a', 'b', 's1', 's2')


def object_table(threshold) -> np.ndarray:
  """table[q] = 1 where the quantised probability q counts as object: the
  reference's own expression (resegmentation_analysis.py:128-129, :140) on all
  256 byte values."""
  prob = storage.dequantize_probability(np.arange(256, dtype=np.uint8))
  prob = np.nan_to_num(prob)  # nans indicate unvisited voxels
  return np.ascontiguousarray(prob >= threshold, dtype=np.uint8)


def _table(table):
  table = np.ascontiguousarray(table, dtype=np.uint8)
  if table.shape != (256,):
    raise ValueError('the object table has 256 entries')
  return table


class Analyzer(_unit.Handle):
  """One stream + grow-only device scratch for resegmentation analysis."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_analyzer_create', 'ffn_analyzer_destroy', device_id)
    self.lock = threading.Lock()
    #: first row capacity of endpoint_overlaps (grown on demand)
    self.initial_cap = 1 << 14

  def pair_stats(self, batch, table, voxel_size_zyx=(1, 1, 1)):
    """(counts uint64 [n, 10] in COUNT_NAMES order, max_edt f64 [n, 4] in
    MASK_NAMES order) for a sequence of PairInput."""
    table = _table(table)
    n = len(batch)
    descs = (_lib.PairDesc * max(n, 1))()
    keep = []  # the arrays the descriptors point into
    for d, item in zip(descs, batch):
      probs = np.ascontiguousarray(item.probs, dtype=np.uint8)
      seg = np.ascontiguousarray(item.seg, dtype=np.uint64)
      if probs.ndim != 4 or probs.shape[0] != 2 or seg.ndim != 3:
        raise ValueError('pair point: probs [2, Z, Y, X] and seg [z, y, x] '
                         'expected, got %r and %r' % (probs.shape, seg.shape))
      keep.append((probs, seg))
      d.probs, d.seg = probs.ctypes.data, seg.ctypes.data
      d.id_a, d.id_b = int(item.id_a), int(item.id_b)
      d.box_zyx[:] = probs.shape[1:]
      d.off_zyx[:] = [int(v) for v in item.offset_zyx]
      d.shape_zyx[:] = seg.shape
    counts = np.zeros((n, len(COUNT_NAMES)), np.uint64)
    max_edt = np.zeros((n, len(MASK_NAMES)), np.float64)
    voxel = (ctypes.c_double * 3)(*[float(v) for v in voxel_size_zyx])
    with self.lock:
      check(self._lib.ffn_analyzer_pair_stats(
          self._h, descs, n, table.ctypes.data, voxel, counts.ctypes.data,
          max_edt.ctypes.data))
    del keep
    return counts, max_edt

  def endpoint_overlaps(self, batch, table):
    """[(num_new, {old id: (num_overlapping, num_original)})] for a sequence of
    EndpointInput; the dict holds every old id (0 included) that the new mask
    overlaps, and the point's own `id` if it occurs in seg at all."""
    table = _table(table)
    n = len(batch)
    descs = (_lib.EndpointDesc * max(n, 1))()
    keep = []
    for d, item in zip(descs, batch):
      probs = np.ascontiguousarray(item.probs, dtype=np.uint8)
      seg = np.ascontiguousarray(item.seg, dtype=np.uint64)
      if probs.ndim != 3 or probs.shape != seg.shape:
        raise ValueError('endpoint point: probs and seg of one 3d shape '
                         'expected, got %r and %r' % (probs.shape, seg.shape))
      keep.append((probs, seg))
      d.probs, d.seg = probs.ctypes.data, seg.ctypes.data
      d.shape_zyx[:] = seg.shape
      if item.id is not None:
        d.id, d.has_id = int(item.id), 1
    num_new = np.zeros(n, np.uint64)

    def call(cap):
      row_point = np.empty(cap, np.int32)
      row_old = np.empty(cap, np.uint64)
      row_counts = np.empty((cap, 2), np.uint32)
      found = ctypes.c_size_t(0)
      rc = self._lib.ffn_analyzer_endpoint_overlaps(
          self._h, descs, n, table.ctypes.data, cap, row_point.ctypes.data,
          row_old.ctypes.data, row_counts.ctypes.data, num_new.ctypes.data,
          ctypes.byref(found))
      return rc, found, (row_point, row_old, row_counts)

    with self.lock:
      m, (row_point, row_old, row_counts) = _unit.grow_until_fits(
          call, max(int(self.initial_cap), 1))
    del keep
    out = [(int(v), {}) for v in num_new]
    for k in range(m):
      out[row_point[k]][1][int(row_old[k])] = (int(row_counts[k, 0]),
                                               int(row_counts[k, 1]))
    return out

  def last_timing(self):
    """((pair kernel ms, voxels), (endpoint kernel ms, voxels)) of the last
    calls; uploads are not part of the kernel time."""
    ms = (ctypes.c_double * 2)()
    voxels = (ctypes.c_double * 2)()
    check(self._lib.ffn_analyzer_last_timing(self._h, ms, voxels))
    return (ms[0], voxels[0]), (ms[1], voxels[1])


_default = _unit.Registry(Analyzer)


def default_analyzer(device_id: int = 0) -> Analyzer:
  """Process-wide Analyzer of a device (created on first use)."""
  return _default.get(device_id)
