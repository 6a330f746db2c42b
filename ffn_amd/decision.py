"""Python handle over the decision point kernels of libffn_hip.so
(include/ffn_decision.h): nearest-segment expansion of a label volume and the
per-pair minimum-distance contacts between expanded segments.

The volume may be host data, int32 labels already in HBM, or the segmentation
of a live device canvas; results stay resident on the handle between the two
stages.  No CPU fallback: without the library / a GPU every call raises.
"""

from __future__ import annotations

import ctypes
import threading
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import _unit
from ._lib import check

_MAX_UINT32 = 2**32 - 1


def _f64x3(v):
  v = [float(x) for x in v]
  if len(v) != 3:
    raise ValueError('voxel_size must have 3 entries (xyz)')
  return (ctypes.c_double * 3)(*v)


def _i64x3(v):
  return (ctypes.c_int64 * 3)(*[int(x) for x in v])


class DecisionOps(_unit.Handle):
  """One stream + grow-only device scratch for the decision point kernels."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_decision_create', 'ffn_decision_destroy', device_id)
    self.lock = threading.Lock()
    self._shape = None   # of the resident expansion
    self._values = None  # original ids of a remapped (>= 2**32 - 1) input
    self._dtype = np.dtype(np.uint32)
    #: first output capacity of contact_minima (grown on demand)
    self.initial_cap = 1 << 16

  # -- stage 1: expansion ---------------------------------------------------------
  @staticmethod
  def _max_distance(max_distance):
    return -1.0 if max_distance is None else float(max_distance)

  def expand(self, seg: np.ndarray, voxel_size: Sequence[float],
             max_distance: Optional[float] = None):
    """Expands a host label volume; results stay on the device (see `read`)."""
    seg = np.asarray(seg)
    if seg.ndim != 3:
      raise ValueError('expected a 3d label volume, got shape %r' % (seg.shape,))
    if seg.dtype.kind not in 'iu':
      raise TypeError('label arrays must be integer, got %s' % seg.dtype)
    if max_distance is not None and not max_distance >= 0:
      raise ValueError('max_distance must be >= 0 or None')
    self._dtype = seg.dtype
    self._values = None
    if seg.dtype.kind == 'i':
      if seg.size and seg.min() < 0:
        raise ValueError('negative labels in a host volume')
    dev = seg
    if seg.dtype.itemsize == 8 and seg.size and seg.max() >= _MAX_UINT32:
      # order-preserving remap, so that "smallest id" means the same thing
      values, inverse = np.unique(seg, return_inverse=True)
      if values[0] != 0:
        values = np.concatenate([np.zeros(1, values.dtype), values])
        inverse = inverse + 1
      self._values = values
      dev = inverse.reshape(seg.shape).astype(np.uint32)
    elif seg.dtype.itemsize < 4:
      dev = seg.astype(np.uint32)
    dev = np.ascontiguousarray(dev)
    self._shape = None
    check(self._lib.ffn_decision_expand(
        self._h, dev.ctypes.data, dev.dtype.itemsize, _i64x3(seg.shape),
        _f64x3(voxel_size), self._max_distance(max_distance)))
    self._shape = tuple(seg.shape)

  def expand_device(self, ptr: int, shape, voxel_size: Sequence[float],
                    max_distance: Optional[float] = None):
    """Expands int32 labels in HBM at `ptr` (values <= 0 unlabelled), in place
    of an upload; the caller synchronises whatever wrote them."""
    self._dtype = np.dtype(np.int32)
    self._values = None
    self._shape = None
    check(self._lib.ffn_decision_expand_device(
        self._h, ctypes.c_void_p(int(ptr)), _i64x3(shape), _f64x3(voxel_size),
        self._max_distance(max_distance)))
    self._shape = tuple(int(v) for v in shape)

  def expand_canvas(self, canvas_handle, voxel_size: Sequence[float],
                    max_distance: Optional[float] = None):
    """Expands the segmentation of a live device canvas (ffn_canvas*)."""
    self._dtype = np.dtype(np.int32)
    self._values = None
    self._shape = None
    shape = (ctypes.c_int64 * 3)()
    check(self._lib.ffn_decision_expand_canvas(
        self._h, canvas_handle, _f64x3(voxel_size),
        self._max_distance(max_distance), shape))
    self._shape = tuple(int(v) for v in shape)

  @property
  def shape(self):
    return self._shape

  def _ids(self, ids: np.ndarray) -> np.ndarray:
    return ids if self._values is None else self._values[ids]

  def read(self) -> Tuple[np.ndarray, np.ndarray]:
    """(expanded, edt) of the resident expansion as host arrays."""
    if self._shape is None:
      raise _lib.FFNHipError('no expansion resident')
    expanded = np.empty(self._shape, np.uint32)
    edt = np.empty(self._shape, np.float64)
    check(self._lib.ffn_decision_read(self._h, expanded.ctypes.data,
                                      edt.ctypes.data))
    return self._ids(expanded).astype(self._dtype, copy=False), edt

  def watershed_expand(self, seg, voxel_size, max_distance=None):
    """`labels.watershed_expand(seg, voxel_size, max_distance)` as
    find_decision_points calls it: (expanded, edt)."""
    self.expand(seg, voxel_size, max_distance)
    return self.read()

  def watershed_expand_device(self, ptr, shape, voxel_size, max_distance=None):
    self.expand_device(ptr, shape, voxel_size, max_distance)
    return self.read()

  # -- stage 2: contacts ------------------------------------------------------------
  def contact_minima(self, sub_box=None):
    """All contact candidates at the minimum distance of their id pair, over
    the resident expansion cropped to sub_box = (lo_zyx, hi_zyx).

    Returns a dict of equally long arrays: a, b (uint64, a < b), dist (f64),
    off (offset number 0..6), z, y, x (relative to the crop); unsorted.
    """
    if self._shape is None:
      raise _lib.FFNHipError('no expansion resident')
    lo = hi = None
    if sub_box is not None:
      lo, hi = _i64x3(sub_box[0]), _i64x3(sub_box[1])

    def call(cap):
      pa = np.empty(cap, np.uint64)
      pb = np.empty(cap, np.uint64)
      dist = np.empty(cap, np.float64)
      off = np.empty((cap, 4), np.int32)
      found = ctypes.c_size_t(0)
      rc = self._lib.ffn_decision_contact_minima(
          self._h, lo, hi, cap, pa.ctypes.data, pb.ctypes.data,
          dist.ctypes.data, off.ctypes.data, ctypes.byref(found))
      return rc, found, (pa, pb, dist, off)

    m, (pa, pb, dist, off) = _unit.grow_until_fits(
        call, max(int(self.initial_cap), 1))
    return {'a': self._ids(pa[:m]).astype(np.uint64),
            'b': self._ids(pb[:m]).astype(np.uint64),
            'dist': dist[:m], 'off': off[:m, 0].copy(), 'z': off[:m, 1].copy(),
            'y': off[:m, 2].copy(), 'x': off[:m, 3].copy()}

  def last_timing(self):
    """((expand ms, bytes), (scan + reduce ms, bytes)) of the last calls."""
    ms = (ctypes.c_double * 2)()
    nbytes = (ctypes.c_double * 2)()
    check(self._lib.ffn_decision_last_timing(self._h, ms, nbytes))
    return (ms[0], nbytes[0]), (ms[1], nbytes[1])


_default = _unit.Registry(DecisionOps)


def default_ops(device_id: int = 0) -> DecisionOps:
  """Process-wide DecisionOps of a device (created on first use)."""
  return _default.get(device_id)
