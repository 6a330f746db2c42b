"""Python handle over the partition kernels of libffn_hip.so
(include/ffn_partitions.h): for every labelled voxel of a segmentation, the
number of equally labelled voxels inside its local object mask (LOM) box,
quantised by a list of thresholds -- compute_partitions of the reference's
compute_partitions.py.

The thresholds are applied once on the host, as a table over the possible
counts (`class_table`); the device only counts and indexes.  No CPU fallback:
without the library / a GPU every call that needs the device raises.
"""

from __future__ import annotations

import ctypes
import threading
from typing import Optional, Sequence

import numpy as np

from . import _lib
from . import _unit
from ._lib import check

MAX_RADIUS = 32
MAX_THRESHOLDS = 253
_MAX_VOXELS = 2**31


def class_table(thresholds: Sequence[float], fov_volume: int) -> np.ndarray:
  """class_of[count] for count = 0 .. fov_volume, evaluated as the reference
  does per voxel (compute_partitions.py:187-199): the count as an element of an
  int array, divided by the integer box volume, compared with Python floats;
  the first threshold that exceeds the fraction wins, fractions at or above the
  last threshold get len(thresholds) + 1, anything else stays 0."""
  thresholds = np.array([float(t) for t in thresholds], np.float64)
  fraction = np.arange(int(fov_volume) + 1, dtype=np.int32) / np.int64(
      fov_volume)
  above = fraction[:, None] < thresholds[None, :]  # counts x thresholds
  table = np.where(fraction >= thresholds[-1], len(thresholds) + 1, 0)
  table = np.where(above.any(axis=1), above.argmax(axis=1) + 1, table)
  return table.astype(np.uint8)


def _check_arguments(seg, thresholds, lom_radius, exclusion_regions, mask):
  """Returns (thresholds, radius_zyx, spheres) or raises before any device
  call."""
  if seg.ndim != 3:
    raise ValueError('expected a 3d label volume, got shape %r' % (seg.shape,))
  if seg.dtype.kind not in 'iu':
    raise TypeError('label arrays must be integer, got %s' % seg.dtype)
  if seg.size >= _MAX_VOXELS:
    raise ValueError('volumes of 2^31 voxels or more are not supported')
  thresholds = [float(t) for t in thresholds]
  if not 1 <= len(thresholds) <= MAX_THRESHOLDS:
    raise ValueError('need 1 to %d thresholds, got %d' %
                     (MAX_THRESHOLDS, len(thresholds)))
  radius = [int(r) for r in lom_radius]
  if len(radius) != 3 or any(r != v for r, v in zip(radius, lom_radius)):
    raise ValueError('lom_radius must be 3 integers (x, y, z)')
  if any(r < 0 or r > MAX_RADIUS for r in radius):
    raise ValueError('each LOM radius must be in 0..%d, got %r' %
                     (MAX_RADIUS, radius))
  spheres = np.zeros((0, 4), np.float64)
  if exclusion_regions is not None and len(exclusion_regions):
    spheres = np.ascontiguousarray(exclusion_regions, dtype=np.float64)
    if spheres.ndim != 2 or spheres.shape[1] != 4:
      raise ValueError('exclusion_regions must be (x, y, z, r) tuples')
  if mask is not None and tuple(np.shape(mask)) != tuple(seg.shape):
    raise ValueError('mask of shape %r for a volume of shape %r' %
                     (tuple(np.shape(mask)), tuple(seg.shape)))
  if seg.size:
    if seg.dtype.kind == 'i' and seg.min() < 0:
      raise ValueError('negative labels in a host volume')
    if seg.dtype == np.uint64 and seg.max() == np.iinfo(np.uint64).max:
      raise ValueError('label id 2^64 - 1 is not supported')
  return thresholds, radius[::-1], spheres


class PartitionOps(_unit.Handle):
  """One stream + grow-only device scratch for the partition kernels."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_partitions_create', 'ffn_partitions_destroy',
                     device_id)
    self.lock = threading.RLock()
    self._histogram = np.zeros(256, np.uint64)
    #: first capacity of the id list of label_sizes (grown on demand)
    self.initial_cap = 1 << 16

  def label_sizes(self, seg: np.ndarray):
    """Uploads `seg` (it stays resident) and returns (ids, voxel counts) of its
    distinct ids, 0 included, unsorted."""
    seg = np.asarray(seg)
    if seg.dtype.itemsize < 4:
      seg = seg.astype(np.uint32)
    seg = np.ascontiguousarray(seg)
    shape = (ctypes.c_int64 * 3)(*seg.shape)

    def call(cap):
      ids = np.empty(cap, np.uint64)
      sizes = np.empty(cap, np.uint64)
      found = ctypes.c_size_t(0)
      rc = self._lib.ffn_partitions_label_sizes(
          self._h, seg.ctypes.data, seg.dtype.itemsize, shape, cap,
          ids.ctypes.data, sizes.ctypes.data, ctypes.byref(found))
      return rc, found, (ids, sizes)

    m, (ids, sizes) = _unit.grow_until_fits(call, max(int(self.initial_cap), 1))
    return ids[:m], sizes[:m]

  def compute(self, seg: np.ndarray, thresholds: Sequence[float],
              lom_radius: Sequence[int], id_whitelist=None,
              exclusion_regions=None, mask: Optional[np.ndarray] = None,
              min_size: int = 10000, return_counts: bool = False):
    """Partition map of the valid region seg[rz:Z-rz, ry:Y-ry, rx:X-rx]
    (uint8); `lom_radius` is (x, y, z) as in the reference.

    Labels of fewer than `min_size` voxels and, with `id_whitelist`, labels not
    listed are background.  `exclusion_regions` are (x, y, z, r) spheres in
    input coordinates, `mask` a boolean volume of the input's shape; a voxel
    inside a sphere or with a masked voxel anywhere in its LOM box gets 255.
    `seg` is left unchanged.  With `return_counts` also the uint32 count
    volume (0 where the centre is background) is returned.
    """
    seg = np.asarray(seg)
    thresholds, radius, spheres = _check_arguments(
        seg, thresholds, lom_radius, exclusion_regions, mask)
    out_shape = tuple(max(0, n - 2 * r) for n, r in zip(seg.shape, radius))
    if 0 in out_shape:  # an axis shorter than the LOM diameter: nothing valid
      with self.lock:
        self._histogram = np.zeros(256, np.uint64)
      empty = np.zeros(out_shape, np.uint8)
      return (empty, np.zeros(out_shape, np.uint32)) if return_counts else empty
    fov_volume = int(np.prod([2 * r + 1 for r in radius]))
    table = class_table(thresholds, fov_volume)
    mask_u8 = None
    if mask is not None:
      mask_u8 = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    with self.lock:
      ids, sizes = self.label_sizes(seg)
      keep = ids != 0
      if min_size > 0:
        keep &= sizes >= np.uint64(min_size)
      if id_whitelist is not None:
        listed = [int(i) for i in id_whitelist]
        listed = np.array([i for i in listed if 0 < i < 2**64], np.uint64)
        keep &= np.isin(ids, listed)
      keep = np.ascontiguousarray(keep, dtype=np.uint8)
      check(self._lib.ffn_partitions_compute(
          self._h, ids.ctypes.data, keep.ctypes.data, len(ids),
          _lib.i3(radius), table.ctypes.data, table.size,
          None if mask_u8 is None else mask_u8.ctypes.data,
          spheres.ctypes.data if len(spheres) else None, len(spheres)))
      partitions = np.empty(out_shape, np.uint8)
      counts = np.empty(out_shape, np.uint32) if return_counts else None
      check(self._lib.ffn_partitions_read(
          self._h, partitions.ctypes.data,
          None if counts is None else counts.ctypes.data,
          self._histogram.ctypes.data))
    return (partitions, counts) if return_counts else partitions

  def partition_counts(self) -> np.ndarray:
    """np.array(np.unique(partitions, return_counts=True)) of the last result,
    from the device's histogram."""
    with self.lock:
      values = np.flatnonzero(self._histogram)
      return np.array([values.astype(np.int64),
                       self._histogram[values].astype(np.int64)])

  def last_timing(self):
    """((label sizes ms, bytes), (compute ms, bytes)) of the last calls."""
    ms = (ctypes.c_double * 2)()
    nbytes = (ctypes.c_double * 2)()
    check(self._lib.ffn_partitions_last_timing(self._h, ms, nbytes))
    return (ms[0], nbytes[0]), (ms[1], nbytes[1])


_default = _unit.Registry(PartitionOps)


def default_ops(device_id: int = 0) -> PartitionOps:
  """Process-wide PartitionOps of a device (created on first use)."""
  return _default.get(device_id)
