"""Agglomeration decision points on the GPU.

A decision point of two segments is a place where they come closest: the list
of `(id_a, id_b, point)` entries a `ResegmentationRequest` is made of.  Every
segment is expanded into the unlabelled gaps (nearest labelled voxel, ties to
the smallest id), contacts between different expanded segments are collected,
and per pair of ids the contact of least distance is kept.  The per-voxel work
runs in HIP kernels (`ffn_amd.decision`); what comes back is a short list of
equally good contacts per pair, and the final choice among them is made here.

The volume may be a host array, int32 labels in HBM (a CUDA/HIP tensor or a
`(pointer, shape_zyx)` tuple, e.g. what `ffn_amd.distributed` assembles) or a
`DeviceCanvas`, so that an assembled volume never visits the host.
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .. import decision


def select_points(candidates) -> Dict[Tuple[int, int], Tuple[float, np.ndarray]]:
  """Final choice among the minimising candidates of every id pair.

  Args:
    candidates: dict of equally long arrays a, b, dist, off, z, y, x as
      `DecisionOps.contact_minima` returns them (any order; a voxel listed
      under several offsets counts once per listing).

  Returns:
    {(id_a, id_b): (dist, np.array([x, y, z]))} in ascending key order: per
    pair, with its candidates in (off, z, y, x) order, the first one whose
    squared distance to the mean candidate coordinate is smallest.
  """
  a = np.asarray(candidates['a'], np.uint64)
  if not a.size:
    return {}
  b = np.asarray(candidates['b'], np.uint64)
  order = np.lexsort((candidates['x'], candidates['y'], candidates['z'],
                      candidates['off'], b, a))
  a, b = a[order], b[order]
  dist = np.asarray(candidates['dist'], np.float64)[order]
  xyz = np.stack([np.asarray(candidates[k])[order] for k in 'xyz'],
                 axis=1).astype(np.int64)
  first = np.ones(a.size, bool)
  first[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
  starts = np.nonzero(first)[0]
  counts = np.diff(np.append(starts, a.size))
  mean = np.add.reduceat(xyz, starts, axis=0) / counts[:, None].astype(np.float64)
  spread = np.sum(np.square(xyz - np.repeat(mean, counts, axis=0)), axis=1)
  best = np.minimum.reduceat(spread, starts)
  # first row of every group that attains the group's minimum
  hit = np.nonzero(spread == np.repeat(best, counts))[0]
  group = np.repeat(np.arange(starts.size), counts)[hit]
  pick = hit[np.searchsorted(group, np.arange(starts.size))]
  return {(int(a[s]), int(b[s])): (dist[s], xyz[p])
          for s, p in zip(starts, pick)}


def _crop(subvol_box, shape):
  """(lo_zyx, hi_zyx) of a `subvol_box` within a volume of `shape`, clipped the
  way the slices of `to_slice3d()` clip."""
  if subvol_box is None:
    return None
  if hasattr(subvol_box, 'to_slice3d'):
    slices = subvol_box.to_slice3d()
  else:
    start, size = subvol_box
    slices = tuple(slice(int(s), int(s) + int(n))
                   for s, n in zip(list(start)[::-1], list(size)[::-1]))
  lo, hi = [], []
  for sl, n in zip(slices, shape):
    s, e, step = sl.indices(n)
    if step != 1:
      raise ValueError('subvol_box must select a contiguous box')
    lo.append(s)
    hi.append(max(e, s))
  return lo, hi


def _tensor_device(seg) -> Optional[int]:
  """Device index of a device tensor, None for every other kind of input."""
  if not hasattr(seg, 'data_ptr'):
    return None
  import torch  # pylint:disable=g-import-not-at-top
  if (seg.dtype != torch.int32 or not seg.is_cuda or not seg.is_contiguous()
      or seg.dim() != 3):
    raise TypeError('device labels must be a contiguous 3d int32 tensor')
  return seg.device.index or 0


def _expand(ops, seg, voxel_size, max_distance):
  """Runs stage 1 for any supported kind of `seg`."""
  handle = getattr(seg, 'canvas_handle', None)
  if handle is None and hasattr(getattr(seg, 'segmentation', None),
                                'canvas_handle'):
    handle = seg.segmentation.canvas_handle  # a DeviceCanvas
  if handle is not None:
    ops.expand_canvas(handle(), voxel_size, max_distance)
  elif hasattr(seg, 'data_ptr'):  # a device tensor
    import torch  # pylint:disable=g-import-not-at-top
    if _tensor_device(seg) != ops.device_id:
      raise ValueError('labels live on device %r, the kernels run on device %d'
                       % (seg.device.index, ops.device_id))
    torch.cuda.synchronize(seg.device)
    ops.expand_device(seg.data_ptr(), tuple(seg.shape), voxel_size,
                      max_distance)
  elif (isinstance(seg, tuple) and len(seg) == 2 and
        isinstance(seg[0], (int, np.integer))):
    ops.expand_device(int(seg[0]), seg[1], voxel_size, max_distance)
  else:
    ops.expand(np.asarray(seg), voxel_size, max_distance)


def find_decision_points(
    seg, voxel_size: Sequence[float], max_distance: Optional[float] = None,
    subvol_box=None, optimize_sparse: bool = False,
    sparse_noise_threshold: int = 0, device_id: Optional[int] = None,
) -> Dict[Tuple[int, int], Tuple[float, np.ndarray]]:
  """Per pair of touching expanded segments, the contact where they are closest.

  Args:
    seg: 3d label volume (zyx): host array, int32 device tensor,
      `(device pointer, shape_zyx)` or a `DeviceCanvas` (values <= 0 of the
      device forms are unlabelled)
    voxel_size: physical voxel size, xyz
    max_distance: largest distance (units of voxel_size) a segment is expanded
      by; None = unlimited
    subvol_box: where to look for decision points, an object with
      `to_slice3d()` or `(start_xyz, size_xyz)`; the expansion always uses the
      whole volume
    optimize_sparse: for a host array: count the segments first, drop those
      below sparse_noise_threshold, and return {} at once if fewer than two
      are left.  For the device forms the flag does nothing (it is an early
      exit plus dust removal, and the volume is not on the host to count)
    sparse_noise_threshold: with optimize_sparse, the voxel count below which
      a segment is neither counted nor searched
    device_id: the GPU to run on; default: the device of a device tensor,
      else 0.  A device tensor on another device than device_id is refused
      (a canvas is checked by the library); a raw (pointer, shape) tuple
      cannot be checked: the caller vouches that it is memory of that device

  Returns:
    {(id_a, id_b): (distance, np.array([x, y, z]))}, id_a < id_b, coordinates
    relative to subvol_box.
  """
  if optimize_sparse and isinstance(seg, np.ndarray):
    from ..inference import segmentation  # pylint:disable=g-import-not-at-top
    # (the count removes segments below the threshold, and the search goes on
    # without them, as in the reference -- but on a copy: the caller's array
    # is left alone)
    seg = seg.copy()
    _, counts = segmentation.clean_up_and_count(
        seg, split_cc=False, min_size=sparse_noise_threshold,
        compute_id_map=False, device_id=device_id)
    if counts is not None and sum(1 for label in counts if label > 0) < 2:
      return {}  # nothing for a segment to touch
  if device_id is None:
    device_id = _tensor_device(seg) or 0
  ops = decision.default_ops(device_id)
  with ops.lock:
    _expand(ops, seg, voxel_size, max_distance)
    candidates = ops.contact_minima(_crop(subvol_box, ops.shape))
  return select_points(candidates)


def to_resegmentation_points(points, request, subvol_box=None):
  """Appends one ResegmentationPoint per decision point, in ascending key
  order, to `request` (a ResegmentationRequest); coordinates are moved from the
  crop of `subvol_box` back to the volume.  Returns the request."""
  origin = np.zeros(3, np.int64)
  if subvol_box is not None:
    if hasattr(subvol_box, 'to_slice3d'):
      origin = np.array([max(int(s.start or 0), 0)
                         for s in subvol_box.to_slice3d()][::-1], np.int64)
    else:
      origin = np.array([max(int(v), 0) for v in subvol_box[0]], np.int64)
  for (id_a, id_b) in sorted(points):
    xyz = np.asarray(points[(id_a, id_b)][1], np.int64) + origin
    p = request.points.add()
    p.id_a, p.id_b = int(id_a), int(id_b)
    p.point.x, p.point.y, p.point.z = (int(v) for v in xyz)
  return request
