"""Scores a segmentation against ground truth and ground-truth skeletons
(include/ffn_metrics.h).

The reference's manual ends its workflow with "evaluate the resulting
segmentations using metrics of interest ... we recommend skeleton metrics" and
ships no code for it.  Here the per-voxel and per-node work runs on the GPU and
returns small INTEGER tables (MetricOps.contingency, MetricOps.skeleton_edges);
every float is derived from those tables on the host by two pure functions
(segmentation_scores, skeleton_scores) that never touch the library.  The tables
are sorted, the sums run in that order, so a score is reproducible bit for bit.
No CPU fallback: without the library / a GPU the MetricOps calls raise.

Volumes are numpy arrays (uploaded) or torch device tensors (scored in place
through their data_ptr: the device assembly of ffn_amd.distributed, or a tensor
filled by labels.LabelOps.copy_canvas, never leave the GPU), 4 or 8 bytes per
voxel, each with a width of its own.

Contingency tables are additive: a sharded caller scores every sub-box's core
(`core=`) on its own GPU and sums the tables on the host.
"""

from __future__ import annotations

import ctypes
import threading
from typing import Any, Dict, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from . import _unit

#: per-edge class of skeleton_edges (include/ffn_metrics.h FFN_EDGE_*)
OMITTED, MERGED, SPLIT, CORRECT = 0, 1, 2, 3
EDGE_CLASSES = ('omitted', 'merged', 'split', 'correct')
#: fixed point of an edge length: 1 / LENGTH_UNIT physical units
LENGTH_UNIT = 1024
_MAX_ID = 2**32 - 1  # ids on the device are below this


class ContingencyTable(NamedTuple):
  """n_ij: voxels with ground-truth id gt_ids[k] and segment id seg_ids[k],
  sorted by (gt id, seg id).  All uint64."""
  gt_ids: np.ndarray
  seg_ids: np.ndarray
  counts: np.ndarray


class Skeletons(NamedTuple):
  """Ground-truth skeletons: nodes_zyx (n, 3) voxel coordinates, node_skeleton
  (n,) non-zero skeleton id per node, edges (e, 2) node indices (both ends in
  one skeleton), voxel_size_zyx the physical size of a voxel."""
  nodes_zyx: np.ndarray
  node_skeleton: np.ndarray
  edges: np.ndarray
  voxel_size_zyx: Sequence[float] = (1.0, 1.0, 1.0)


class SkeletonEdges(NamedTuple):
  """Integer result of MetricOps.skeleton_edges.  class_counts / class_lengths:
  edges and summed fixed-point length per class (OMITTED .. CORRECT); runs:
  summed length of the correct edges of run_skeletons[k] inside
  run_segments[k], sorted by (skeleton, segment); mergers: sorted segment ids;
  node_segment / edge_class: per node / per edge."""
  class_counts: np.ndarray
  class_lengths: np.ndarray
  run_skeletons: np.ndarray
  run_segments: np.ndarray
  run_lengths: np.ndarray
  mergers: np.ndarray
  node_segment: np.ndarray
  edge_class: np.ndarray


def edge_lengths_q(skeletons: Skeletons) -> np.ndarray:
  """uint32 round(1024 * |delta_zyx * voxel_size_zyx|) per edge, in f64."""
  nodes = np.asarray(skeletons.nodes_zyx, np.float64).reshape(-1, 3)
  edges = np.asarray(skeletons.edges, np.int64).reshape(-1, 2)
  size = np.asarray(skeletons.voxel_size_zyx, np.float64).reshape(3)
  delta = (nodes[edges[:, 0]] - nodes[edges[:, 1]]) * size
  q = np.rint(LENGTH_UNIT * np.sqrt((delta * delta).sum(1)))
  if q.size and q.max() >= 2.0**32:
    raise ValueError('edge length %g overflows the 1/1024 fixed point' %
                     (q.max() / LENGTH_UNIT))
  return q.astype(np.uint32)


def _i64x3(v):
  return (ctypes.c_int64 * 3)(*[int(x) for x in v])


class _Volume:
  """A label volume as the library takes it: pointer, width, where it lives;
  `ids` maps compacted ids back (None: ids are themselves)."""

  def __init__(self, ptr, elem_bytes, on_device, shape, keep, ids=None):
    self.ptr, self.elem_bytes, self.on_device = ptr, elem_bytes, on_device
    self.shape, self.keep, self.ids = tuple(shape), keep, ids

  def restore(self, ids: np.ndarray) -> np.ndarray:
    return ids if self.ids is None else self.ids[ids.astype(np.int64)]


def _is_tensor(vol) -> bool:
  return hasattr(vol, 'data_ptr') and hasattr(vol, 'is_contiguous')


def _as_volume(vol, device_id: int) -> _Volume:
  if _is_tensor(vol):
    import torch  # pylint:disable=g-import-not-at-top
    if vol.device.type != 'cuda' or (vol.device.index or 0) != device_id:
      raise ValueError('tensor lives on %s, the handle on GPU %d' %
                       (vol.device, device_id))
    if vol.is_floating_point() or vol.element_size() not in (4, 8):
      raise TypeError('label tensors must be 4- or 8-byte integers, got %s' %
                      vol.dtype)
    if not vol.is_contiguous():
      raise ValueError('label tensors must be contiguous')
    torch.cuda.synchronize(vol.device)  # whatever filled it has finished
    return _Volume(vol.data_ptr(), vol.element_size(), 1, vol.shape, vol)
  arr = np.asarray(vol)
  if arr.dtype.kind not in 'iu':
    raise TypeError('label arrays must be integer, got %s' % arr.dtype)
  if arr.dtype.itemsize < 4:
    arr = arr.astype(np.uint32)
  if arr.dtype.kind == 'i' and arr.size and arr.min() < 0:
    arr = np.maximum(arr, 0)  # a canvas' -1 "excluded" markers
  ids = None
  if arr.dtype.itemsize == 8 and arr.size and int(arr.max()) >= _MAX_ID:
    # wider ids: score compacted ones, give the real ones back
    ids, inverse = np.unique(arr, return_inverse=True)
    ids = ids.astype(np.uint64)
    if ids[0] != 0:  # 0 stays 0: "unlabelled" / "outside" on the device
      ids = np.concatenate([np.zeros(1, np.uint64), ids])
      inverse = inverse + 1
    if len(ids) >= _MAX_ID:
      raise ValueError('more than 2**32 - 2 distinct ids')
    arr = inverse.reshape(arr.shape).astype(np.uint32)
  arr = np.ascontiguousarray(arr)
  return _Volume(arr.ctypes.data, arr.dtype.itemsize, 0, arr.shape, arr, ids)


def _box(core, shape):
  """-> (lo, hi) ctypes arrays, or (None, None) for the whole volume."""
  if core is None:
    return None, None
  lo, hi = core
  if len(lo) != 3 or len(hi) != 3:
    raise ValueError('core is ((z0, y0, x0), (z1, y1, x1))')
  return _i64x3(lo), _i64x3(hi)


class MetricOps(_unit.Handle):
  """One stream + grow-only device scratch for the metric kernels on one GPU."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_metrics_create', 'ffn_metrics_destroy', device_id)
    self._lock = threading.Lock()

  def contingency(self, gt, seg, core=None,
                  ignore_gt_zero: bool = True) -> ContingencyTable:
    """Joint histogram of (gt id, seg id) over the volume, or over the half-open
    box core = ((z0, y0, x0), (z1, y1, x1)) of it (a margin left out).  With
    ignore_gt_zero, voxels whose ground truth is 0 (unlabelled) count nowhere.
    Tables of boxes that tile a volume add up to the volume's table."""
    a = _as_volume(gt, self.device_id)
    b = _as_volume(seg, self.device_id)
    if a.shape != b.shape or len(a.shape) != 3:
      raise ValueError('gt %r and seg %r must be 3d and of one shape' %
                       (a.shape, b.shape))
    shape = _i64x3(a.shape)
    lo, hi = _box(core, a.shape)

    def call(cap):
      pg = np.empty(cap, np.uint64)
      ps = np.empty(cap, np.uint64)
      pc = np.empty(cap, np.uint64)
      found = ctypes.c_size_t(0)
      rc = self._lib.ffn_metrics_contingency(
          self._h, ctypes.c_void_p(a.ptr), a.elem_bytes, a.on_device,
          ctypes.c_void_p(b.ptr), b.elem_bytes, b.on_device, shape, lo, hi,
          1 if ignore_gt_zero else 0, cap, pg.ctypes.data, ps.ctypes.data,
          pc.ctypes.data, ctypes.byref(found))
      return rc, found, (pg, ps, pc)

    with self._lock:
      m, (pg, ps, pc) = _unit.grow_until_fits(call, 1 << 15)
    pg, ps = a.restore(pg[:m]), b.restore(ps[:m])
    order = np.lexsort((ps, pg))
    return ContingencyTable(pg[order], ps[order], pc[:m][order])

  def skeleton_edges(self, seg, skeletons, merge_min_nodes: int = 2,
                     core=None) -> SkeletonEdges:
    """Classifies every skeleton edge against `seg` (see SkeletonEdges).

    skeletons: a Skeletons, or a mapping with its fields (an .npz).  A node
    outside the volume or `core` has segment 0.  A merger is a segment != 0 in
    which at least two skeletons have >= merge_min_nodes nodes each.  An edge
    is, by the first rule that applies, omitted (an end in segment 0), merged
    (an end in a merger), split (ends in two segments) or correct.  A RUN is
    all correct edges of one skeleton inside one segment, whether or not they
    are contiguous along the skeleton (the common table-based definition).
    """
    if not isinstance(skeletons, Skeletons):
      skeletons = Skeletons(
          skeletons['nodes_zyx'], skeletons['node_skeleton'],
          skeletons['edges'],
          skeletons['voxel_size_zyx'] if 'voxel_size_zyx' in skeletons
          else (1.0, 1.0, 1.0))
    nodes = np.ascontiguousarray(skeletons.nodes_zyx, np.int32).reshape(-1, 3)
    skel = np.ascontiguousarray(skeletons.node_skeleton, np.uint32).reshape(-1)
    edges = np.ascontiguousarray(skeletons.edges, np.int32).reshape(-1, 2)
    if skel.size != len(nodes):
      raise ValueError('one skeleton id per node')
    if not np.array_equal(skel, np.asarray(skeletons.node_skeleton).reshape(-1)):
      raise ValueError('skeleton ids must fit 32 bits')
    if skel.size and (skel.min() == 0 or skel.max() >= _MAX_ID):
      raise ValueError('skeleton ids must be in [1, 2**32 - 2]')
    if edges.size and (edges.min() < 0 or edges.max() >= len(nodes)):
      raise ValueError('edge with a node index out of range')
    if edges.size and np.any(skel[edges[:, 0]] != skel[edges[:, 1]]):
      raise ValueError('edge joins two skeletons')
    if int(merge_min_nodes) < 1:
      raise ValueError('merge_min_nodes must be >= 1')
    length = edge_lengths_q(skeletons._replace(nodes_zyx=nodes, edges=edges))
    s = _as_volume(seg, self.device_id)
    if len(s.shape) != 3:
      raise ValueError('seg must be 3d')
    shape = _i64x3(s.shape)
    lo, hi = _box(core, s.shape)
    counts = np.zeros(4, np.uint64)
    lengths = np.zeros(4, np.uint64)
    node_seg = np.zeros(len(nodes), np.uint32)
    edge_class = np.zeros(len(edges), np.uint8)

    def call(cap):
      rs = np.empty(cap, np.uint64)
      rg = np.empty(cap, np.uint64)
      rl = np.empty(cap, np.uint64)
      mg = np.empty(cap, np.uint64)
      n_runs = ctypes.c_size_t(0)
      n_mergers = ctypes.c_size_t(0)
      rc = self._lib.ffn_metrics_skeleton(
          self._h, ctypes.c_void_p(s.ptr), s.elem_bytes, s.on_device, shape, lo,
          hi, len(nodes), nodes.ctypes.data, skel.ctypes.data, len(edges),
          edges.ctypes.data, length.ctypes.data, int(merge_min_nodes),
          counts.ctypes.data, lengths.ctypes.data, cap, rs.ctypes.data,
          rg.ctypes.data, rl.ctypes.data, ctypes.byref(n_runs), cap,
          mg.ctypes.data, ctypes.byref(n_mergers), node_seg.ctypes.data,
          edge_class.ctypes.data)
      # one cap for both tables: the larger of the two has to fit
      found = ctypes.c_size_t(max(n_runs.value, n_mergers.value))
      return rc, found, (rs[:n_runs.value], rg[:n_runs.value],
                         rl[:n_runs.value], mg[:n_mergers.value])

    with self._lock:
      _, (rs, rg, rl, mg) = _unit.grow_until_fits(call, 1 << 12)
    rg, mg = s.restore(rg), s.restore(mg)
    order = np.lexsort((rg, rs))
    return SkeletonEdges(counts, lengths, rs[order], rg[order], rl[order],
                         np.sort(mg), s.restore(node_seg.astype(np.uint64)),
                         edge_class)

  def last_timing(self) -> Tuple[float, float]:
    """(kernel milliseconds, algorithmic HBM bytes) of the last call."""
    ms = ctypes.c_double(0)
    nbytes = ctypes.c_double(0)
    _lib.check(self._lib.ffn_metrics_last_timing(self._h, ctypes.byref(ms),
                                                 ctypes.byref(nbytes)))
    return ms.value, nbytes.value


_default = _unit.Registry(MetricOps)


def default_ops(device_id: int = 0) -> MetricOps:
  """Process-wide MetricOps of a device (created on first use)."""
  return _default.get(device_id)


# ---- floats, on the host, from the integer tables ------------------------------


def _group_sums(ids: np.ndarray, counts: np.ndarray):
  """-> (unique ids ascending, summed counts, index of every row's id)."""
  uniq, inverse = np.unique(ids, return_inverse=True)
  sums = np.zeros(len(uniq), np.uint64)
  np.add.at(sums, inverse, counts)
  return uniq, sums, inverse


def _sum_sq(values: np.ndarray) -> int:
  v = values.astype(object)
  return int((v * v).sum()) if len(v) else 0


def segmentation_scores(table: ContingencyTable, background: str = 'segment',
                        min_overlap: int = 1) -> Dict[str, Any]:
  """Voxel scores of a contingency table n_ij (a_i = sum_j n_ij, b_j =
  sum_i n_ij, N = sum n_ij).

  background='segment': segment id 0 is one more segment.  'singletons': every
  voxel of segment 0 is a segment of its own (FFN leaves voxels unfilled; one
  giant "0" segment would score as a merger) -- in closed form, a row (i, 0, c)
  gives c instead of c^2 to sum n^2 and to sum b^2, and c terms of size 1 to the
  entropies.

  Returns a dict: n_voxels; sum_sq_pairs / sum_sq_gt / sum_sq_seg (exact ints);
  rand_precision = sum n^2 / sum b^2, rand_recall = sum n^2 / sum a^2,
  adapted_rand_error = 1 - 2PR / (P + R); vi_split = H(seg | gt) and vi_merge =
  H(gt | seg) in bits, summed in the table's sorted order; n_objects,
  n_segments, n_split_objects (pieces > 1), n_missed_objects (pieces = 0),
  n_merging_segments (objects > 1), mean_best_iou; `objects` (per ground-truth
  id: size, pieces, best_segment, best_overlap, best_iou) and `segments` (per
  segment != 0: size, objects) as arrays.  Pieces and objects count overlaps >=
  min_overlap with segments != 0; the best segment is the segment != 0 of
  largest overlap (ties: the smaller id; none: 0 with IoU 0); IoU = overlap /
  (a_i + b_j - overlap), b_j counted over the scored voxels only.
  """
  if background not in ('segment', 'singletons'):
    raise ValueError("background must be 'segment' or 'singletons'")
  gt = np.asarray(table.gt_ids, np.uint64)
  seg = np.asarray(table.seg_ids, np.uint64)
  cnt = np.asarray(table.counts, np.uint64)
  order = np.lexsort((seg, gt))
  gt, seg, cnt = gt[order], seg[order], cnt[order]
  gt_ids, a, gt_idx = _group_sums(gt, cnt)
  seg_ids, b, seg_idx = _group_sums(seg, cnt)
  n = int(cnt.astype(object).sum()) if len(cnt) else 0
  single = (seg == 0) if background == 'singletons' else np.zeros(len(seg), bool)
  n_single = int(cnt[single].astype(object).sum()) if single.any() else 0
  sum_sq_pairs = _sum_sq(cnt[~single]) + n_single
  sum_sq_gt = _sum_sq(a)
  sum_sq_seg = _sum_sq(b[seg_ids != 0] if background == 'singletons' else b)
  sum_sq_seg += n_single
  precision = sum_sq_pairs / sum_sq_seg if sum_sq_seg else 1.0
  recall = sum_sq_pairs / sum_sq_gt if sum_sq_gt else 1.0
  are = (1.0 - 2.0 * precision * recall / (precision + recall)
         if precision + recall > 0 else 1.0)
  vi_split = vi_merge = 0.0
  if n:
    c = cnt.astype(np.float64)
    ai = a[gt_idx].astype(np.float64)
    bj = b[seg_idx].astype(np.float64)
    # a singleton row: c voxels, each alone in its segment (n = b = 1)
    split_terms = np.where(single, c * np.log2(ai), -c * np.log2(c / ai)) / n
    merge_terms = np.where(single, 0.0, -c * np.log2(c / bj)) / n
    for t in split_terms.tolist():
      vi_split += t
    for t in merge_terms.tolist():
      vi_merge += t
  # per object / per segment
  real = (seg != 0) & (cnt >= np.uint64(max(int(min_overlap), 0)))
  pieces = np.bincount(gt_idx[real], minlength=len(gt_ids)).astype(np.int64)
  best_segment = np.zeros(len(gt_ids), np.uint64)
  best_overlap = np.zeros(len(gt_ids), np.uint64)
  best_iou = np.zeros(len(gt_ids), np.float64)
  nz = np.flatnonzero(seg != 0)
  if len(nz):
    # rows are sorted by (gt, seg): the first row of the largest count wins ties
    rank = np.lexsort((seg[nz], -cnt[nz].astype(np.int64), gt_idx[nz]))
    rows = nz[rank]
    first = np.ones(len(rows), bool)
    first[1:] = gt_idx[rows][1:] != gt_idx[rows][:-1]
    rows = rows[first]
    o = gt_idx[rows]
    best_segment[o] = seg[rows]
    best_overlap[o] = cnt[rows]
    union = (a[o].astype(object) + b[seg_idx[rows]].astype(object) -
             cnt[rows].astype(object))
    best_iou[o] = [int(x) / int(u) for x, u in zip(cnt[rows], union)]
  seg_real = seg_ids != 0
  seg_objects = np.bincount(seg_idx[real], minlength=len(seg_ids))[seg_real]
  return {
      'background': background,
      'min_overlap': int(min_overlap),
      'n_voxels': n,
      'sum_sq_pairs': sum_sq_pairs,
      'sum_sq_gt': sum_sq_gt,
      'sum_sq_seg': sum_sq_seg,
      'rand_precision': precision,
      'rand_recall': recall,
      'adapted_rand_error': are,
      'vi_split': vi_split,
      'vi_merge': vi_merge,
      'n_objects': int(len(gt_ids)),
      'n_segments': int(seg_real.sum()),
      'n_split_objects': int((pieces > 1).sum()),
      'n_missed_objects': int((pieces == 0).sum()),
      'n_merging_segments': int((seg_objects > 1).sum()),
      'mean_best_iou': float(best_iou.mean()) if len(best_iou) else 0.0,
      'objects': {'id': gt_ids, 'size': a, 'pieces': pieces,
                  'best_segment': best_segment, 'best_overlap': best_overlap,
                  'best_iou': best_iou},
      'segments': {'id': seg_ids[seg_real], 'size': b[seg_real],
                   'objects': seg_objects.astype(np.int64)},
  }


def skeleton_scores(edges: SkeletonEdges) -> Dict[str, Any]:
  """Edge counts and length fractions per class, and the expected run length

    ERL = sum_runs L_r^2 / (1024 * sum_all-edges edge_len_q)

  in physical units, evaluated as an exact integer ratio and divided once.  A
  run L_r is all correct edges of one skeleton inside one segment, whether or
  not they are contiguous along the skeleton (the common table-based
  definition; a contiguity-based one needs connected components of the edge
  graph)."""
  counts = [int(v) for v in edges.class_counts]
  lengths = [int(v) for v in edges.class_lengths]
  total_edges, total_len = sum(counts), sum(lengths)
  out = {'n_edges': total_edges,
         'total_length': total_len / LENGTH_UNIT,
         'n_runs': int(len(edges.run_lengths)),
         'n_mergers': int(len(edges.mergers))}
  for k, name in enumerate(EDGE_CLASSES):
    out['%s_edges' % name] = counts[k]
    out['%s_edge_fraction' % name] = (counts[k] / total_edges
                                      if total_edges else 0.0)
    out['%s_length_fraction' % name] = (lengths[k] / total_len
                                        if total_len else 0.0)
  sum_sq_runs = _sum_sq(np.asarray(edges.run_lengths, np.uint64))
  out['sum_sq_run_lengths'] = sum_sq_runs
  out['expected_run_length'] = (sum_sq_runs / (LENGTH_UNIT * total_len)
                                if total_len else 0.0)
  return out


def to_json(scores: Mapping[str, Any], per_object: bool = False):
  """A scores dict as JSON-ready builtins; the per-object / per-segment arrays
  only with per_object."""
  out = {}
  for key, value in scores.items():
    if isinstance(value, dict):
      if per_object:
        out[key] = {k: np.asarray(v).tolist() for k, v in value.items()}
    elif isinstance(value, (np.integer, np.floating)):
      out[key] = value.item()
    else:
      out[key] = value
  return out
