"""Specification of the segmentation metrics (include/ffn_metrics.h,
ffn_amd/metrics.py) in numpy and plain Python, written from the formulas of
DESIGN.md and independent of the product module: np.unique on packed keys for
the voxel table, loops over nodes and edges for the skeleton rules.  Nothing in
the reference computes these numbers; this file is the yardstick."""

import math

import numpy as np

OMITTED, MERGED, SPLIT, CORRECT = 0, 1, 2, 3


def _crop(vol, core):
  if core is None:
    return vol
  lo, hi = core
  return vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]


def contingency(gt, seg, core=None, ignore_gt_zero=True):
  """-> (gt_ids, seg_ids, counts), uint64, sorted by (gt id, seg id).  Ids
  must be < 2**32."""
  a = _crop(np.asarray(gt), core).astype(np.uint64).ravel()
  b = _crop(np.asarray(seg), core).astype(np.uint64).ravel()
  assert a.shape == b.shape
  if ignore_gt_zero:
    keep = a != 0
    a, b = a[keep], b[keep]
  assert not a.size or (a.max() < 2**32 and b.max() < 2**32)
  keys, counts = np.unique((a << np.uint64(32)) | b, return_counts=True)
  return (keys >> np.uint64(32), keys & np.uint64(0xffffffff),
          counts.astype(np.uint64))


def segmentation_scores(table, background='segment', min_overlap=1):
  """The scores of the issue, from exact Python integers and math.log2."""
  rows = [(int(i), int(j), int(c)) for i, j, c in zip(*table)]
  rows.sort()
  a, b = {}, {}
  for i, j, c in rows:
    a[i] = a.get(i, 0) + c
    b[j] = b.get(j, 0) + c
  n = sum(c for _, _, c in rows)
  singles = background == 'singletons'
  s_pairs = s_seg = 0
  vi_split = vi_merge = 0.0
  for i, j, c in rows:
    if singles and j == 0:
      s_pairs += c                      # c segments of one voxel: c * 1^2
      vi_split += c * -(1.0 / n) * math.log2(1.0 / a[i])
      # vi_merge: c terms of log2(1 / 1) = 0
    else:
      s_pairs += c * c
      vi_split += -(c / n) * math.log2(c / a[i])
      vi_merge += -(c / n) * math.log2(c / b[j])
  for j, size in b.items():
    s_seg += size if (singles and j == 0) else size * size
  s_gt = sum(size * size for size in a.values())
  p = s_pairs / s_seg if s_seg else 1.0
  r = s_pairs / s_gt if s_gt else 1.0
  objects = {}
  for i in sorted(a):
    mine = [(j, c) for ii, j, c in rows if ii == i and j != 0]
    pieces = sum(1 for _, c in mine if c >= min_overlap)
    best_j, best_c = 0, 0
    for j, c in mine:  # ascending j: a tie keeps the smaller id
      if c > best_c:
        best_j, best_c = j, c
    iou = best_c / (a[i] + b[best_j] - best_c) if best_c else 0.0
    objects[i] = dict(size=a[i], pieces=pieces, best_segment=best_j,
                      best_overlap=best_c, best_iou=iou)
  segments = {}
  for j in sorted(b):
    if j != 0:
      segments[j] = dict(size=b[j], objects=sum(
          1 for _, jj, c in rows if jj == j and c >= min_overlap))
  ious = [o['best_iou'] for o in objects.values()]
  return dict(
      n_voxels=n, sum_sq_pairs=s_pairs, sum_sq_gt=s_gt, sum_sq_seg=s_seg,
      rand_precision=p, rand_recall=r,
      adapted_rand_error=1.0 - 2.0 * p * r / (p + r) if p + r > 0 else 1.0,
      vi_split=vi_split, vi_merge=vi_merge,
      n_split_objects=sum(1 for o in objects.values() if o['pieces'] > 1),
      n_missed_objects=sum(1 for o in objects.values() if o['pieces'] == 0),
      n_merging_segments=sum(1 for s in segments.values() if s['objects'] > 1),
      mean_best_iou=sum(ious) / len(ious) if ious else 0.0,
      objects=objects, segments=segments)


def edge_lengths_q(nodes_zyx, edges, voxel_size_zyx):
  out = []
  for u, v in np.asarray(edges).reshape(-1, 2).tolist():
    d = [(float(nodes_zyx[u][k]) - float(nodes_zyx[v][k])) *
         float(voxel_size_zyx[k]) for k in range(3)]
    out.append(int(round(1024.0 * math.sqrt(d[0] * d[0] + d[1] * d[1] +
                                            d[2] * d[2]))))
  return np.asarray(out, np.uint32)


def skeleton_edges(seg, nodes_zyx, node_skeleton, edges, edge_len_q,
                   merge_min_nodes=2, core=None):
  """-> dict of the integer results: class_counts, class_lengths (4,), runs
  {(skeleton, segment): length}, mergers (sorted list), node_segment,
  edge_class."""
  seg = np.asarray(seg)
  lo, hi = core if core is not None else ((0, 0, 0), seg.shape)
  node_seg = []
  for z, y, x in np.asarray(nodes_zyx).reshape(-1, 3).tolist():
    inside = (lo[0] <= z < hi[0] and lo[1] <= y < hi[1] and lo[2] <= x < hi[2])
    node_seg.append(int(seg[z, y, x]) if inside else 0)
  skel = [int(s) for s in np.asarray(node_skeleton).tolist()]
  per = {}
  for s, k in zip(node_seg, skel):
    if s != 0:
      per[(s, k)] = per.get((s, k), 0) + 1
  qualified = {}
  for (s, _), c in per.items():
    if c >= merge_min_nodes:
      qualified[s] = qualified.get(s, 0) + 1
  mergers = sorted(s for s, q in qualified.items() if q >= 2)
  merger_set = set(mergers)
  counts, lengths, runs, classes = [0] * 4, [0] * 4, {}, []
  for (u, v), length in zip(np.asarray(edges).reshape(-1, 2).tolist(),
                            np.asarray(edge_len_q).tolist()):
    assert skel[u] == skel[v]
    su, sv = node_seg[u], node_seg[v]
    if su == 0 or sv == 0:
      cls = OMITTED
    elif su in merger_set or sv in merger_set:
      cls = MERGED
    elif su != sv:
      cls = SPLIT
    else:
      cls = CORRECT
      runs[(skel[u], su)] = runs.get((skel[u], su), 0) + int(length)
    classes.append(cls)
    counts[cls] += 1
    lengths[cls] += int(length)
  return dict(class_counts=np.asarray(counts, np.uint64),
              class_lengths=np.asarray(lengths, np.uint64), runs=runs,
              mergers=mergers, node_segment=np.asarray(node_seg, np.uint64),
              edge_class=np.asarray(classes, np.uint8))


def expected_run_length(result):
  """(sum L^2, 1024 * sum of all edge lengths) as exact integers, and their
  f64 ratio."""
  num = sum(v * v for v in result['runs'].values())
  den = 1024 * int(sum(int(v) for v in result['class_lengths']))
  return num, den, (num / den if den else 0.0)


def random_walk_skeletons(shape, n_skeletons, n_nodes, seed, slack=2):
  """Chains of `n_nodes` nodes: random walks with steps in {-1, 0, 1}^3,
  clipped to the volume grown by `slack` voxels on every side (so some nodes
  fall outside).  -> (nodes_zyx int32, node_skeleton uint32, edges int32)."""
  rng = np.random.RandomState(seed)
  nodes, skel, edges = [], [], []
  for k in range(n_skeletons):
    start = np.array([rng.randint(0, s) for s in shape])
    steps = rng.randint(-1, 2, (n_nodes, 3))
    steps[0] = 0
    walk = np.clip(start + np.cumsum(steps, 0), -slack,
                   np.asarray(shape) - 1 + slack)
    base = k * n_nodes
    nodes.append(walk)
    skel += [k + 1] * n_nodes
    edges += [(base + i, base + i + 1) for i in range(n_nodes - 1)]
  return (np.concatenate(nodes).astype(np.int32), np.asarray(skel, np.uint32),
          np.asarray(edges, np.int32))
