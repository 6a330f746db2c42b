"""Numpy specification of the partition map (include/ffn_partitions.h): direct
neighbourhood counts, the class table, the exclusion spheres and the box-any of
the mask.  Test infrastructure; the product never imports it.

`per_label_restatement` has the cost structure of the reference's algorithm
(box sums over the whole volume once per label, O(labels x voxels)) in this
project's own words: separable windowed prefix sums and the class table.  The
benchmark times it as the CPU baseline.
"""
import numpy as np


def valid_shape(shape, radius_zyx):
  return tuple(max(0, int(n) - 2 * int(r)) for n, r in zip(shape, radius_zyx))


def _windows(vol, radius_zyx):
  """Yields the valid-region view of `vol` for every offset of the LOM box."""
  oz, oy, ox = valid_shape(vol.shape, radius_zyx)
  rz, ry, rx = radius_zyx
  for dz in range(2 * rz + 1):
    for dy in range(2 * ry + 1):
      for dx in range(2 * rx + 1):
        yield vol[dz:dz + oz, dy:dy + oy, dx:dx + ox]


def direct_counts(seg, radius_zyx):
  """count(v) = #{u in box(v): seg[u] == seg[v]} for seg[v] != 0, else 0
  (uint32, valid region)."""
  out_shape = valid_shape(seg.shape, radius_zyx)
  counts = np.zeros(out_shape, np.uint32)
  if 0 in out_shape:
    return counts
  rz, ry, rx = radius_zyx
  centre = seg[rz:rz + out_shape[0], ry:ry + out_shape[1],
               rx:rx + out_shape[2]]
  for window in _windows(seg, radius_zyx):
    counts += window == centre
  counts[centre == 0] = 0
  return counts


def box_any(mask, radius_zyx):
  """True where any voxel of the LOM box is masked (valid region)."""
  out = np.zeros(valid_shape(mask.shape, radius_zyx), bool)
  if out.size:
    for window in _windows(np.asarray(mask) != 0, radius_zyx):
      out |= window
  return out


def _fractions(counts, fov_volume):
  """count / V in f64 the way the reference gets it: an int32 array over the
  integer product of the diameters."""
  return np.asarray(counts, np.int32) / np.prod(np.array([fov_volume]))


def class_table(thresholds, fov_volume):
  """class_of[count], one count at a time: the class is the 1-based position
  of the first threshold above the fraction; with none above, one past the end
  if the fraction reaches the last threshold, else 0 (a NaN threshold)."""
  thresholds = [float(t) for t in thresholds]
  table = np.zeros(fov_volume + 1, np.uint8)
  for count in range(fov_volume + 1):
    fraction = _fractions([count], fov_volume)[0]
    for position, th in enumerate(thresholds, 1):
      if fraction < th:
        table[count] = position
        break
    else:
      if fraction >= thresholds[-1]:
        table[count] = len(thresholds) + 1
  return table


def class_table_fast(thresholds, fov_volume):
  """The same over all counts at once (for large boxes): one comparison
  matrix, counts down and thresholds across."""
  thresholds = np.array([float(t) for t in thresholds], np.float64)
  fraction = _fractions(np.arange(fov_volume + 1), fov_volume)
  above = fraction[:, None] < thresholds[None, :]
  table = np.where(fraction >= thresholds[-1], len(thresholds) + 1, 0)
  table = np.where(above.any(axis=1), above.argmax(axis=1) + 1, table)
  return table.astype(np.uint8)


def in_spheres(out_shape, corner_xyz, exclusion_regions):
  """True where an output voxel lies in a sphere (x, y, z, r), f64:
  ((hx - x)^2 + (hy - y)^2) + (hz - z)^2 <= r * r."""
  hit = np.zeros(out_shape, bool)
  if not hit.size or exclusion_regions is None:
    return hit
  hz, hy, hx = np.mgrid[:out_shape[0], :out_shape[1], :out_shape[2]]
  hz = (hz + int(corner_xyz[2])).astype(np.float64)
  hy = (hy + int(corner_xyz[1])).astype(np.float64)
  hx = (hx + int(corner_xyz[0])).astype(np.float64)
  for x, y, z, r in exclusion_regions:
    x, y, z, r = float(x), float(y), float(z), float(r)
    dx, dy, dz = hx - x, hy - y, hz - z
    hit |= (dx * dx + dy * dy) + dz * dz <= r * r
  return hit


def background_cleared(seg, id_whitelist=None, min_size=10000):
  """Copy of `seg` with dust and ids outside the whitelist set to 0."""
  seg = np.array(seg)
  ids, sizes = np.unique(seg, return_counts=True)
  keep = ids != 0
  if min_size > 0:
    keep &= sizes >= min_size
  if id_whitelist is not None:
    keep &= np.isin(ids, np.array([int(i) for i in id_whitelist if int(i) > 0],
                                  dtype=np.uint64).astype(ids.dtype))
  seg[np.isin(seg, ids[~keep])] = 0
  return seg


def partitions_spec(seg, thresholds, lom_radius, id_whitelist=None,
                    exclusion_regions=None, mask=None, min_size=10000):
  """(partitions uint8, counts uint32) over the valid region; lom_radius is
  (x, y, z)."""
  radius = tuple(int(r) for r in lom_radius)[::-1]
  work = background_cleared(seg, id_whitelist, min_size)
  counts = direct_counts(work, radius)
  fov_volume = int(np.prod([2 * r + 1 for r in radius]))
  out = class_table_fast([float(t) for t in thresholds], fov_volume)[counts]
  out[counts == 0] = 0
  out[in_spheres(out.shape, lom_radius, exclusion_regions)] = 255
  if mask is not None:
    out[box_any(mask, radius)] = 255
  return out, counts


# ---- box sums through prefix sums, and the per-label algorithm --------


def _window_sums(values, width, axis):
  """Sums of all runs of `width` consecutive elements along `axis`: the
  difference of a zero-led prefix sum with itself `width` places on."""
  lead = list(values.shape)
  lead[axis] = 1
  prefix = np.concatenate(
      [np.zeros(lead, np.int32), np.cumsum(values, axis=axis, dtype=np.int32)],
      axis=axis)
  def along(start, stop):
    return tuple(slice(start, stop) if k == axis else slice(None)
                 for k in range(values.ndim))

  return prefix[along(width, None)] - prefix[along(0, -width)]


def box_sums(flags, radius_zyx):
  """Number of set voxels in the LOM box of every valid centre (int32): the
  box is separable, so one windowed sum per axis."""
  sums = flags
  for axis, r in enumerate(radius_zyx):
    sums = _window_sums(sums, 2 * int(r) + 1, axis)
  return sums


def _centre(vol, radius_zyx):
  return vol[tuple(slice(r, n - r) for r, n in zip(radius_zyx, vol.shape))]


def table_counts(seg, radius_zyx):
  """direct_counts through one whole-volume prefix sum per label (for boxes
  too large to enumerate)."""
  centre = _centre(seg, radius_zyx)
  counts = np.zeros(centre.shape, np.uint32)
  for label in np.unique(centre):
    if label:
      here = centre == label
      counts[here] = box_sums(seg == label, radius_zyx)[here]
  return counts


def per_label_restatement(seg, thresholds, lom_radius, min_size=10000):
  """The partition map the way the reference goes about it: for every label
  of the volume in turn, box sums of its indicator over the whole volume, and
  classes for that label's own centres (here through the class table)."""
  seg = background_cleared(seg, None, min_size)
  radius = tuple(int(r) for r in lom_radius)[::-1]
  fov_volume = int(np.prod([2 * r + 1 for r in radius]))
  table = class_table_fast(thresholds, fov_volume)
  centre = _centre(seg, radius)
  output = np.zeros(centre.shape, np.uint8)
  for label in np.unique(seg):
    if label:
      here = centre == label
      output[here] = table[box_sums(seg == label, radius)[here]]
  return output


# ---- test volumes ------------------------------------------------------


def voronoi_labels(shape, n_labels, seed, dtype=np.uint64, id_base=1,
                   id_step=1):
  """Seeded Voronoi cells: every voxel takes the id of the nearest of
  `n_labels` random sites."""
  rng = np.random.RandomState(seed)
  sites = np.stack([rng.randint(0, n, n_labels) for n in shape], 1)
  grid = np.stack(np.mgrid[:shape[0], :shape[1], :shape[2]], -1).reshape(-1, 3)
  best = np.full(len(grid), np.inf)
  owner = np.zeros(len(grid), np.int64)
  for k, s in enumerate(sites):
    d = ((grid - s) ** 2).sum(1)
    closer = d < best
    best[closer] = d[closer]
    owner[closer] = k
  ids = (id_base + id_step * np.arange(n_labels, dtype=np.uint64)).astype(dtype)
  return ids[owner].reshape(shape)


class EmulatedPartitionOps:
  """PartitionOps whose device is the specification (no GPU): what the root
  script sees of ffn_amd.partitions."""

  def __init__(self):
    self._last = np.zeros((0, 0, 0), np.uint8)

  def compute(self, seg, thresholds, lom_radius, id_whitelist=None,
              exclusion_regions=None, mask=None, min_size=10000,
              return_counts=False):
    out, counts = partitions_spec(seg, thresholds, lom_radius, id_whitelist,
                                  exclusion_regions, mask, min_size)
    self._last = out
    return (out, counts) if return_counts else out

  def partition_counts(self):
    return np.array(np.unique(self._last, return_counts=True))
