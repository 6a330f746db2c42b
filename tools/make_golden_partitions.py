#!/usr/bin/env python3
"""Mints tests/golden/ref_partitions.npz with the reference's own
compute_partitions (compute_partitions.py at the root of the google/ffn
checkout).

Runs in the build container only (needs the reference checkout and scipy).
The reference module is imported through tools/ref_shims and runs unmodified.
Two things stand in for its surroundings:

  * the input is passed as a view of an ndarray subclass whose __getitem__
    turns a list of slices into a tuple, which is how numpy < 1.23 read the
    reference's `seg_array[valid_sel]`;
  * for the mask case `storage.build_mask` is replaced by a function that
    returns the case's array; the summed-volume query over it and the `>= 1`
    test stay the reference's.

Per case the file holds the input volume, the parameters, the reference's
output and the count volume of the specification (tests/partitions_ref.py).
The minter asserts what each case is there for.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('FFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)
# (the reference's generated *_pb2 modules predate the installed protobuf)
os.environ['PROTOCOL_BUFFERS_PYTHON_IMPLEMENTATION'] = 'python'

import importlib.util  # noqa: E402

import numpy as np  # noqa: E402

import partitions_ref  # noqa: E402

# (by path: this repository's root has a compute_partitions.py of its own)
_spec = importlib.util.spec_from_file_location(
    'ref_compute_partitions', os.path.join(REF, 'compute_partitions.py'))
ref_cp = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref_cp)

GOLD = os.path.join(ROOT, 'tests', 'golden')
SAMPLE12 = [0.025, 0.05, 0.075, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9]
TIE_THRESHOLDS = [1 / 3, 10 / 27, 0.5, 2 / 3, 26 / 27, 1.0]
TIE_COUNTS = (9, 10, 18, 26, 27)
TILE = (8, 8, 64)  # output tile of the device kernel at small radii


class LegacyIndexArray(np.ndarray):
  """numpy < 1.23: a list of slices indexes like the tuple of them."""

  def __getitem__(self, idx):
    if isinstance(idx, list) and idx and all(isinstance(i, slice) for i in idx):
      idx = tuple(idx)
    return super().__getitem__(idx)


class _MaskConfigs:
  masks = ()


def holes(seg, seed, fraction):
  rng = np.random.RandomState(seed)
  seg = seg.copy()
  seg[rng.rand(*seg.shape) < fraction] = 0
  return seg


def cells(shape, n_labels, seed, hole_fraction=0.1, **kw):
  return holes(partitions_ref.voronoi_labels(shape, n_labels, seed, **kw),
               seed + 100, hole_fraction)


def ties_volume():
  """Two slabs with a few holes (27, 26, and 18 at their common face), a sheet
  one voxel thick (9) and one voxel on top of the sheet (10)."""
  seg = np.zeros((14, 16, 18), np.uint32)
  seg[:6] = 3
  seg[6:11] = 5
  seg = holes(seg, 7, 0.004)
  seg[11] = 0
  seg[12] = 8
  seg[13] = 0
  seg[13, 8, 9] = 8
  return seg


def thin_volume():
  seg = cells((24, 26, 28), 6, 17, hole_fraction=0.0, dtype=np.uint32)
  for i in range(24):  # a one-voxel diagonal line through the whole volume
    seg[i, i, i] = 99
  return seg


def make_cases():
  small = cells((20, 24, 28), 7, 1, dtype=np.uint32)
  sizes = np.unique(small[small > 0], return_counts=True)[1]
  dust = int(np.sort(sizes)[0]) + 1  # exactly the smallest label goes
  mask = np.zeros((30, 34, 38), bool)
  mask[0, 0, 0] = mask[29, 33, 37] = mask[14, 20, 11] = mask[15, 20, 11] = True
  big = cells((30, 34, 38), 60, 3, dtype=np.uint32, id_base=2, id_step=3)
  big_ids = np.unique(big[big > 0])
  return {
      'aniso': dict(seg=small, thresholds=[0.1, 0.3, 0.5, 0.8],
                    lom_radius=(3, 2, 1), min_size=dust),
      'zero_axis': dict(seg=small, thresholds=[0.1, 0.3, 0.5, 0.8],
                        lom_radius=(0, 2, 1), min_size=dust),
      'sample12': dict(seg=small, thresholds=SAMPLE12, lom_radius=(2, 2, 2),
                       min_size=dust),
      'unsorted': dict(seg=small, thresholds=[0.5, 0.2, 0.9],
                       lom_radius=(2, 2, 2), min_size=dust),
      'excl': dict(seg=small, thresholds=[0.1, 0.3, 0.5, 0.8],
                   lom_radius=(3, 2, 1), min_size=dust,
                   exclusion_regions=[(12, 10, 9, 2.5), (25, 21, 4, 4)]),
      'mask_whitelist': dict(seg=big, thresholds=SAMPLE12, lom_radius=(2, 3, 4),
                             min_size=200, mask=mask,
                             id_whitelist=[int(i) for i in big_ids[::2]]),
      'ties': dict(seg=ties_volume(), thresholds=TIE_THRESHOLDS,
                   lom_radius=(1, 1, 1), min_size=1),
      'solid_u32': dict(seg=np.full((44, 43, 42), 7, np.uint32),
                        thresholds=SAMPLE12, lom_radius=(20, 20, 20),
                        min_size=10000),
      'wide_x': dict(seg=cells((5, 5, 80), 5, 5, dtype=np.uint32),
                     thresholds=SAMPLE12, lom_radius=(32, 1, 1), min_size=1),
      'one_out': dict(seg=cells((7, 12, 14), 4, 6, dtype=np.uint32),
                      thresholds=SAMPLE12, lom_radius=(3, 2, 3), min_size=1),
      'many_labels': dict(seg=cells((48, 48, 48), 300, 8, hole_fraction=0.02,
                                    dtype=np.uint32),
                          thresholds=SAMPLE12, lom_radius=(3, 3, 3), min_size=1),
      'thin': dict(seg=thin_volume(), thresholds=SAMPLE12, lom_radius=(2, 2, 2),
                   min_size=10),
      'big_ids': dict(seg=cells((20, 24, 28), 7, 9, dtype=np.uint64,
                                id_base=2**32 + 11, id_step=2**20 + 1),
                      thresholds=[0.1, 0.3, 0.5, 0.8], lom_radius=(2, 2, 2),
                      min_size=100),
  }


def run_reference(case):
  seg = case['seg'].copy().view(LegacyIndexArray)
  mask = case.get('mask')
  build_mask = ref_cp.storage.build_mask
  if mask is not None:
    ref_cp.storage.build_mask = lambda *a, **k: mask.copy()
  try:
    corner, out = ref_cp.compute_partitions(
        seg, case['thresholds'], case['lom_radius'], case.get('id_whitelist'),
        case.get('exclusion_regions'),
        _MaskConfigs() if mask is not None else None, case['min_size'])
  finally:
    ref_cp.storage.build_mask = build_mask
  assert tuple(corner) == tuple(case['lom_radius'])
  return np.asarray(out)


def labels_per_tile(seg, radius_zyx):
  rz, ry, rx = radius_zyx
  centre = seg[rz:seg.shape[0] - rz, ry:seg.shape[1] - ry,
               rx:seg.shape[2] - rx]
  best = 0
  for z in range(0, centre.shape[0], TILE[0]):
    for y in range(0, centre.shape[1], TILE[1]):
      for x in range(0, centre.shape[2], TILE[2]):
        tile = centre[z:z + TILE[0], y:y + TILE[1], x:x + TILE[2]]
        best = max(best, len(np.unique(tile[tile > 0])))
  return best


def check_purpose(name, case, out, counts):
  """What each case is in the file for."""
  seg, radius = case['seg'], tuple(case['lom_radius'])[::-1]
  sizes = np.unique(seg[seg > 0], return_counts=True)[1]
  if name in ('aniso', 'zero_axis', 'sample12', 'unsorted', 'excl'):
    assert (sizes < case['min_size']).sum() == 1 and np.any(seg == 0)
    assert len(np.unique(out)) >= 3
  if name == 'zero_axis':
    assert 0 in case['lom_radius'] and out.shape[2] == seg.shape[2]
  if name == 'sample12':
    assert len(np.unique(out)) >= 8
  if name == 'excl':
    plain = partitions_ref.partitions_spec(seg, case['thresholds'],
                                           case['lom_radius'],
                                           min_size=case['min_size'])[0]
    assert np.any(plain != 255) and np.any(out == 255)
    whole = 0
    for x, y, z, r in case['exclusion_regions']:
      one = partitions_ref.in_spheres(out.shape, case['lom_radius'],
                                      [(x, y, z, r)])
      g = np.mgrid[:seg.shape[0], :seg.shape[1], :seg.shape[2]]
      full = ((g[2] - x)**2 + (g[1] - y)**2 + (g[0] - z)**2 <= r * r).sum()
      assert 0 < one.sum() <= full
      whole += one.sum() == full
    assert whole == 1  # the other sphere is cut by the output's edge
    assert any(float(r) != int(r) for _, _, _, r in case['exclusion_regions'])
  if name == 'mask_whitelist':
    assert np.any(out == 255) and np.any(out == 0) and np.any(
        (out > 0) & (out < 255))
    assert out[0, 0, 0] == 255 and out[-1, -1, -1] == 255
    assert (sizes < 200).any()
    kept = partitions_ref.background_cleared(seg, case['id_whitelist'], 200)
    assert 0 < len(np.unique(kept)) - 1 < len(sizes)
  if name == 'ties':
    present = set(np.unique(counts).tolist())
    assert present >= set(TIE_COUNTS), present
    # a count on a threshold takes the next class
    for c in TIE_COUNTS:
      assert c / 27 in TIE_THRESHOLDS
  if name == 'solid_u32':
    assert counts.min() == counts.max() == 41**3 > 65535 and out.size > 1
  if name == 'wide_x':
    assert max(case['lom_radius']) == 32 and out.size > 0
  if name == 'one_out':
    assert 1 in out.shape and out.size > 1
  if name == 'many_labels':
    assert len(sizes) > 250 and labels_per_tile(seg, radius) >= 16
  if name == 'thin':
    line = seg == 99
    assert line.sum() == 24 and np.all(np.ptp(np.argwhere(line), 0) == 23)
    centre = seg[radius[0]:-radius[0], radius[1]:-radius[1],
                 radius[2]:-radius[2]]
    assert np.all(counts[centre == 99] <= 5) and np.any(counts > 100)
  if name == 'big_ids':
    assert seg.dtype == np.uint64 and seg[seg > 0].min() >= 2**32


def main():
  cases = make_cases()
  out = {'cases': np.array(sorted(cases))}
  for name in sorted(cases):
    case = cases[name]
    ref = run_reference(case)
    spec, counts = partitions_ref.partitions_spec(
        case['seg'], case['thresholds'], case['lom_radius'],
        case.get('id_whitelist'), case.get('exclusion_regions'),
        case.get('mask'), case['min_size'])
    assert ref.dtype == np.uint8 and ref.shape == spec.shape, name
    assert np.array_equal(ref, spec), (name, int((ref != spec).sum()))
    check_purpose(name, case, ref, counts)
    out[name + '_seg'] = case['seg']
    out[name + '_thresholds'] = np.array(case['thresholds'], np.float64)
    out[name + '_lom_radius'] = np.array(case['lom_radius'], np.int64)
    out[name + '_min_size'] = np.array(case['min_size'], np.int64)
    if case.get('id_whitelist') is not None:
      out[name + '_id_whitelist'] = np.array(case['id_whitelist'], np.uint64)
    if case.get('exclusion_regions') is not None:
      out[name + '_exclusion_regions'] = np.array(case['exclusion_regions'],
                                                  np.float64)
    if case.get('mask') is not None:
      out[name + '_mask'] = np.packbits(case['mask'])
    out[name + '_partitions'] = ref
    # (in the narrowest type that holds them; the specification's are uint32)
    out[name + '_counts'] = counts.astype(np.min_scalar_type(int(counts.max())))
    print('%-15s shape %s radius %s -> %s  values %s' % (
        name, case['seg'].shape, case['lom_radius'], ref.shape,
        np.unique(ref).tolist()))
  dst = os.path.join(GOLD, 'ref_partitions.npz')
  np.savez_compressed(dst, **out)
  print('wrote', dst, os.path.getsize(dst), 'bytes')


if __name__ == '__main__':
  main()
