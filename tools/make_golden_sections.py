#!/usr/bin/env python3
"""Mints tests/golden/ref_sections.npz with the reference's own section
augmentations: misalignment, missing_section, out_of_focus_section and
grayscale_perturb of ffn/training/augmentation.py of the google/ffn checkout,
unmodified, imported through tools/ref_shims (TensorFlow, tf.transformations,
skimage.transform, connectomics.common.object_utils and
multidim_image_augmentation are stubs there: the four functions are numpy and
scipy.ndimage and call none of them).

Runs in the build container only (needs the reference checkout).  Per case:
np.random.seed(seed), then the functions whose keys the case's configuration
holds, in apply_section_augmentations' order, on the image box as float32 and
-- after seeding again -- as float64.  The label ids go through misalignment
as int64, and so does an all-one mask of their shape.  Stored per case: the
configuration (JSON), the seed, the final sizes, the margin, the image volume
(float32; the box read from it is the whole of it in y and x), the label
volume, both image outputs, the label output, and what the functions return
for their summaries (z_start, z indices, applied).  elastic_warp,
affine_transform, apply_rotation and random_contrast_brightness_adjustment
cannot run here and are not minted.
"""
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('FFN_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(ROOT, 'tools', 'ref_shims'))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden', 'ref_sections.npz')
MAX_BYTES = 300 * 1000

MISALIGN = dict(misalignment_skip_ratio=0.0, max_xy_offset=2,
                slip_vs_translate_ratio=0.5)
MISSING = dict(missing_section_skip_ratio=0.0,
               max_missing_section_indices_ratio=0.6)
BLUR = dict(outoffocus_skip_ratio=0.0, max_outoffocus_indices_ratio=0.6,
            max_filter_stdev=2.0)
GRAY = dict(grayscale_skip_ratio=0.0, max_contrast_factor=0.6,
            max_brightness_factor=0.6)
ALL = dict(MISALIGN, **MISSING, **BLUR, **GRAY)
SMALL = ((5, 9, 11), (3, 5, 7))
EVEN = ((6, 6, 6), (6, 6, 6))


def cases():
  """(name, config, seed, image final zyx, label final zyx, margin yx, image
  kind)."""
  out = []
  add = lambda *row: out.append(row)
  for seed in range(6):
    add('misalign_%d' % seed, MISALIGN, 10 + seed, *SMALL, (2, 2), 'u8')
  for seed in range(3):
    add('misalign_wrap_%d' % seed, MISALIGN, 20 + seed, *EVEN, (0, 0), 'u8')
  add('misalign_margin13', dict(MISALIGN, max_xy_offset=3), 23, *EVEN, (1, 3),
      'f32')
  for seed in range(4):
    add('missing_%d' % seed, MISSING, 30 + seed, *SMALL, (0, 0), 'u8')
  for seed in range(4):
    add('blur_%d' % seed, BLUR, 40 + seed, *SMALL, (0, 0), 'u8')
  add('blur_wide', dict(BLUR, max_filter_stdev=6.0), 44, *SMALL, (0, 0), 'f32')
  add('blur_35x67', BLUR, 45, (2, 35, 67), (2, 35, 67), (0, 0), 'u8')
  for seed in range(4):
    add('gray_%d' % seed, GRAY, 50 + seed, *SMALL, (0, 0), 'u8')
  add('gray_strong', dict(GRAY, max_brightness_factor=2.0), 54, *SMALL, (0, 0),
      'f32')
  for seed in range(8):
    add('all_%d' % seed, ALL, 60 + seed, *SMALL, (2, 2), 'u8')
  for seed in range(3):
    add('all_skips_%d' % seed,
        {k: (0.5 if k.endswith('skip_ratio') else v) for k, v in ALL.items()},
        70 + seed, *EVEN, (2, 2), 'f32')
  add('all_35x67', ALL, 80, (3, 35, 67), (3, 33, 65), (2, 2), 'u8')
  return out


def make_volumes(image_zyx, label_zyx, margin_yx, kind, seed):
  """An image volume that is exactly the enlarged image box (taller in z
  where the label patch is), and labels of a few ids of its shape."""
  rng = np.random.RandomState(1000 + seed)
  shape = (max(image_zyx[0], label_zyx[0]),
           max(image_zyx[1], label_zyx[1]) + 2 * margin_yx[0],
           max(image_zyx[2], label_zyx[2]) + 2 * margin_yx[1])
  if kind == 'u8':
    image = rng.randint(0, 256, shape).astype(np.float32)
  else:
    image = rng.uniform(0, 255, shape).astype(np.float32)
  labels = rng.randint(0, 4, shape).astype(np.int64)
  labels = np.repeat(np.repeat(labels[:, ::2, ::2], 2, 1), 2, 2)[
      :, :shape[1], :shape[2]]
  return image, np.ascontiguousarray(labels)


def box(volume, final_zyx, margin_yx):
  """The box of the final size plus margins around the volume's centre voxel
  (s - 1) // 2."""
  size = (final_zyx[0], final_zyx[1] + 2 * margin_yx[0],
          final_zyx[2] + 2 * margin_yx[1])
  sel = []
  for axis in range(3):
    c = (volume.shape[axis] - 1) // 2
    margin = 0 if axis == 0 else margin_yx[axis - 1]
    start = c - (final_zyx[axis] - 1) // 2 - margin
    assert start >= 0 and start + size[axis] <= volume.shape[axis]
    sel.append(slice(start, start + size[axis]))
  return volume[tuple(sel)]


def run_reference(ra, config, seed, image_box, label_box, image_zyx, label_zyx):
  """-> (image [z, y, x], labels, summaries) of the reference's functions."""
  to5 = lambda a: np.ascontiguousarray(a)[None, ..., None]
  np.random.seed(seed)
  patch, labels = to5(image_box), to5(label_box)
  summary = {'misalignment_z': -1, 'missing_z': [], 'outoffocus_z': [],
             'grayscale': 0}
  if 'max_xy_offset' in config:
    patch, labels, _, z = ra.misalignment(
        patch, labels, np.ones_like(labels), list(image_zyx), list(label_zyx),
        list(label_zyx), config['max_xy_offset'],
        config['slip_vs_translate_ratio'], config['misalignment_skip_ratio'])
    summary['misalignment_z'] = int(z)
  listed = lambda z: [] if np.ndim(z) == 0 else sorted(int(v) for v in z)
  if 'missing_section_skip_ratio' in config:
    patch, z = ra.missing_section(
        patch, config['max_missing_section_indices_ratio'],
        config['missing_section_skip_ratio'])
    summary['missing_z'] = listed(z)
  if 'outoffocus_skip_ratio' in config:
    patch, z = ra.out_of_focus_section(
        patch, config['max_outoffocus_indices_ratio'],
        config['max_filter_stdev'], config['outoffocus_skip_ratio'])
    summary['outoffocus_z'] = listed(z)
  if 'grayscale_skip_ratio' in config:
    patch, applied = ra.grayscale_perturb(
        patch, config['max_contrast_factor'], config['max_brightness_factor'],
        config['grayscale_skip_ratio'])
    summary['grayscale'] = int(applied)
  return np.asarray(patch)[0, ..., 0], np.asarray(labels)[0, ..., 0], summary


def main():
  warnings.simplefilter('ignore', DeprecationWarning)
  from ffn.training import augmentation as ra  # the reference's, unmodified
  out = {'cases': []}
  for name, config, seed, image_zyx, label_zyx, margin, kind in cases():
    image_volume, label_volume = make_volumes(image_zyx, label_zyx, margin,
                                              kind, seed)
    image_box = box(image_volume, image_zyx, margin)
    label_box = box(label_volume, label_zyx, margin)
    got = {}
    for dtype in (np.float32, np.float64):
      got[dtype] = run_reference(ra, config, seed, image_box.astype(dtype),
                                 label_box, image_zyx, label_zyx)
      assert got[dtype][0].dtype == dtype
      assert got[dtype][0].shape == tuple(image_zyx)
    (ref32, labels32, summary), (ref64, labels64, summary64) = (
        got[np.float32], got[np.float64])
    assert summary == summary64 and np.array_equal(labels32, labels64)
    assert labels32.shape == tuple(label_zyx)
    spread = float(np.abs(ref32.astype(np.float64) - ref64).max())
    print('%-18s %s  spread f32 - f64 %.3g' % (name, summary, spread))
    out['cases'].append(name)
    out[name + '_config'] = np.array(json.dumps(config, sort_keys=True))
    out[name + '_seed'] = np.int64(seed)
    out[name + '_sizes'] = np.array([image_zyx, label_zyx], np.int64)
    out[name + '_margin'] = np.array(margin, np.int64)
    # integer-valued images are stored as uint8
    out[name + '_image'] = (image_volume.astype(np.uint8) if kind == 'u8'
                            else image_volume)
    out[name + '_labels'] = label_volume.astype(np.uint8)
    out[name + '_ref32'] = ref32
    out[name + '_ref64'] = ref64
    out[name + '_ref_labels'] = labels32.astype(np.uint8)
    out[name + '_summary'] = np.array(json.dumps(summary, sort_keys=True))
  out['cases'] = np.array(out['cases'])
  np.savez_compressed(GOLD, **out)
  size = os.path.getsize(GOLD)
  print('%s: %d cases, %d bytes' % (GOLD, len(out['cases']), size))
  assert size < MAX_BYTES


if __name__ == '__main__':
  main()
