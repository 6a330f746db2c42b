"""Numpy restatement of the reference's build_coordinates.py (test
infrastructure, no product code), and a record-by-record Python encoder of the
TFRecord / tf.train.Example bytes written from the format description in
include/ffn_coordinates.h.

Steps, as the reference's main() goes through them:
  1. crop every volume by the margin (here a margin of 0 means "no crop");
  2. per class != 255, ascending, of every volume in turn: totals[c] += count,
     and the C-order flat indices of the class are appended to the class's list
     as (volume, flat) rows -- the classes keep the order of first appearance;
  3. every class's rows are permuted and repeated cyclically up to the largest
     total, the blocks are concatenated in class order and shuffled;
  4. a row becomes centre = (mx + x, my + y, mz + z) and the volume's name.
"""
import struct

import numpy as np

IGNORE_PARTITION = 255


def crop_of(vol, margin):
  return vol[tuple(slice(m, n - m) for m, n in zip(margin, vol.shape))]


def class_lists(volumes, margin):
  """({class: total}, {class: (n, 2) int64 rows (volume, flat)}, crop shapes),
  the dicts in the order the classes first appear."""
  totals, rows, shapes = {}, {}, []
  for i, (_, vol) in enumerate(volumes):
    crop = crop_of(np.asarray(vol), margin)
    shapes.append(crop.shape)
    values, counts = np.unique(crop, return_counts=True)
    for value, count in zip(values, counts):
      if value == IGNORE_PARTITION:
        continue
      c = int(value)
      totals[c] = totals.get(c, 0) + int(count)
      flat = np.flatnonzero(crop == value)
      rows.setdefault(c, []).append(
          np.stack([np.full(len(flat), i, np.int64), flat.astype(np.int64)], 1))
  return totals, {c: np.concatenate(r) for c, r in rows.items()}, shapes


def coordinates_spec(volumes, margin, rng=None):
  """(centres (N, 3) int64 xyz, volume indices (N,), {class: total}) with the
  reference's own calls on (n, 2) arrays; rng is a RandomState or None for the
  global np.random."""
  rng = np.random if rng is None else rng
  mz, my, mx = [int(m) for m in margin]
  totals, rows, shapes = class_lists(volumes, (mz, my, mx))
  max_count = max(totals.values())  # ValueError when every voxel is 255
  table = np.concatenate(
      [np.resize(rng.permutation(rows[c]), (max_count, 2)) for c in totals], 0)
  rng.shuffle(table)
  centers = np.zeros((len(table), 3), np.int64)
  for i, shape in enumerate(shapes):  # (all rows of a volume at once)
    rows_i = table[:, 0] == i
    z, y, x = np.unravel_index(table[rows_i, 1], shape)
    centers[rows_i] = np.stack([mx + x, my + y, mz + z], 1)
  return centers, table[:, 0].copy(), totals


# ---- TFRecord / Example bytes, one record at a time ----------------------------


def _crc_entry(value):
  for _ in range(8):
    value = (value >> 1) ^ 0x82F63B78 if value & 1 else value >> 1
  return value


_CRC = [_crc_entry(i) for i in range(256)]


def crc32c(data):
  crc = 0xFFFFFFFF
  for byte in data:
    crc = _CRC[(crc ^ byte) & 0xFF] ^ (crc >> 8)
  return crc ^ 0xFFFFFFFF


def masked_crc(data):
  crc = crc32c(data)
  return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) % 2**32


def varint(value):
  value &= 2**64 - 1  # int64 on the wire: two's complement
  out = bytearray()
  while True:
    if value < 128:
      out.append(value)
      return bytes(out)
    out.append(value & 0x7F | 0x80)
    value >>= 7


def field(number, payload):
  """A length-delimited field."""
  return varint(number << 3 | 2) + varint(len(payload)) + payload


def example_bytes(center_xyz, name):
  """tf.train.Example{features{feature{"center": int64_list,
  "label_volume_name": bytes_list}}}, the entries in key order."""
  int64_list = field(1, b''.join(varint(int(v)) for v in center_xyz))
  center = field(1, b'center') + field(2, field(3, int64_list))
  bytes_list = field(1, name)
  volume = field(1, b'label_volume_name') + field(2, field(1, bytes_list))
  return field(1, field(1, center) + field(1, volume))


def record_bytes(payload):
  header = struct.pack('<Q', len(payload))
  return (header + struct.pack('<I', masked_crc(header)) + payload +
          struct.pack('<I', masked_crc(payload)))


def tfrecord_bytes(centers, volume_index, names):
  """Uncompressed TFRecord bytes of the rows; names are str."""
  encoded = [n.encode('utf-8') for n in names]
  return b''.join(record_bytes(example_bytes(c, encoded[int(i)]))
                  for c, i in zip(centers, volume_index))
