"""Python handle over the coordinate kernels of libffn_hip.so
(include/ffn_coordinates.h): balanced training coordinates from partition maps,
the reference's build_coordinates.py.

Every class other than 255 is resampled to the size of the largest one
(permuted, then repeated cyclically) and all rows are shuffled; a row is a
centre (x, y, z) and the volume it lies in.  The random draws come from numpy's
legacy MT19937 stream on the host, in the reference's order, so a seed gives the
reference's sequence; the device sorts the voxels by class, gathers the rows
and encodes them as TFRecord bytes.  No CPU fallback: without the library / a
GPU every call that needs the device raises.
"""

from __future__ import annotations

import ctypes
import gzip
import io
import struct
import threading
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _unit
from ._lib import check

IGNORE_PARTITION = 255
_MAX_VOXELS = 2**31
_MAX_ROWS = 2**31
#: rows per serialised window of write_tfrecord (about 80 MB of records)
DEFAULT_WINDOW = 1 << 20
#: zlib's own default, which is what TensorFlow's GZIP option uses
GZIP_LEVEL = 6


def check_volumes(volumes, margin):
  """Returns (names, crops as views, margin (mz, my, mx)) or raises before any
  device call: every limit of build() is checked here.  A margin of 0 on an
  axis means "no crop" there."""
  margin_in = tuple(margin)
  if len(margin_in) != 3:
    raise ValueError('margin must be 3 integers (z, y, x)')
  margin = [int(m) for m in margin_in]
  if any(m != v for m, v in zip(margin, margin_in)) or min(margin) < 0:
    raise ValueError('margin must be 3 non-negative integers, got %r' %
                     (margin_in,))
  if not volumes:
    raise ValueError('no partition volumes')
  names, crops = [], []
  for name, vol in volumes:
    if not isinstance(name, str) or not name or ':' in name:
      raise ValueError('volume names are non-empty strings without ":", got %r'
                       % (name,))
    vol = np.asarray(vol)
    if vol.ndim != 3:
      raise ValueError('expected a 3d partition map, got shape %r' %
                       (vol.shape,))
    if vol.dtype != np.uint8:
      raise TypeError('partition maps are uint8, got %s' % vol.dtype)
    if any(2 * m >= n for m, n in zip(margin, vol.shape)):
      raise ValueError('margin %r leaves nothing of a volume of shape %r' %
                       (tuple(margin), vol.shape))
    crop = vol[tuple(slice(m, n - m) for m, n in zip(margin, vol.shape))]
    if crop.size >= _MAX_VOXELS:
      raise ValueError('crops of 2^31 voxels or more are not supported')
    names.append(name)
    crops.append(crop)
  if not any((crop != IGNORE_PARTITION).any() for crop in crops):
    raise ValueError('every voxel is 255: max() arg is an empty sequence')
  if (IGNORE_PARTITION * sum(crop.size for crop in crops)) >= _MAX_ROWS:
    # only now can classes x max_count reach the limit: count on the host
    counts = sum(np.bincount(crop.reshape(-1), minlength=256) for crop in crops)
    check_rows({c: int(counts[c])
                for c in np.flatnonzero(counts[:IGNORE_PARTITION])})
  return names, crops, tuple(margin)


def check_rows(totals: Dict[int, int]) -> int:
  """max_count of the class totals; raises as the reference's max() does when
  every voxel is 255, and when the output would reach 2^31 rows."""
  if not totals:
    raise ValueError('every voxel is 255: max() arg is an empty sequence')
  max_count = max(totals.values())
  if len(totals) * max_count >= _MAX_ROWS:
    raise ValueError('%d classes x %d rows reach 2^31 output rows' %
                     (len(totals), max_count))
  return max_count


def _varint_len(v: int) -> int:
  return max(1, (int(v).bit_length() + 6) // 7)


def record_bound(name_len: int) -> int:
  """Most bytes one record (framing included) of a volume name of `name_len`
  bytes takes, whatever its centre: three 10-byte varints, which is the bound
  the library puts on a window (include/ffn_coordinates.h)."""
  ints = 3 * 10
  int_list = 1 + _varint_len(ints) + ints
  feat_c = 1 + _varint_len(int_list) + int_list
  entry_c = 2 + len('center') + 1 + _varint_len(feat_c) + feat_c
  byte_list = 1 + _varint_len(name_len) + name_len
  feat_n = 1 + _varint_len(byte_list) + byte_list
  entry_n = 2 + len('label_volume_name') + 1 + _varint_len(feat_n) + feat_n
  features = (1 + _varint_len(entry_c) + entry_c + 1 + _varint_len(entry_n) +
              entry_n)
  return 16 + 1 + _varint_len(features) + features


class CoordinateOps(_unit.Handle):
  """One stream + device storage for the coordinate kernels."""

  def __init__(self, device_id: int = 0):
    super().__init__('ffn_coordinates_create', 'ffn_coordinates_destroy',
                     device_id)
    self.lock = threading.RLock()
    self.num_rows = 0
    self.num_volumes = 0
    self._longest_name = 0
    #: wall seconds of the steps of the last build / write_tfrecord; the
    #: `*_kernels` entries are the device-event times inside those steps
    self.split = {}

  def reset(self):
    with self.lock:
      check(self._lib.ffn_coordinates_reset(self._h))
      self.num_rows = self.num_volumes = 0

  def add_volume(self, crop: np.ndarray) -> np.ndarray:
    """Sorts the flat indices of `crop` (uint8, 3-d) by value on the device and
    keeps the lists of the classes other than 255; returns the 256 counts."""
    crop = np.ascontiguousarray(crop, dtype=np.uint8)
    if crop.ndim != 3 or crop.size == 0 or crop.size >= _MAX_VOXELS:
      raise ValueError('expected a non-empty 3d crop of fewer than 2^31 voxels')
    counts = np.zeros(256, np.uint64)
    with self.lock:
      check(self._lib.ffn_coordinates_add_volume(
          self._h, crop.ctypes.data, (ctypes.c_int64 * 3)(*crop.shape),
          counts.ctypes.data))
      self.num_volumes += 1
    return counts

  def class_list(self, volume: int, cls: int) -> np.ndarray:
    """The resident list of class `cls` of volume `volume`: ascending flat
    indices (uint32)."""

    def call(cap):
      flat = np.empty(cap, np.uint32)
      found = ctypes.c_size_t(0)
      rc = self._lib.ffn_coordinates_read_class(
          self._h, int(volume), int(cls), cap, flat.ctypes.data,
          ctypes.byref(found))
      return rc, found, flat

    with self.lock:
      n, flat = _unit.grow_until_fits(call, 1 << 12)
    return flat[:n]

  def gather(self, classes: Sequence[int], max_count: int,
             perms: Sequence[np.ndarray], order: np.ndarray, margin):
    """Output rows from the class order, one index vector per class and the
    order of all rows (include/ffn_coordinates.h); they stay on the device."""
    classes = np.ascontiguousarray(classes, dtype=np.uint8)
    perm = np.ascontiguousarray(np.concatenate(perms), dtype=np.uint32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    with self.lock:
      check(self._lib.ffn_coordinates_gather(
          self._h, classes.ctypes.data, len(classes), int(max_count),
          perm.ctypes.data, perm.size, order.ctypes.data, order.size,
          (ctypes.c_int32 * 3)(*[int(m) for m in margin])))
      self.num_rows = int(order.size)

  def read(self, row0: int = 0, n_rows: Optional[int] = None):
    """(centres (n, 3) int32 xyz, volume indices (n,) int32) of resident
    rows."""
    with self.lock:
      if n_rows is None:
        n_rows = self.num_rows - row0
      centers = np.empty((n_rows, 3), np.int32)
      volume_index = np.empty(n_rows, np.int32)
      check(self._lib.ffn_coordinates_read(
          self._h, int(row0), int(n_rows), centers.ctypes.data,
          volume_index.ctypes.data))
    return centers, volume_index

  def set_names(self, names: Sequence[str]):
    encoded = [n.encode('utf-8') for n in names]
    if not encoded or any(not e for e in encoded):
      raise ValueError('volume names must not be empty')
    blob = np.frombuffer(b''.join(encoded), np.uint8)
    offsets = np.zeros(len(encoded) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(e) for e in encoded])
    with self.lock:
      check(self._lib.ffn_coordinates_set_names(
          self._h, blob.ctypes.data, offsets.ctypes.data, len(encoded)))
      self._longest_name = max(len(e) for e in encoded)

  def serialize(self, row0: int, n_rows: int) -> bytes:
    """Rows [row0, row0 + n_rows) as uncompressed TFRecord bytes."""

    def call(cap):
      out = np.empty(cap, np.uint8)
      found = ctypes.c_size_t(0)
      rc = self._lib.ffn_coordinates_serialize(
          self._h, int(row0), int(n_rows), cap, out.ctypes.data,
          ctypes.byref(found))
      return rc, found, out

    with self.lock:
      n, out = _unit.grow_until_fits(
          call, max(record_bound(self._longest_name) * int(n_rows), 1))
    return out[:n].tobytes()

  def build(self, volumes, margin, rng=None):
    """Balanced, shuffled coordinates of `volumes`, a list of (name, uint8
    partition map zyx), cropped by `margin` = (z, y, x) voxels on every side.

    `rng` is a np.random.RandomState, or None for the global np.random, which
    is what the reference draws from.  The draws are the reference's, in its
    order: permutation(n_c) for every class in the order the classes first
    appear (a volume's classes ascending, volume after volume), then one
    shuffle of arange(K * max_count).

    A margin of 0 means "no crop" on that axis.  This differs from the
    reference on purpose: it slices [m:-m], so that 0 gives an empty crop and
    its max() over no class raises.

    Returns (centres (N, 3) int32 xyz, volume indices (N,) int32, {class: total}
    in that class order).  The rows stay resident for write_tfrecord.  The
    caller's arrays are not modified.
    """
    names, crops, margin = check_volumes(volumes, margin)
    rng = np.random if rng is None else rng
    split = {}
    with self.lock:
      self.reset()
      totals = {}
      kernel_s = [0.0]
      t0 = time.time()
      for crop in crops:
        counts = self.add_volume(crop)
        kernel_s[0] += self.last_timing()[0][0] * 1e-3
        for c in np.flatnonzero(counts[:IGNORE_PARTITION]):
          totals[int(c)] = totals.get(int(c), 0) + int(counts[c])
      split['sort'] = time.time() - t0
      split['sort_kernels'] = kernel_s[0]
      max_count = check_rows(totals)
      t0 = time.time()
      perms = [rng.permutation(n).astype(np.uint32) for n in totals.values()]
      order = np.arange(len(totals) * max_count, dtype=np.uint32)
      rng.shuffle(order)
      split['host_rng'] = time.time() - t0
      t0 = time.time()
      self.gather(list(totals), max_count, perms, order, margin)
      self.set_names(names)
      split['gather'] = time.time() - t0
      split['gather_kernels'] = self.last_timing()[1][0] * 1e-3
      t0 = time.time()
      centers, volume_index = self.read()
      split['read'] = time.time() - t0
      self.split = split
    return centers, volume_index, totals

  def write_tfrecord(self, path: str, names: Optional[Sequence[str]] = None,
                     window: int = DEFAULT_WINDOW,
                     compresslevel: int = GZIP_LEVEL):
    """Writes the resident rows as a GZIP-compressed TFRecord file of
    tf.train.Example{center, label_volume_name}, one device-serialised window
    of `window` rows at a time.  `names` replaces the names given to build().
    Returns the number of uncompressed bytes."""
    if window < 1:
      raise ValueError('window must be positive')
    total = 0
    t_device = t_gzip = t_kernels = 0.0
    with self.lock:
      if names is not None:
        if len(names) != self.num_volumes:
          raise ValueError('%d names for %d volumes' %
                           (len(names), self.num_volumes))
        self.set_names(names)
      with gzip.open(path, 'wb', compresslevel=compresslevel) as f:
        for row0 in range(0, self.num_rows, window):
          t0 = time.time()
          chunk = self.serialize(row0, min(window, self.num_rows - row0))
          t1 = time.time()
          t_kernels += self.last_timing()[2][0] * 1e-3
          f.write(chunk)
          t_gzip += time.time() - t1
          t_device += t1 - t0
          total += len(chunk)
      self.split = dict(self.split, serialize=t_device,
                        serialize_kernels=t_kernels, gzip=t_gzip)
    return total

  def last_timing(self):
    """((add_volume ms, bytes), (gather ms, bytes), (serialize ms, bytes)) of
    the last calls."""
    ms = (ctypes.c_double * 3)()
    nbytes = (ctypes.c_double * 3)()
    check(self._lib.ffn_coordinates_last_timing(self._h, ms, nbytes))
    return tuple((ms[k], nbytes[k]) for k in range(3))


_default = _unit.Registry(CoordinateOps)


def default_ops(device_id: int = 0) -> CoordinateOps:
  """Process-wide CoordinateOps of a device (created on first use)."""
  return _default.get(device_id)


# ---- reading the file back (pure Python / numpy) --------------------------------


def _crc_table():
  table = np.arange(256, dtype=np.uint32)
  for _ in range(8):
    table = np.where(table & 1, (table >> 1) ^ np.uint32(0x82F63B78),
                     table >> 1).astype(np.uint32)
  return [int(v) for v in table]


_CRC_TABLE = _crc_table()


def crc32c(data: bytes) -> int:
  """CRC-32C (Castagnoli), as TFRecord uses it."""
  crc = 0xFFFFFFFF
  table = _CRC_TABLE
  for b in data:
    crc = table[(crc ^ b) & 0xFF] ^ (crc >> 8)
  return crc ^ 0xFFFFFFFF


def masked_crc32c(data: bytes) -> int:
  crc = crc32c(data)
  return (((crc >> 15) | (crc << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _varint(buf: bytes, pos: int) -> Tuple[int, int]:
  result = 0
  shift = 0
  while True:
    b = buf[pos]
    pos += 1
    result |= (b & 0x7F) << shift
    if not b & 0x80:
      return result, pos
    shift += 7


def _fields(buf: bytes):
  """Protobuf wire-format walk -> (field, wire type, value) triples; only the
  varint and length-delimited types an Example of coordinates holds."""
  pos = 0
  while pos < len(buf):
    tag, pos = _varint(buf, pos)
    field, wt = tag >> 3, tag & 7
    if wt == 0:
      val, pos = _varint(buf, pos)
    elif wt == 2:
      ln, pos = _varint(buf, pos)
      if pos + ln > len(buf):
        raise ValueError('truncated field %d' % field)
      val = buf[pos:pos + ln]
      pos += ln
    else:
      raise ValueError('unsupported wire type %d' % wt)
    yield field, wt, val


def _one(buf: bytes, want: int) -> bytes:
  found = [val for field, wt, val in _fields(buf) if field == want and wt == 2]
  if len(found) != 1:
    raise ValueError('expected one field %d, found %d' % (want, len(found)))
  return found[0]


def parse_example(payload: bytes) -> Tuple[List[int], bytes]:
  """(centre [x, y, z], volume name) of one serialised tf.train.Example, its
  two entries in either order."""
  center = name = None
  for field, wt, entry in _fields(_one(payload, 1)):
    if field != 1 or wt != 2:
      raise ValueError('unexpected field %d in Features' % field)
    key, feature = _one(entry, 1), _one(entry, 2)
    if key == b'center':
      values = []
      for f, w, val in _fields(_one(feature, 3)):
        if f != 1:
          raise ValueError('unexpected field %d in Int64List' % f)
        if w == 0:  # not packed
          values.append(val)
          continue
        pos = 0
        while pos < len(val):
          v, pos = _varint(val, pos)
          values.append(v)
      center = [v - (1 << 64) if v >> 63 else v for v in values]
    elif key == b'label_volume_name':
      name = _one(_one(feature, 1), 1)
    else:
      raise ValueError('unexpected feature %r' % key)
  if center is None or name is None or len(center) != 3:
    raise ValueError('an example needs a 3-element center and a volume name')
  return center, name


def _read_exactly(f, n: int, pos: int) -> bytes:
  data = f.read(n)
  if len(data) != n:
    raise ValueError('truncated record at byte %d' % pos)
  return data


def iter_record_stream(f):
  """Payloads of the uncompressed TFRecord bytes a binary file object yields,
  read one record at a time; both CRCs of every record are verified."""
  pos = 0
  while True:
    header = f.read(8)
    if not header:
      return
    if len(header) != 8:
      raise ValueError('truncated record header at byte %d' % pos)
    (length,) = struct.unpack('<Q', header)
    (crc,) = struct.unpack('<I', _read_exactly(f, 4, pos))
    if crc != masked_crc32c(header):
      raise ValueError('length CRC mismatch at byte %d' % pos)
    pos += 12
    payload = _read_exactly(f, length, pos)
    (crc,) = struct.unpack('<I', _read_exactly(f, 4, pos))
    if crc != masked_crc32c(payload):
      raise ValueError('payload CRC mismatch at byte %d' % pos)
    pos += length + 4
    yield payload


def iter_records(data: bytes):
  """Payloads of uncompressed TFRecord bytes; both CRCs of every record are
  verified."""
  return iter_record_stream(io.BytesIO(data))


def read_tfrecord(path: str):
  """Reads a GZIP-compressed (or plain) TFRecord file of coordinates back into
  (centres (N, 3) int64 xyz, list of N volume names as str), verifying both
  CRCs of every record.  Needs neither TensorFlow nor the device.

  The file is streamed record by record, so memory holds the result and not
  the file; but the CRCs and the protobuf walk are byte-by-byte Python, some
  tens of microseconds a record.  It is meant for checking what was written,
  on small files or on a part of a large one, not as the input pipeline of a
  training run."""
  with open(path, 'rb') as f:
    magic = f.read(2)
  opener = gzip.open if magic == b'\x1f\x8b' else open
  centers, names = [], {}
  name_index = []
  with opener(path, 'rb') as f:
    for payload in iter_record_stream(f):
      center, name = parse_example(payload)
      centers.extend(center)
      name_index.append(names.setdefault(name, len(names)))
  decoded = [name.decode('utf-8') for name in names]
  return (np.array(centers, np.int64).reshape(-1, 3),
          [decoded[i] for i in name_index])
