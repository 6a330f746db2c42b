"""TEST INFRASTRUCTURE: the restrictor's two bits per voxel (include/ffn_hip.h,
ffn_canvas_set_restrictor) restated in numpy, independently of the device's
separable OR passes: the shift-mask box is counted with a summed-area table.
Plus the packing of a bit plane as the library's loop reads it, and an emulated
canvas (over tests/host_loop_restrict_shim.cpp) that carries a restrictor."""
import ctypes

import numpy as np

from tests.native_shim import ShimClient, ShimHandle


def _axis_ranges(n_canvas, n_shift, pre, post, scale):
  """Per canvas coordinate: [lo, hi1) of shift-mask indices, clipped (lo = hi1
  for an empty range)."""
  i = np.arange(n_canvas, dtype=np.int64)
  lo = np.maximum(i + pre, 0) // scale
  hi = np.minimum((i + post) // scale, n_shift - 1)
  lo_c = np.clip(lo, 0, n_shift)
  hi1 = np.clip(hi + 1, 0, n_shift)
  hi1 = np.maximum(hi1, lo_c)
  return lo_c, hi1


def shift_blocked(shape, shift, pre, post, scale):
  """bool [shape]: any true voxel of the reduced shift mask in the box of each
  position (z unscaled, y and x floor-divided by `scale`)."""
  shift = np.asarray(shift) != 0
  zs, ys, xs = shift.shape
  sat = np.zeros((zs + 1, ys + 1, xs + 1), np.int64)
  sat[1:, 1:, 1:] = shift.cumsum(0).cumsum(1).cumsum(2)
  z0, z1 = _axis_ranges(shape[0], zs, pre[0], post[0], 1)
  y0, y1 = _axis_ranges(shape[1], ys, pre[1], post[1], scale)
  x0, x1 = _axis_ranges(shape[2], xs, pre[2], post[2], scale)
  out = np.empty(shape, bool)
  for z in range(shape[0]):  # (one z slab at a time: bounded memory)
    a, b = z0[z], z1[z]
    def s(zz):
      t = sat[zz]
      return (t[y1][:, x1] - t[y0][:, x1] - t[y1][:, x0] + t[y0][:, x0])
    out[z] = (s(b) - s(a)) > 0
  return out


def restriction(shape, mask=None, seed_mask=None, shift=None, pre=(0, 0, 0),
                post=(0, 0, 0), scale=1):
  """uint8 [shape]: bit 0 pos_blocked, bit 1 seed_blocked."""
  pos = np.zeros(shape, bool)
  if mask is not None:
    pos |= np.asarray(mask) != 0
  if shift is not None:
    pos |= shift_blocked(shape, shift, pre, post, scale)
  out = pos.astype(np.uint8)
  if seed_mask is not None:
    out |= (np.asarray(seed_mask) != 0).astype(np.uint8) << 1
  return out


def restrictor_args(r):
  """ffn_canvas_set_restrictor's arguments for a stock MovementRestrictor."""
  out = {'mask': r.mask, 'seed_mask': r.seed_mask, 'shift': r.shift_mask}
  if r.shift_mask is not None:
    out.update(pre=[int(v) for v in r._shift_mask_fov_pre_offset],
               post=[int(v) for v in r._shift_mask_fov_post_offset],
               scale=int(r._shift_mask_scale))
  return out


def pack_plane(plane):
  """bool [Z, Y, X] -> uint64 [Z, Y, ceil(X / 64)]: bit x % 64 of word x / 64."""
  z, y, x = plane.shape
  w = (x + 63) // 64
  padded = np.zeros((z, y, w * 64), bool)
  padded[..., :x] = plane
  return np.ascontiguousarray(
      np.packbits(padded, axis=-1, bitorder='little').view('<u8'))


class RestrictShimHandle(ShimHandle):
  """Emulated canvas whose library loop (the shim) and segment turn apply a
  restrictor, as the HIP canvas does after ffn_canvas_set_restrictor."""

  def __init__(self, image):
    super().__init__(image)
    self.bits = None
    self._plane = None
    self.flag4 = 0  # turn candidates flagged "restricted"

  def set_restrictor(self, mask=None, seed_mask=None, shift_mask=None,
                     pre=(0, 0, 0), post=(0, 0, 0), scale=1):
    if mask is None and seed_mask is None and shift_mask is None:
      self.bits = self._plane = None
      self.shim.shim_state_set_restriction(self._state, None, None, 0)
      return
    self.bits = restriction(self.shape, mask, seed_mask, shift_mask, pre, post,
                            scale)
    self._plane = pack_plane((self.bits & 1) != 0)
    dims = (ctypes.c_int32 * 3)(*self.shape)
    self.shim.shim_state_set_restriction(self._state, self._plane.ctypes.data,
                                         dims, self._plane.shape[-1])

  def read_restriction(self, lo=None, hi=None):
    lo = lo or (0, 0, 0)
    hi = hi or self.shape
    if self.bits is None:
      return np.zeros([h - l for l, h in zip(lo, hi)], np.uint8)
    return np.array(self.bits[tuple(slice(l, h) for l, h in zip(lo, hi))])

  def take_restricted_skips(self):
    return int(self.shim.shim_take_restricted_skips(self._state))

  def segment_turn(self, commit=None, mark=None, candidates=(), mbd=(0, 0, 0),
                   init_value=None):
    """EmulatedHandle.segment_turn with flag 4 (ffn_canvas_segment_turn): not
    segmented, but vetoed by the restrictor -- skipped, no marker."""
    if self.bits is None:
      return super().segment_turn(commit, mark, candidates, mbd, init_value)
    # commit and marker as the stock turn does them, then the candidates
    head = super().segment_turn(commit, mark, (), mbd, None)
    cand = np.asarray(candidates, np.int32).reshape(-1, 3)
    n = len(cand)
    flags = np.full(n, 3, np.int32)
    cseed = np.zeros(n, np.float32)
    cseg = np.zeros(n, np.int32)
    for k, p in enumerate(cand):  # (values: the canvas before any marker)
      cseed[k], cseg[k] = self.seed[tuple(p)], self.seg[tuple(p)]
    chosen = -1
    for k, p in enumerate(cand):
      p = tuple(int(v) for v in p)
      if self.seg[p] > 0:
        flags[k] = 1
        continue
      if self.bits[p]:
        flags[k] = 4
        self.flag4 += 1
        continue
      lo = [v - m for v, m in zip(p, mbd)]
      hi = [v + m + 1 for v, m in zip(p, mbd)]
      if self.any_segmented(lo, hi):
        flags[k] = 2
        self.seg[p] = -1
        continue
      flags[k] = 0
      chosen = k
      break
    if chosen >= 0 and init_value is not None:
      self.init_seed(tuple(int(v) for v in cand[chosen]), init_value)
    return tuple(head[:5]) + (chosen, flags, cseed, cseg)


class RestrictShimClient(ShimClient):

  def create_canvas(self, image):
    ShimHandle.client = self
    return RestrictShimHandle(image)
