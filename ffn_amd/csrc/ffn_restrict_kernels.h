// MovementRestrictor (reference movement.py:247-336) on the device: the two
// static tests of a restricted canvas built once, as bit planes, by
// ffn_canvas_set_restrictor (include/ffn_hip.h).
//
//   pos_blocked(z, y, x)  = mask[z, y, x] != 0, or any voxel of the reduced shift
//                           mask in the box below (MovementRestrictor.is_valid_pos)
//   seed_blocked(z, y, x) = seed_mask[z, y, x] != 0 (is_valid_seed)
//
// The shift box of a position: z rows max(z + pre_z, 0) .. min(z + post_z, Zs-1)
// (z indexes the shift mask directly), y columns floor(max(y + pre_y, 0) / s) ..
// min(floor((y + post_y) / s), Ys-1), x the same; an empty range on any axis
// means "not blocked".  Divisions are floor divisions (numpy's //).
//
// Layout: a plane holds one bit per voxel, 64 voxels of a row per 64-bit word
// along x (bit x % 64 of word x / 64), rows padded to whole words:
//   word index (z * Y + y) * W + x / 64,  W = ceil(X / 64).
// The pos plane comes first, the seed plane right behind it.  One word is one
// __ballot of a wave, written by lane 0 with a plain vector store.
//
// The shift box is separable: x first (per bit, from the u8 shift mask), then y
// and z as ORs of whole words.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace ffn {

__device__ inline int restrict_floordiv(int a, int b) {  // Python's //, b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// plane[(r * W) + w] bit l = src[r * X + w * 64 + l] != 0 (r: a row of the canvas);
// one wave per word
__global__ __launch_bounds__(256) void restrict_pack_kernel(
    const uint8_t* __restrict__ src, long rows, int X, int W,
    unsigned long long* __restrict__ plane) {
  const int lane = threadIdx.x & 63;
  const size_t nwords = (size_t)rows * W;
  const size_t stride = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t wi = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wi < nwords;
       wi += stride) {
    const size_t r = wi / W;
    const int x = (int)(wi - r * W) * 64 + lane;
    const bool hit = x < X && src[r * X + x] != 0;
    const unsigned long long m = __ballot(hit);
    if (lane == 0) plane[wi] = m;
  }
}

// x pass: ax[(zs * Ys + ys) * W + w] bit l = OR of shift[zs, ys, xs] over the
// x range of canvas column x = w * 64 + l
__global__ __launch_bounds__(256) void restrict_shift_x_kernel(
    const uint8_t* __restrict__ shift, long rows, int Xs, int X, int W, int pre,
    int post, int scale, unsigned long long* __restrict__ ax) {
  const int lane = threadIdx.x & 63;
  const size_t nwords = (size_t)rows * W;
  const size_t stride = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t wi = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; wi < nwords;
       wi += stride) {
    const size_t r = wi / W;
    const int x = (int)(wi - r * W) * 64 + lane;
    bool hit = false;
    if (x < X) {
      const int lo = restrict_floordiv(max(x + pre, 0), scale);
      const int hi = min(restrict_floordiv(x + post, scale), Xs - 1);
      const uint8_t* row = shift + r * Xs;
      for (int xs = lo; xs <= hi && !hit; ++xs) hit = row[xs] != 0;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) ax[wi] = m;
  }
}

// y pass: ay[(zs * Y + y) * W + w] = OR of ax[(zs * Ys + ys) * W + w] over the
// y range of canvas row y (floor-divided by the scale, as x)
__global__ __launch_bounds__(256) void restrict_shift_y_kernel(
    const unsigned long long* __restrict__ ax, int Zs, int Ys, int Y, int W, int pre,
    int post, int scale, unsigned long long* __restrict__ ay) {
  const size_t nwords = (size_t)Zs * Y * W;
  for (size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; wi < nwords;
       wi += (size_t)gridDim.x * blockDim.x) {
    const int w = (int)(wi % W);
    const size_t t = wi / W;
    const int y = (int)(t % Y);
    const size_t zs = t / Y;
    const int lo = restrict_floordiv(max(y + pre, 0), scale);
    const int hi = min(restrict_floordiv(y + post, scale), Ys - 1);
    unsigned long long acc = 0;
    for (int ys = lo; ys <= hi; ++ys) acc |= ax[(zs * Ys + ys) * W + w];
    ay[wi] = acc;
  }
}

// z pass, into the pos plane (which holds the mask bits already): z indexes the
// shift mask unscaled
__global__ __launch_bounds__(256) void restrict_shift_z_kernel(
    const unsigned long long* __restrict__ ay, int Zs, int Z, int Y, int W, int pre,
    int post, unsigned long long* __restrict__ pos_plane) {
  const size_t nwords = (size_t)Z * Y * W;
  const size_t slab = (size_t)Y * W;
  for (size_t wi = (size_t)blockIdx.x * blockDim.x + threadIdx.x; wi < nwords;
       wi += (size_t)gridDim.x * blockDim.x) {
    const int z = (int)(wi / slab);
    const size_t yw = wi - (size_t)z * slab;
    const int lo = max(z + pre, 0);
    const int hi = min(z + post, Zs - 1);
    unsigned long long acc = 0;
    for (int zs = lo; zs <= hi; ++zs) acc |= ay[(size_t)zs * slab + yw];
    if (acc) pos_plane[wi] |= acc;
  }
}

// ffn_canvas_read_restriction: out[e] = pos bit | seed bit << 1 over a box
__global__ __launch_bounds__(256) void restrict_read_kernel(
    const unsigned long long* __restrict__ planes, size_t plane_words, int Y, int W,
    int z0, int y0, int x0, int ny, int nx, long total, uint8_t* __restrict__ out) {
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long)gridDim.x * blockDim.x) {
    const int x = x0 + (int)(e % nx);
    const long t = e / nx;
    const int y = y0 + (int)(t % ny);
    const int z = z0 + (int)(t / ny);
    const size_t wi = ((size_t)z * Y + y) * W + (x >> 6);
    const int b = x & 63;
    out[e] = (uint8_t)(((planes[wi] >> b) & 1ull) |
                       (((planes[plane_words + wi] >> b) & 1ull) << 1));
  }
}

}  // namespace ffn
