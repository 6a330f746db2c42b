// libffn_hip.so, gradients of the conv stack (include/ffn_gradients.h): the
// 3x3x3 conv with its two gradients, the 1x1x1 head with its gradient, and the
// weighted loss.  Everything is exact f32.
//
// The three 32-channel contractions run on v_mfma_f32_16x16x4_f32 over DENSE
// channels-last arrays; a workgroup stages its tile with the one-voxel halo in
// LDS, zero-filling whatever lies outside the FoV without reading it.
//   forward / backward to the input (conv32_kernel): M = 16 x-positions of a
//     row, N = 32 channels out (two accumulators), K = 27 taps x 32 channels
//     in.  A workgroup is 4 waves = 4 y-rows of one z-plane.  The backward
//     call is the same kernel on the weights read flipped in space and
//     transposed in channels, in place.
//   backward to the weights (conv32_dw_kernel): per tap M = 32 cin, N = 32
//     cout, K = positions.  A workgroup walks a slice of tiles (16 x by 2 y),
//     keeps all 27 taps of its quadrant (16 cin x 16 cout per wave) in
//     registers, and writes one partial [27][32][32] + [32];
//     reduce_partials_kernel adds the partials in slice order.  A slice never
//     crosses a batch item and its size depends on (z, y, x) only, so an
//     item's terms are summed in the same order whatever the batch holds.
// conv0_a (two input planes, 54 products per output) and the head are plain
// fmaf kernels; their sums over positions use the same partial + reduce form.
// The loss uses ffn_evaluation's finish tree: per-thread sums in index order,
// a shuffle tree per wave, an LDS tree per workgroup, one workgroup over the
// partials.

#include "../../include/ffn_gradients.h"

#include <hip/hip_runtime.h>

#include <algorithm>

#include "ffn_unit.h"

namespace {

using ffn_unit::DevBuf;
using ffn_unit::PinnedBuf;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kF = FFN_GRADIENTS_FEATURES;
constexpr int kTX = 16;        // x-positions of a tile = M (or K) of one MFMA
constexpr int kHX = kTX + 2;   // with the halo

struct Geo {
  int n, Z, Y, X;
  int tx, ty;  // tiles per row, tile rows per plane
};

// (n, z, y0, x0) of tile t; rows = y-rows of a tile.
__device__ __forceinline__ void tile_origin(const Geo& g, int t, int rows,
                                            int& n, int& z, int& y0, int& x0) {
  const int txi = t % g.tx;
  t /= g.tx;
  const int tyi = t % g.ty;
  t /= g.ty;
  z = t % g.Z;
  n = t / g.Z;
  y0 = tyi * rows;
  x0 = txi * kTX;
}

// Stages 3 z-planes x HY rows x kHX voxels x 32 channels around (z, y0, x0)
// into `lds` (row stride STRIDE floats); zero outside the FoV.
template <int HY, int STRIDE>
__device__ __forceinline__ void stage_halo(const Geo& g, const float* item,
                                           int z, int y0, int x0, bool relu,
                                           float* lds) {
  constexpr int kRows = 3 * HY * kHX;
  for (int e = threadIdx.x; e < kRows * 8; e += kThreads) {
    const int row = e >> 3, q = e & 7;
    const int dz = row / (HY * kHX);
    const int rem = row - dz * (HY * kHX);
    const int hy = rem / kHX, hx = rem - hy * kHX;
    const int zz = z + dz - 1, yy = y0 + hy - 1, xx = x0 + hx - 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)zz < (unsigned)g.Z && (unsigned)yy < (unsigned)g.Y &&
        (unsigned)xx < (unsigned)g.X) {
      v = *reinterpret_cast<const f32x4*>(
          item + (((size_t)zz * g.Y + yy) * g.X + xx) * kF + q * 4);
      if (relu) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaxf(v[c], 0.f);
      }
    }
    *reinterpret_cast<f32x4*>(lds + row * STRIDE + q * 4) = v;
  }
}

// ---------------------------------------------------------------------------
// conv32: forward, and backward to the input (TRANSPOSED).
// ---------------------------------------------------------------------------
constexpr int kCTY = 4, kCHY = kCTY + 2;
// 160-byte rows: the ds_read_b128 of 16 consecutive rows is bank-conflict free
// (ffn_conv_exact.h, kCLdsStride)
constexpr int kCStride = 40;

struct Conv32Args {
  const float* in;
  const float* w;     // [27][32][32]
  const float* bias;  // may be NULL
  const float* mask;  // may be NULL: result * (mask > 0)
  const float* add;   // may be NULL, may alias out
  float* out;
  Geo g;
  int relu_in;
};

template <bool TRANSPOSED>
__global__ __launch_bounds__(kThreads) void conv32_kernel(Conv32Args a) {
  __shared__ __attribute__((aligned(16))) float lds[3 * kCHY * kHX * kCStride];
  const Geo g = a.g;
  int n, z, y0, x0;
  tile_origin(g, blockIdx.x, kCTY, n, z, y0, x0);
  const size_t item = (size_t)n * g.Z * g.Y * g.X * kF;
  stage_halo<kCHY, kCStride>(g, a.in + item, z, y0, x0, a.relu_in != 0, lds);
  __syncthreads();

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int i = lane & 15, grp = lane >> 4;
  // [half of N][half of K]: four independent chains cover the MFMA's
  // dependent latency and shorten each fmaf chain to 27 x 16 terms
  f32x4 acc[2][2];
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k >> 1][k & 1] = f32x4{0.f, 0.f, 0.f, 0.f};

  // K order inside a tap: k-step s of half h is channel 16 h + 4 grp + s, so
  // one b128 read of the lane's row yields the A operand of 4 k-steps.
#pragma unroll 1
  for (int kzy = 0; kzy < 9; ++kzy) {
    const int kz = kzy / 3, ky = kzy - kz * 3;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int tap = kzy * 3 + kx;
      const int row = (kz * kCHY + wave + ky) * kHX + i + kx;
      const float* ap = lds + row * kCStride + grp * 4;
      f32x4 av[2];
      av[0] = *reinterpret_cast<const f32x4*>(ap);
      av[1] = *reinterpret_cast<const f32x4*>(ap + 16);
      f32x4 bv[2][2];  // [half of N][half of K]
      if (TRANSPOSED) {
        const float* wp = a.w + (26 - tap) * (kF * kF);
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            bv[nh][h] = *reinterpret_cast<const f32x4*>(
                wp + (16 * nh + i) * kF + 16 * h + 4 * grp);
      } else {
        const float* wp = a.w + tap * (kF * kF);
#pragma unroll
        for (int nh = 0; nh < 2; ++nh)
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < 4; ++s)
              bv[nh][h][s] = wp[(16 * h + 4 * grp + s) * kF + 16 * nh + i];
      }
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int nh = 0; nh < 2; ++nh)
            acc[nh][h] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                av[h][s], bv[nh][h][s], acc[nh][h], 0, 0, 0);
    }
  }

  // D[row = 4 grp + r][col = i] -> out[x0 + 4 grp + r][16 nh + i]
  const int y = y0 + wave;
  if (y >= g.Y) return;
#pragma unroll
  for (int nh = 0; nh < 2; ++nh) {
    const int co = 16 * nh + i;
    const float b = a.bias ? a.bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = x0 + 4 * grp + r;
      if (x >= g.X) continue;
      const size_t o = item + (((size_t)z * g.Y + y) * g.X + x) * kF + co;
      float v = (acc[nh][0][r] + acc[nh][1][r]) + b;
      if (a.mask) v = a.mask[o] > 0.f ? v : 0.f;
      if (a.add) v += a.add[o];
      a.out[o] = v;
    }
  }
}

// ---------------------------------------------------------------------------
// conv32 backward to the weights.
// ---------------------------------------------------------------------------
constexpr int kWTY = 2, kWHY = kWTY + 2;
// 192-byte rows: a ds_read_b32 of 16 channels x 4 consecutive rows touches 64
// distinct banks (row offsets 0, 48, 32, 16 mod 64)
constexpr int kWStride = 48;
constexpr int kWTile = kWTY * kTX;  // 32 positions = 8 k-steps
constexpr int kDwCount = 27 * kF * kF + kF;

struct DwArgs {
  const float* x;
  const float* dy;
  float* part;  // [nslices][kDwCount]
  Geo g;        // ty counts tiles of kWTY rows
  int relu_in;
  int item_tiles, tiles_per_slice, slices_per_item;
};

__global__ __launch_bounds__(kThreads) void conv32_dw_kernel(DwArgs a) {
  __shared__ __attribute__((aligned(16))) float lx[3 * kWHY * kHX * kWStride];
  __shared__ __attribute__((aligned(16))) float ldy[kWTile * kWStride];
  const Geo g = a.g;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int cih = wave & 1, coh = wave >> 1;
  const int i = lane & 15, grp = lane >> 4;

  f32x4 acc[27];
#pragma unroll
  for (int t = 0; t < 27; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;

  const int n = blockIdx.x / a.slices_per_item;
  const int t0 = (blockIdx.x - n * a.slices_per_item) * a.tiles_per_slice;
  const int t1 = min(t0 + a.tiles_per_slice, a.item_tiles);
  const size_t item = (size_t)n * g.Z * g.Y * g.X * kF;
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    int n0, z, y0, x0;  // n0 = 0: t counts the tiles of one item
    tile_origin(g, t, kWTY, n0, z, y0, x0);
    __syncthreads();  // the previous tile's reads are done
    stage_halo<kWHY, kWStride>(g, a.x + item, z, y0, x0, a.relu_in != 0, lx);
    {  // dy tile: 32 positions x 8 quads = one 16-byte load per thread
      const int r = tid >> 3, q = tid & 7;
      const int yy = y0 + (r >> 4), xx = x0 + (r & 15);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (yy < g.Y && xx < g.X)
        v = *reinterpret_cast<const f32x4*>(
            a.dy + item + (((size_t)z * g.Y + yy) * g.X + xx) * kF + q * 4);
      *reinterpret_cast<f32x4*>(ldy + r * kWStride + q * 4) = v;
    }
    __syncthreads();
    if (tid < kF) {
      float s = 0.f;
      for (int r = 0; r < kWTile; ++r) s += ldy[r * kWStride + tid];
      dbacc += s;
    }
    // A[m = cin][k = position], B[k = position][n = cout]
#pragma unroll 1
    for (int ks = 0; ks < kWTile / 4; ++ks) {
      const int yr = ks >> 2, xk = (ks & 3) * 4 + grp;
      const float b = ldy[(yr * kTX + xk) * kWStride + 16 * coh + i];
      const float* xp = lx + (yr * kHX + xk) * kWStride + 16 * cih + i;
#pragma unroll
      for (int tap = 0; tap < 27; ++tap) {
        const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
        const float av = xp[((kz * kWHY + ky) * kHX + kx) * kWStride];
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b, acc[tap], 0, 0, 0);
      }
    }
  }

  // D[row = 4 grp + r][col = i] -> dW[tap][16 cih + 4 grp + r][16 coh + i]
  float* dst = a.part + (size_t)blockIdx.x * kDwCount;
#pragma unroll
  for (int tap = 0; tap < 27; ++tap)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      dst[tap * (kF * kF) + (16 * cih + 4 * grp + r) * kF + 16 * coh + i] =
          acc[tap][r];
  if (tid < kF) dst[27 * kF * kF + tid] = dbacc;
}

// out[j] = sum over slices, in slice order; entries >= split go to out_b.
__global__ __launch_bounds__(kThreads) void reduce_partials_kernel(
    const float* __restrict__ part, int nslices, int count, int split,
    float* __restrict__ out_a, float* __restrict__ out_b) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= count) return;
  float s = 0.f;
  for (int k = 0; k < nslices; ++k) s += part[(size_t)k * count + j];
  if (j < split)
    out_a[j] = s;
  else
    out_b[j - split] = s;
}

// ---------------------------------------------------------------------------
// conv0_a: two input planes.
// ---------------------------------------------------------------------------
constexpr int kW2 = 27 * 2 * kF;       // 1728 weights
constexpr int kDw2Count = kW2 + kF;
constexpr int kDw2Slice = 128;         // positions per workgroup

struct Conv2Args {
  const float* img;
  const float* seed;
  const float* w;
  const float* bias;
  const float* skip;  // may be NULL
  float* out;
  int Z, Y, X, P;     // P = n z y x
  int relu_in;
};

__global__ __launch_bounds__(kThreads) void conv2_forward_kernel(Conv2Args a) {
  __shared__ float sw[kW2];
  for (int e = threadIdx.x; e < kW2; e += kThreads) sw[e] = a.w[e];
  __syncthreads();
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  const int p = idx >> 5, co = idx & 31;
  if (p >= a.P) return;
  const int x = p % a.X;
  int r = p / a.X;
  const int y = r % a.Y;
  r /= a.Y;
  const int z = r % a.Z;
  float acc = 0.f;
#pragma unroll
  for (int tap = 0; tap < 27; ++tap) {
    const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
    const int zz = z + kz - 1, yy = y + ky - 1, xx = x + kx - 1;
    if ((unsigned)zz < (unsigned)a.Z && (unsigned)yy < (unsigned)a.Y &&
        (unsigned)xx < (unsigned)a.X) {
      const int q = p + ((kz - 1) * a.Y + (ky - 1)) * a.X + (kx - 1);
      float v0 = a.img[q], v1 = a.seed[q];
      if (a.relu_in) {
        v0 = fmaxf(v0, 0.f);
        v1 = fmaxf(v1, 0.f);
      }
      acc = fmaf(v0, sw[(tap * 2) * kF + co], acc);
      acc = fmaf(v1, sw[(tap * 2 + 1) * kF + co], acc);
    }
  }
  float v = acc + a.bias[co];
  const size_t o = (size_t)p * kF + co;
  if (a.skip) v += a.skip[o];
  a.out[o] = v;
}

// Thread (co = tid & 31, group = tid >> 5) owns the (tap, plane) pairs k =
// group + 8 j of channel co and walks the slice's positions in order.
__global__ __launch_bounds__(kThreads) void conv2_dw_kernel(
    const float* __restrict__ img, const float* __restrict__ seed,
    const float* __restrict__ dy, int relu_in, int Z, int Y, int X,
    int slices_per_item, float* __restrict__ part) {
  const int co = threadIdx.x & 31, group = threadIdx.x >> 5;
  float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float dbs = 0.f;
  const int item = blockIdx.x / slices_per_item;
  const int first = (blockIdx.x - item * slices_per_item) * kDw2Slice;
  const int voxels = Z * Y * X;
  const int p0 = item * voxels + first;
  const int p1 = item * voxels + min(first + kDw2Slice, voxels);
  for (int p = p0; p < p1; ++p) {
    const int x = p % X;
    int r = p / X;
    const int y = r % Y;
    r /= Y;
    const int z = r % Z;
    const float dyv = dy[(size_t)p * kF + co];
    dbs += dyv;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const int k = group + 8 * j;
      if (k >= 54) continue;
      const int tap = k >> 1;
      const int kz = tap / 9, ky = (tap / 3) % 3, kx = tap % 3;
      const int zz = z + kz - 1, yy = y + ky - 1, xx = x + kx - 1;
      if ((unsigned)zz < (unsigned)Z && (unsigned)yy < (unsigned)Y &&
          (unsigned)xx < (unsigned)X) {
        const int q = p + ((kz - 1) * Y + (ky - 1)) * X + (kx - 1);
        float v = (k & 1) ? seed[q] : img[q];
        if (relu_in) v = fmaxf(v, 0.f);
        acc[j] = fmaf(v, dyv, acc[j]);
      }
    }
  }
  float* dst = part + (size_t)blockIdx.x * kDw2Count;
#pragma unroll
  for (int j = 0; j < 7; ++j) {
    const int k = group + 8 * j;
    if (k < 54) dst[k * kF + co] = acc[j];
  }
  if (group == 0) dst[kW2 + co] = dbs;
}

// ---------------------------------------------------------------------------
// head: 1x1x1 conv 32 -> 1 on max(net, 0), logits = seed + update.
// ---------------------------------------------------------------------------
constexpr int kHeadSlice = 256;  // positions per workgroup of head_backward
constexpr int kHeadCount = kF + 1;

// 8 lanes per position, one 16-byte quad each.
__global__ __launch_bounds__(kThreads) void head_forward_kernel(
    const float* __restrict__ net, const float* __restrict__ seed,
    const float* __restrict__ w, const float* __restrict__ b, int P,
    float* __restrict__ logits) {
  const int idx = blockIdx.x * kThreads + threadIdx.x;
  const int p = idx >> 3, q = idx & 7;
  float partial = 0.f;
  if (p < P) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(net + (size_t)p * kF + q * 4);
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + q * 4);
    partial = fmaxf(v[0], 0.f) * w4[0];
    partial = fmaf(fmaxf(v[1], 0.f), w4[1], partial);
    partial = fmaf(fmaxf(v[2], 0.f), w4[2], partial);
    partial = fmaf(fmaxf(v[3], 0.f), w4[3], partial);
  }
  partial += __shfl_xor(partial, 1);
  partial += __shfl_xor(partial, 2);
  partial += __shfl_xor(partial, 4);
  if (p < P && q == 0) logits[p] = seed[p] + (partial + b[0]);
}

__global__ __launch_bounds__(kThreads) void head_backward_kernel(
    const float* __restrict__ net, const float* __restrict__ dlogits,
    const float* __restrict__ w, int voxels, int slices_per_item,
    float* __restrict__ dnet, float* __restrict__ part) {
  __shared__ float s[kThreads / kF][kF];
  const int tid = threadIdx.x;
  const int item = blockIdx.x / slices_per_item;
  const int first = (blockIdx.x - item * slices_per_item) * kHeadSlice;
  const int p0 = item * voxels + first;
  const int p1 = item * voxels + min(first + kHeadSlice, voxels);
  {
    const int q = tid & 7;
    const f32x4 w4 = *reinterpret_cast<const f32x4*>(w + q * 4);
    for (int p = p0 + (tid >> 3); p < p1; p += kThreads / 8) {
      const f32x4 v =
          *reinterpret_cast<const f32x4*>(net + (size_t)p * kF + q * 4);
      const float d = dlogits[p];
      f32x4 o;
#pragma unroll
      for (int c = 0; c < 4; ++c) o[c] = v[c] > 0.f ? d * w4[c] : 0.f;
      *reinterpret_cast<f32x4*>(dnet + (size_t)p * kF + q * 4) = o;
    }
  }
  const int c = tid & 31, r = tid >> 5;
  float acc = 0.f;
  for (int p = p0 + r; p < p1; p += kThreads / kF)
    acc = fmaf(dlogits[p], fmaxf(net[(size_t)p * kF + c], 0.f), acc);
  s[r][c] = acc;
  __syncthreads();
  float* dst = part + (size_t)blockIdx.x * kHeadCount;
  if (tid < kF) {
    float t = 0.f;
    for (int k = 0; k < kThreads / kF; ++k) t += s[k][tid];
    dst[tid] = t;
  } else if (tid == kF) {
    float t = 0.f;
    for (int p = p0; p < p1; ++p) t += dlogits[p];
    dst[kF] = t;
  }
}

// ---------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------
constexpr int kLossBlocks = kThreads;  // at most; loss_sum_kernel is one workgroup

__device__ __forceinline__ float block_tree(float v, float* s_v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
  __syncthreads();
  // kWaves = 4: ((0 + 1) + (2 + 3))
  return (s_v[0] + s_v[1]) + (s_v[2] + s_v[3]);
}

__global__ __launch_bounds__(kThreads) void loss_kernel(
    const float* __restrict__ logits, const float* __restrict__ labels,
    const float* __restrict__ weights, int N, float* __restrict__ dlogits,
    float* __restrict__ partials) {
  __shared__ float s_v[kWaves];
  const float fn = (float)N;
  float loss = 0.f;
  for (int i = blockIdx.x * kThreads + threadIdx.x; i < N;
       i += gridDim.x * kThreads) {
    const float x = logits[i], z = labels[i], w = weights[i];
    const float e = expf(-fabsf(x));
    loss += w * (fmaxf(x, 0.f) - x * z + log1pf(e));
    if (dlogits) {
      const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
      dlogits[i] = w * (sig - z) / fn;
    }
  }
  loss = block_tree(loss, s_v);
  if (threadIdx.x == 0) partials[blockIdx.x] = loss;
}

__global__ __launch_bounds__(kThreads) void loss_sum_kernel(
    const float* __restrict__ partials, int nblocks, float* __restrict__ out) {
  __shared__ float s_v[kWaves];
  float v = (int)threadIdx.x < nblocks ? partials[threadIdx.x] : 0.f;
  v = block_tree(v, s_v);
  if (threadIdx.x == 0) out[0] = v;
}

}  // namespace

struct ffn_gradients : ffn_unit::Unit {
  DevBuf part;      // partial sums of the weight-gradient kernels
  DevBuf loss_dev;  // kLossBlocks partials + the sum
  PinnedBuf stage;
  double ms[6] = {0, 0, 0, 0, 0, 0};
};

namespace {

// n, shape -> Geo and the position count; FFN_ERR_ARG otherwise.
int check_geometry(const ffn_gradients* h, int n, const int32_t shape_zyx[3],
                   Geo* g, int* P) {
  if (!h) return ffn_set_error(FFN_ERR_ARG, "handle is NULL");
  if (!shape_zyx) return ffn_set_error(FFN_ERR_ARG, "shape_zyx is NULL");
  if (n < 1 || n > FFN_GRADIENTS_MAX_BATCH)
    return ffn_set_error(FFN_ERR_ARG, "n = %d, expected 1 .. %d", n,
                         FFN_GRADIENTS_MAX_BATCH);
  long long total = n;
  for (int k = 0; k < 3; ++k) {
    if (shape_zyx[k] < 1)
      return ffn_set_error(FFN_ERR_ARG, "shape_zyx[%d] = %d < 1", k,
                           shape_zyx[k]);
    total *= shape_zyx[k];
    if (total >= (1ll << 26))
      return ffn_set_error(FFN_ERR_ARG, "n z y x must stay below 2^26");
  }
  g->n = n;
  g->Z = shape_zyx[0];
  g->Y = shape_zyx[1];
  g->X = shape_zyx[2];
  g->tx = (g->X + kTX - 1) / kTX;
  g->ty = 0;
  *P = (int)total;
  return FFN_OK;
}

int check_cin(int cin) {
  if (cin != 2 && cin != kF)
    return ffn_set_error(FFN_ERR_ARG, "cin = %d, expected 2 or %d", cin, kF);
  return FFN_OK;
}

#define G_PTR(p)                                                  \
  do {                                                            \
    if (!(p)) return ffn_set_error(FFN_ERR_ARG, #p " is NULL");   \
  } while (0)

bool overlap(const float* a, const float* b, size_t count) {
  return a < b + count && b < a + count;
}

int select_device(ffn_gradients* h) {
  U_TRY(hipSetDevice(h->device_id));
  return FFN_OK;
}

int begin(ffn_gradients* h) {
  U_OK(select_device(h));
  return h->timer_start();
}

int end(ffn_gradients* h, int which) {
  U_TRY(hipGetLastError());
  return h->timer_stop(&h->ms[which]);
}

int launch_reduce(ffn_gradients* h, int nslices, int count, int split,
                  float* out_a, float* out_b) {
  hipLaunchKernelGGL(reduce_partials_kernel,
                     dim3((count + kThreads - 1) / kThreads), dim3(kThreads), 0,
                     h->stream, static_cast<const float*>(h->part.p), nslices,
                     count, split, out_a, out_b);
  return FFN_OK;
}

int launch_conv32(ffn_gradients* h, bool transposed, Conv32Args a) {
  a.g.ty = (a.g.Y + kCTY - 1) / kCTY;
  const unsigned tiles = (unsigned)a.g.n * a.g.Z * a.g.ty * a.g.tx;
  if (transposed)
    hipLaunchKernelGGL(conv32_kernel<true>, dim3(tiles), dim3(kThreads), 0,
                       h->stream, a);
  else
    hipLaunchKernelGGL(conv32_kernel<false>, dim3(tiles), dim3(kThreads), 0,
                       h->stream, a);
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_gradients_create(int device_id, ffn_gradients** out) {
  U_OK(ffn_unit::unit_create(device_id, out));
  ffn_gradients* h = *out;
  int rc = ffn_unit::ensure(h->loss_dev, (kLossBlocks + 1) * sizeof(float));
  if (rc == FFN_OK) rc = ffn_unit::ensure(h->stage, sizeof(float));
  if (rc != FFN_OK) {
    ffn_unit::unit_destroy(h);
    *out = nullptr;
  }
  return rc;
}

void ffn_gradients_destroy(ffn_gradients* h) { ffn_unit::unit_destroy(h); }

int ffn_gradients_conv_forward(ffn_gradients* h, int n,
                               const int32_t shape_zyx[3], int cin,
                               const float* x_dev, const float* x2_dev,
                               int relu_in, const float* w_dev,
                               const float* b_dev, const float* skip_dev,
                               float* y_dev) {
  Geo g;
  int P;
  U_OK(check_geometry(h, n, shape_zyx, &g, &P));
  U_OK(check_cin(cin));
  G_PTR(x_dev);
  G_PTR(w_dev);
  G_PTR(b_dev);
  G_PTR(y_dev);
  if (cin == 2) G_PTR(x2_dev);
  if (cin == kF && overlap(x_dev, y_dev, (size_t)P * kF))
    return ffn_set_error(FFN_ERR_ARG, "y_dev overlaps x_dev");
  U_OK(begin(h));
  if (cin == kF) {
    Conv32Args a = {x_dev, w_dev, b_dev, nullptr, skip_dev, y_dev, g,
                    relu_in != 0};
    U_OK(launch_conv32(h, false, a));
  } else {
    Conv2Args a = {x_dev, x2_dev, w_dev, b_dev, skip_dev, y_dev,
                   g.Z,   g.Y,    g.X,   P,     relu_in != 0};
    const unsigned blocks = (unsigned)(((size_t)P * kF + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(conv2_forward_kernel, dim3(blocks), dim3(kThreads), 0,
                       h->stream, a);
  }
  return end(h, 0);
}

int ffn_gradients_conv_backward_input(ffn_gradients* h, int n,
                                      const int32_t shape_zyx[3],
                                      const float* dy_dev, const float* w_dev,
                                      const float* pre_dev, int accumulate,
                                      float* dx_dev) {
  Geo g;
  int P;
  U_OK(check_geometry(h, n, shape_zyx, &g, &P));
  G_PTR(dy_dev);
  G_PTR(w_dev);
  G_PTR(dx_dev);
  if (overlap(dy_dev, dx_dev, (size_t)P * kF))
    return ffn_set_error(FFN_ERR_ARG, "dx_dev overlaps dy_dev");
  U_OK(begin(h));
  Conv32Args a = {dy_dev, w_dev, nullptr, pre_dev,
                  accumulate ? dx_dev : nullptr, dx_dev, g, 0};
  U_OK(launch_conv32(h, true, a));
  return end(h, 1);
}

int ffn_gradients_conv_backward_weights(ffn_gradients* h, int n,
                                        const int32_t shape_zyx[3], int cin,
                                        const float* x_dev, const float* x2_dev,
                                        int relu_in, const float* dy_dev,
                                        float* dw_dev, float* db_dev) {
  Geo g;
  int P;
  U_OK(check_geometry(h, n, shape_zyx, &g, &P));
  U_OK(check_cin(cin));
  G_PTR(x_dev);
  G_PTR(dy_dev);
  G_PTR(dw_dev);
  G_PTR(db_dev);
  if (cin == 2) G_PTR(x2_dev);
  U_OK(select_device(h));
  if (cin == kF) {
    g.ty = (g.Y + kWTY - 1) / kWTY;
    const int item_tiles = g.Z * g.ty * g.tx;
    // a function of (z, y, x) only: at least 4 tiles, at most 128 slices an item
    const int per = std::max(4, (item_tiles + 127) / 128);
    const int per_item = (item_tiles + per - 1) / per;
    const int nslices = g.n * per_item;
    U_OK(ffn_unit::ensure(h->part, (size_t)nslices * kDwCount * sizeof(float)));
    U_OK(begin(h));
    DwArgs a = {x_dev, dy_dev, static_cast<float*>(h->part.p), g, relu_in != 0,
                item_tiles, per, per_item};
    hipLaunchKernelGGL(conv32_dw_kernel, dim3(nslices), dim3(kThreads), 0,
                       h->stream, a);
    U_OK(launch_reduce(h, nslices, kDwCount, 27 * kF * kF, dw_dev, db_dev));
  } else {
    const int per_item = (P / g.n + kDw2Slice - 1) / kDw2Slice;
    const int nslices = g.n * per_item;
    U_OK(ffn_unit::ensure(h->part, (size_t)nslices * kDw2Count * sizeof(float)));
    U_OK(begin(h));
    hipLaunchKernelGGL(conv2_dw_kernel, dim3(nslices), dim3(kThreads), 0,
                       h->stream, x_dev, x2_dev, dy_dev, (int)(relu_in != 0),
                       g.Z, g.Y, g.X, per_item, static_cast<float*>(h->part.p));
    U_OK(launch_reduce(h, nslices, kDw2Count, kW2, dw_dev, db_dev));
  }
  return end(h, 2);
}

int ffn_gradients_head_forward(ffn_gradients* h, int n,
                               const int32_t shape_zyx[3], const float* net_dev,
                               const float* seed_dev, const float* w_dev,
                               const float* b_dev, float* logits_dev) {
  Geo g;
  int P;
  U_OK(check_geometry(h, n, shape_zyx, &g, &P));
  G_PTR(net_dev);
  G_PTR(seed_dev);
  G_PTR(w_dev);
  G_PTR(b_dev);
  G_PTR(logits_dev);
  U_OK(begin(h));
  const unsigned blocks = (unsigned)(((size_t)P * 8 + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(head_forward_kernel, dim3(blocks), dim3(kThreads), 0,
                     h->stream, net_dev, seed_dev, w_dev, b_dev, P, logits_dev);
  return end(h, 3);
}

int ffn_gradients_head_backward(ffn_gradients* h, int n,
                                const int32_t shape_zyx[3],
                                const float* net_dev, const float* dlogits_dev,
                                const float* w_dev, float* dnet_dev,
                                float* dw_dev, float* db_dev) {
  Geo g;
  int P;
  U_OK(check_geometry(h, n, shape_zyx, &g, &P));
  G_PTR(net_dev);
  G_PTR(dlogits_dev);
  G_PTR(w_dev);
  G_PTR(dnet_dev);
  G_PTR(dw_dev);
  G_PTR(db_dev);
  if (overlap(net_dev, dnet_dev, (size_t)P * kF))
    return ffn_set_error(FFN_ERR_ARG, "dnet_dev overlaps net_dev");
  U_OK(select_device(h));
  const int per_item = (P / g.n + kHeadSlice - 1) / kHeadSlice;
  const int nslices = g.n * per_item;
  U_OK(ffn_unit::ensure(h->part, (size_t)nslices * kHeadCount * sizeof(float)));
  U_OK(begin(h));
  hipLaunchKernelGGL(head_backward_kernel, dim3(nslices), dim3(kThreads), 0,
                     h->stream, net_dev, dlogits_dev, w_dev, P / g.n, per_item,
                     dnet_dev, static_cast<float*>(h->part.p));
  U_OK(launch_reduce(h, nslices, kHeadCount, kF, dw_dev, db_dev));
  return end(h, 4);
}

int ffn_gradients_loss(ffn_gradients* h, int n, const int32_t shape_zyx[3],
                       const float* logits_dev, const float* labels_dev,
                       const float* weights_dev, float* loss,
                       float* dlogits_dev) {
  Geo g;
  int P;
  U_OK(check_geometry(h, n, shape_zyx, &g, &P));
  G_PTR(logits_dev);
  G_PTR(labels_dev);
  G_PTR(weights_dev);
  G_PTR(loss);
  U_OK(begin(h));
  float* partials = static_cast<float*>(h->loss_dev.p);
  const int blocks = std::min(kLossBlocks, (P + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(loss_kernel, dim3(blocks), dim3(kThreads), 0, h->stream,
                     logits_dev, labels_dev, weights_dev, P, dlogits_dev,
                     partials);
  hipLaunchKernelGGL(loss_sum_kernel, dim3(1), dim3(kThreads), 0, h->stream,
                     static_cast<const float*>(partials), blocks,
                     partials + kLossBlocks);
  U_OK(end(h, 5));
  U_TRY(hipMemcpyAsync(h->stage.p, partials + kLossBlocks, sizeof(float),
                       hipMemcpyDeviceToHost, h->stream));
  U_TRY(hipStreamSynchronize(h->stream));
  *loss = (float)((double)*static_cast<const float*>(h->stage.p) / (double)P);
  return FFN_OK;
}

int ffn_gradients_last_timing(ffn_gradients* h, double kernel_ms[6]) {
  if (!h || !kernel_ms)
    return ffn_set_error(FFN_ERR_ARG, "NULL argument");
  for (int k = 0; k < 6; ++k) kernel_ms[k] = h->ms[k];
  return FFN_OK;
}

}  // extern "C"
