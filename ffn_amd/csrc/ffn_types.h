// Plain types and constants that the host code and the device kernels of the MI355X
// (gfx950 / CDNA4) FFN field-of-view engine share.  No kernel and no device function
// lives here: every translation unit of the engine may include it (ffn_engine.h does).
//
// Written for gfx950 only: 64-wide wavefronts, v_mfma_f32_16x16x4_f32 (exact f32
// MFMA, bitwise an fmaf chain), 160 KiB LDS per CU, 256 CUs in 8 XCDs.
//
// Activation layout in HBM ("padded flat", channels last):
//   position p = z*plane + y*XS + x,  XS = fx+1, plane = (fy+1)*XS
//   one zero column (x = fx) and one zero row (y = fy) are shared between
//   neighbouring rows / planes, and a zero guard of plane+XS+1 positions sits
//   in front of and behind the FoV, so EVERY 3x3x3 tap of EVERY position is a
//   plain constant offset  dz*plane + dy*XS + dx  -- the SAME zero padding of
//   tf_slim.convolution3d (reference convstack_3d.py:28-31) without a single
//   bounds test in the inner loop.  Invalid (padding) positions are never
//   written, so they stay zero for the lifetime of the engine.
//   Each position holds 32 channels = 128 B = one cache line.
#pragma once

#include <stdint.h>

#include "../../include/ffn_hip.h"

namespace ffn {

constexpr int kFeatures = 32;
constexpr int kChunk = 160;          // output positions per workgroup
constexpr int kTile = 16;            // positions per MFMA M-tile
constexpr int kTilesPerWave = 5;     // 2 tile groups x 5 tiles = 10 tiles = kChunk
constexpr int kConvThreads = 256;    // 4 waves: (nhalf, tile group)

// Chunk sizes, LDS rows and LDS bytes of the conv kernel families: what the host's
// arithmetic on a FoV (ffn_stack_plan.h) shares with the kernels that use them.
// conv32c (ffn_conv_exact.h)
constexpr int kCChunk = 144;
constexpr int kCLdsStride = 40;      // LDS row stride in floats: 32 channels + 8 pad
// conv32d (ffn_conv_split.h), and its 96-voxel form (conv_variant 7)
constexpr int kDChunk = 160;
constexpr int kDThreads = 256;
constexpr int kDRowB = 144;          // epilogue: row stride of the partial sums in LDS
constexpr int kDTaps = 28;           // taps of a layer's packed weights: 27 + the all-zero tap
constexpr int kFlowStride = 64;      // FLOW hand-off: words between two producers' words
constexpr int kERows = 208, kETiles = 3, kEPieces = 7;
// conv32m
constexpr int kMChunk = 128;
constexpr int kMRows = 240;
constexpr int kMSeg = 8 * kMRows * 16;         // bytes of a segment slot
constexpr int kMRing = 2 * kMSeg;              // LDS offset of the weight ring
constexpr int kMRingTaps = 5;                  // taps resident in the weight ring
constexpr int kMLdsBytes = kMRing + kMRingTaps * 4096;  // 81,920: two per CU
// conv32mt's tail workgroups: rows per dz segment
constexpr int kTRows = 144;          // TNT = 1
constexpr int kT3Rows = 208;         // TNT = 3 (= conv_variant 7's kERows)
// conv32h / conv32hs (ffn_conv_half.h)
constexpr int kHChunk = 80;
constexpr int kHRows = 192;  // 80 voxels + 3 row ends + one plane end (XS) + 2 (XS + 1), XS <= 34
constexpr int kHSeg = 8 * kHRows * 16;            // bytes of a segment slot (24 DMA pieces)
constexpr int kHRingOff = 2 * kHSeg;
constexpr int kHUnit = 4 * 4096;                  // four taps of weight fragments
constexpr int kHLdsBytes = kHRingOff + 2 * kHUnit;  // 81,920: two per CU
constexpr int kHeadBlocks = 281;  // head kernel grid.x (4 sweeps of 32 voxels x 281)

struct Geom {
  int fz, fy, fx;      // FoV (zyx)
  int dz, dy, dx;      // deltas (zyx)
  int XS, plane;       // padded strides (positions)
  int npos;            // fz * plane
  int guard;           // plane + XS + 1
  int nchunks;         // ceil(npos / kChunk)
  int V;               // fz*fy*fx
  int R;               // LDS rows per dz segment = kChunk + 2*(XS+1)
  long act_stride;     // floats per FoV activation buffer
  // The split-product kernels may lay the FoV out with its axes permuted (the
  // shortest one as the row direction): axis a of THIS geometry is axis oa[a]
  // (0 z, 1 y, 2 x) of the caller's FoV / of the canvas, and one step along it
  // moves dstr[a] voxels in the caller's dense [z][y][x] order.  Identity:
  // oa = {0, 1, 2}, dstr = {fy fx, fx, 1}.
  int oa[3];
  int dstr[3];
  // A model that predicts a SMALLER mask than the seed it reads (ModelInfo
  // pred_mask_size < input_seed_size, reference model.py:168-183, inference.py:
  // 218,410-411): the canvas step scores, counts and pastes only the centred
  // box [c0, c1) of the FoV (caller's zyx); crop = 0: the whole FoV.
  int crop;
  int c0[3], c1[3];
  int Vp;              // voxels of the box (= V without a crop)
};

// Per-FoV step descriptor read by the gather / paste kernels.
struct StepItem {
  const float* image;        // f32 canvas image (already normalised), or NULL:
  const uint8_t* image_u8;   //   raw uint8 image ...
  const float* image_lut;    //   ... and its 256-entry normalisation table
  float* seed;
  const int32_t* seg;
  int cz, cy, cx;
  ffn_step_request req;
};

// positions a speculative conv0_a launch looks at (SpecArgs, ffn_conv0a.h)
constexpr int kSpecMax = 3;

// the segment turn (ffn_canvas_kernels.h): grid cap of its sweeps = partial sums per
// count, and the record its commit and pick kernels leave for the publish kernel
constexpr int kTurnBlocks = 512;
struct TurnRecord {
  unsigned long long counts[2];  // raw, actual (turn_count_kernel's partials, summed)
  int committed;                 // the id was assigned
  int chosen;                    // index of the next seed in the candidate list, -1 none
  int pad[2];
};

// the debug tracers of the split-product kernels (ffn_conv_split.h): workgroups that
// debug_clock 2 / 3 record, layers per workgroup slot of the debug_clock 4 trace
constexpr int kDbgMaxWgs = 4096;
constexpr int kFlowTraceLayers = 64;

}  // namespace ffn
