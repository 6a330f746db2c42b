// libffn_hip.so -- everything a canvas does between two FoV steps (ffn_engine.h): its
// creation and destruction, init_seed, the MovementRestrictor planes, point and box
// reads and writes, the commit and the segment turn.  All of it runs on the engine's
// utility stream under UtilLock; no conv or step kernel is launched from here.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "ffn_engine.h"
#include "ffn_kernels.h"
#include "ffn_canvas_kernels.h"
#include "ffn_restrict_kernels.h"

namespace {
// host-side: nothing queued on canvas c is still running
hipError_t canvas_quiesce(ffn_engine* e, ffn_canvas* c) {
  drop_spec(e);  // the caller is about to read or change the canvas directly
  hipError_t err = hipSuccess;
  if (c->paste_after_flag) {
    err = hipStreamSynchronize(e->stream);
    if (err == hipSuccess) c->paste_after_flag = false;
  }
  if (err == hipSuccess && c->util_pending) {
    err = hipEventSynchronize(c->ev_util);
    if (err == hipSuccess) c->util_pending = false;
  }
  return err;
}
}  // namespace

int ffn_canvas_view(ffn_canvas* c, FfnCanvasView* out) {
  if (!c || !out) return ffn_set_error(FFN_ERR_ARG, "NULL canvas");
  if (!c->engine)
    return ffn_set_error(FFN_ERR_STATE, "canvas outlived its engine");
  {
    // the caller (label / seed kernels on their own streams) reads the canvas
    // once the engine's stream is idle: the utility stream has to be, too
    EngineLock lock_(c->engine);
    if (canvas_quiesce(c->engine, c) != hipSuccess)
      return ffn_set_error(FFN_ERR_HIP, "canvas_quiesce failed");
  }
  out->device_id = c->engine->device;
  out->engine_stream = c->engine->stream;
  out->image = c->image;
  out->image_u8 = c->image_u8;
  out->image_lut = c->image_lut;
  out->segmentation = c->seg;
  out->shape_zyx[0] = c->cz;
  out->shape_zyx[1] = c->cy;
  out->shape_zyx[2] = c->cx;
  return FFN_OK;
}

int ensure_scratch(ffn_engine* e, size_t bytes) {
  if (bytes <= e->scratch_bytes) return FFN_OK;
  HIP_TRY(hipStreamSynchronize(e->ustream));  // (only utility calls use it)
  if (e->d_scratch) HIP_TRY(hipFree(e->d_scratch));
  if (e->h_scratch) HIP_TRY(hipHostFree(e->h_scratch));
  e->d_scratch = e->h_scratch = nullptr;
  e->scratch_bytes = 0;
  size_t want = std::max<size_t>(bytes, 1 << 20);
  HIP_TRY(hipMalloc(&e->d_scratch, want));
  HIP_TRY(hipHostMalloc(&e->h_scratch, want, hipHostMallocDefault));
  e->scratch_bytes = want;
  return FFN_OK;
}

int ensure_turn(ffn_engine* e, size_t n, size_t hist_n, size_t novl) {
  if (n > e->turn_ncap || hist_n > e->turn_hcap || novl > e->turn_ocap) {
    HIP_TRY(hipStreamSynchronize(e->ustream));  // (only utility calls use it)
    if (e->d_turn) HIP_TRY(hipFree(e->d_turn));
    if (e->h_turn) HIP_TRY(hipHostFree(e->h_turn));
    e->d_turn = nullptr;
    e->h_turn = e->h_turn_dev = nullptr;
    const size_t ncap = (std::max<size_t>({n, e->turn_ncap, 256}) + 3) & ~(size_t)3;
    const size_t hcap = std::max<size_t>({hist_n, e->turn_hcap, (size_t)kTurnHistLds});
    const size_t ocap = std::max<size_t>({novl, e->turn_ocap, 1024});
    e->turn_ncap = e->turn_hcap = e->turn_ocap = 0;
    const TurnLayout lay(ncap, hcap, ocap);
    HIP_TRY(hipMalloc(&e->d_turn, lay.d_bytes));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->h_turn), lay.h_words * 8,
                          hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(e->h_turn, 0, lay.h_words * 8);  // no word carries a live turn's number
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&e->h_turn_dev), e->h_turn, 0));
    e->turn_ncap = ncap;
    e->turn_hcap = hcap;
    e->turn_ocap = ocap;
    e->turn_hist_clean = false;
  }
  if (!e->turn_hist_clean) {
    // newly allocated, grown, or left behind by a turn that failed: zeroed here, once
    const TurnLayout lay(e->turn_ncap, e->turn_hcap, e->turn_ocap);
    HIP_TRY(hipMemsetAsync(static_cast<char*>(e->d_turn) + lay.o_hist, 0,
                           4 * e->turn_hcap, e->ustream));
  }
  e->turn_hist_clean = false;  // until this turn's publish kernel has run
  return FFN_OK;
}

namespace {

// for_box_rows: log2 of the lanes a row of nx voxels gets (1 .. 64 of them)
int row_lanes_log2(int nx) {
  int xs = 0;
  while (xs < 6 && (1 << xs) < nx) ++xs;
  return xs;
}

// the grid of a for_box_rows sweep: 4 waves per block, 64 >> xs rows per wave pass
int turn_grid(long rows, int xs) {
  const long per_block = 4 * (64 >> xs);
  return (int)std::max<long>(1, std::min<long>((rows + per_block - 1) / per_block,
                                               kTurnBlocks));
}

Box make_box(const ffn_canvas* c, const int32_t lo[3], const int32_t hi[3],
             long* total) {
  Box b;
  for (int k = 0; k < 3; ++k) {
    b.lo[k] = lo[k];
    b.n[k] = hi[k] - lo[k];
  }
  b.cy = c->cy;
  b.cx = c->cx;
  *total = (long)b.n[0] * b.n[1] * b.n[2];
  return b;
}

}  // namespace

extern "C" {

namespace {

// image_f32 (already normalised) or image_u8 + the normalisation constants
int canvas_create(ffn_engine* e, const float* image_f32, const uint8_t* image_u8,
                  float mean, float stddev, const int32_t shape_zyx[3],
                  ffn_canvas** out) {
  EngineLock lock_(e);
  if (!e || (!image_f32 && !image_u8) || !shape_zyx || !out)
    return fail(FFN_ERR_ARG, "null argument");
  *out = nullptr;
  for (int k = 0; k < 3; ++k)
    if (shape_zyx[k] < 1) return fail(FFN_ERR_ARG, "bad canvas shape");
  if (image_u8 && !(stddev != 0.0f))
    return fail(FFN_ERR_ARG, "image_stddev must be non-zero");
  HIP_TRY(hipSetDevice(e->device));
  ffn_canvas* c = new ffn_canvas();
  c->engine = e;
  c->cz = shape_zyx[0];
  c->cy = shape_zyx[1];
  c->cx = shape_zyx[2];
  c->nvox = (size_t)c->cz * c->cy * c->cx;
  hipError_t err = hipSuccess;
  if (image_f32) {
    err = hipMalloc(&c->image, c->nvox * sizeof(float));
    if (err == hipSuccess)
      err = hipMemcpy(c->image, image_f32, c->nvox * sizeof(float),
                      hipMemcpyHostToDevice);
  } else {
    // (image.astype(np.float32) - image_mean) / image_stddev (runner.py:383-385):
    // two correctly rounded f32 operations per value, evaluated here for the
    // 256 possible inputs -- the device only looks the result up, so a uint8
    // canvas is bit-identical to the f32 one by construction
    float lut[256];
    for (int v = 0; v < 256; ++v) {
      volatile float d = (float)v - mean;  // volatile: no fused / widened form
      lut[v] = d / stddev;
    }
    err = hipMalloc(&c->image_u8, c->nvox);
    if (err == hipSuccess) err = hipMalloc(&c->image_lut, sizeof(lut));
    if (err == hipSuccess)
      err = hipMemcpy(c->image_u8, image_u8, c->nvox, hipMemcpyHostToDevice);
    if (err == hipSuccess)
      err = hipMemcpy(c->image_lut, lut, sizeof(lut), hipMemcpyHostToDevice);
  }
  if (err == hipSuccess) err = hipMalloc(&c->seed, c->nvox * sizeof(float));
  if (err == hipSuccess) err = hipMalloc(&c->seg, c->nvox * sizeof(int32_t));
  if (err == hipSuccess) err = hipMemset(c->seg, 0, c->nvox * sizeof(int32_t));
  if (err == hipSuccess) {
    hipLaunchKernelGGL(fill_u32_kernel, dim3(2048), dim3(256), 0, e->stream,
                       reinterpret_cast<uint32_t*>(c->seed), 0x7fc00000u, c->nvox);
    err = hipStreamSynchronize(e->stream);
  }
  if (err != hipSuccess) {
    int rc = fail(FFN_ERR_HIP, "canvas allocation failed: %s", hipGetErrorString(err));
    ffn_canvas_destroy(c);
    return rc;
  }
  {
    const hipError_t ee = hipEventCreateWithFlags(&c->ev_util, hipEventDisableTiming);
    if (ee != hipSuccess) {
      int rc = fail(FFN_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(ee));
      ffn_canvas_destroy(c);
      return rc;
    }
  }
  e->canvases.push_back(c);
  *out = c;
  return FFN_OK;
}

}  // namespace

int ffn_canvas_create(ffn_engine* e, const float* image_f32,
                      const int32_t shape_zyx[3], ffn_canvas** out) {
  if (!image_f32) return fail(FFN_ERR_ARG, "null argument");
  return canvas_create(e, image_f32, nullptr, 0.f, 1.f, shape_zyx, out);
}

int ffn_canvas_create_u8(ffn_engine* e, const uint8_t* image_u8,
                         const int32_t shape_zyx[3], float image_mean,
                         float image_stddev, ffn_canvas** out) {
  if (!image_u8) return fail(FFN_ERR_ARG, "null argument");
  return canvas_create(e, nullptr, image_u8, image_mean, image_stddev, shape_zyx,
                       out);
}

void ffn_canvas_destroy(ffn_canvas* c) {
  if (c && c->engine) (void)resolve_many_carry(c->engine, c);  // a step in flight
  EngineLock lock_(c ? c->engine : nullptr);
  if (!c) return;
  if (c->engine) {
    ffn_engine* e = c->engine;
    drop_spec(e);
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    (void)hipStreamSynchronize(e->ustream);
    if (c->ev_util) (void)hipEventDestroy(c->ev_util);
    e->canvases.erase(std::remove(e->canvases.begin(), e->canvases.end(), c),
                      e->canvases.end());
    (void)hipFree(c->image);
    (void)hipFree(c->image_u8);
    (void)hipFree(c->image_lut);
    (void)hipFree(c->seed);
    (void)hipFree(c->seg);
    (void)hipFree(c->restrict_planes);
  }
  delete c;
}

int ffn_canvas_init_seed(ffn_canvas* c, const int32_t pos[3], float value) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !pos) return fail(FFN_ERR_ARG, "null argument");
  if (pos[0] < 0 || pos[0] >= c->cz || pos[1] < 0 || pos[1] >= c->cy ||
      pos[2] < 0 || pos[2] >= c->cx)
    return fail(FFN_ERR_ARG, "seed position outside the canvas");
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c));
  if (c->dirty_lo[0] < c->dirty_hi[0]) {
    long total = 0;
    Box b = make_box(c, c->dirty_lo, c->dirty_hi, &total);
    if ((size_t)total * 2 >= c->nvox) {  // most of the volume: linear fill
      hipLaunchKernelGGL(fill_u32_kernel, dim3(2048), dim3(256), 0, e->ustream,
                         reinterpret_cast<uint32_t*>(c->seed), 0x7fc00000u,
                         c->nvox);
    } else if (total > 0) {
      hipLaunchKernelGGL((box_fill_kernel<uint32_t>), dim3(grid_for(total)),
                         dim3(256), 0, e->ustream,
                         reinterpret_cast<uint32_t*>(c->seed), b, total,
                         0x7fc00000u);
    }
  }
  {
    const int lo[3] = {pos[0], pos[1], pos[2]};
    const int hi[3] = {pos[0] + 1, pos[1] + 1, pos[2] + 1};
    c->dirty_lo[0] = c->dirty_hi[0] = 0;  // clean, then the seed point itself
    c->mark_dirty(lo, hi);
  }
  const size_t ci = ((size_t)pos[0] * c->cy + pos[1]) * c->cx + pos[2];
  hipLaunchKernelGGL(set_seed_point_kernel, dim3(1), dim3(1), 0, e->ustream,
                     c->seed, ci, value);
  HIP_TRY(hipGetLastError());
  HIP_TRY(lock_.end(e, c));
  return FFN_OK;
}

int ffn_canvas_segment_history(ffn_canvas* c, size_t first, size_t n,
                               int32_t* pos, uint32_t* deleted, size_t* total) {
  if (!c) return fail(FFN_ERR_ARG, "null canvas");
  if (c->engine)
    if (int rc = resolve_many_carry(c->engine, c)) return rc;
  const size_t have = c->loop.history_deleted.size();
  if (total) *total = have;
  if (n == 0) return FFN_OK;
  if (first > have || n > have - first)
    return fail(FFN_ERR_ARG, "history range [%zu, +%zu) of %zu", first, n, have);
  if (pos) std::memcpy(pos, c->loop.history.data() + 3 * first, 12 * n);
  if (deleted) std::memcpy(deleted, c->loop.history_deleted.data() + first, 4 * n);
  return FFN_OK;
}

int ffn_canvas_set_restrictor(ffn_canvas* c, const uint8_t* mask,
                              const uint8_t* seed_mask, const uint8_t* shift_mask,
                              const int32_t shift_shape[3], const int32_t pre[3],
                              const int32_t post[3], int32_t scale) {
  if (!c) return fail(FFN_ERR_ARG, "null canvas");
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  if (shift_mask) {
    if (!shift_shape || !pre || !post)
      return fail(FFN_ERR_ARG, "shift mask without its shape / FoV offsets");
    for (int k = 0; k < 3; ++k) {
      if (shift_shape[k] < 1) return fail(FFN_ERR_ARG, "bad shift mask shape");
      // (post >= -1: every numpy stop of is_valid_pos is >= 0 at a position >= 0)
      if (post[k] < -1) return fail(FFN_ERR_ARG, "shift mask FoV ends before 0");
    }
    if (scale < 1) return fail(FFN_ERR_ARG, "shift mask scale must be >= 1");
  }
  if (int rc = resolve_many_carry(e, c)) return rc;
  UtilLock lock_(e);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c));
  // the old planes: no turn queued on the utility stream may still read them
  HIP_TRY(hipStreamSynchronize(e->ustream));
  (void)hipFree(c->restrict_planes);
  c->restrict_planes = nullptr;
  c->restrict_plane_words = 0;
  c->restrict_row_words = 0;
  std::vector<uint64_t>().swap(c->restrict_host);
  c->loop.restrict_bits = nullptr;
  if (!mask && !seed_mask && !shift_mask) return FFN_OK;  // cleared

  const int Z = c->cz, Y = c->cy, X = c->cx;
  const int W = (X + 63) / 64;
  const size_t pw = (size_t)Z * Y * W;
  const size_t wave_blocks = std::min<size_t>((pw + 3) / 4, 8192);  // 4 waves / block
  unsigned long long* planes = nullptr;
  uint8_t* d_src = nullptr;
  unsigned long long *d_ax = nullptr, *d_ay = nullptr;
  hipError_t err = hipMalloc(&planes, 2 * pw * sizeof(uint64_t));
  // mask -> pos plane, seed mask -> seed plane: one u8 temporary at a time
  const uint8_t* srcs[2] = {mask, seed_mask};
  for (int k = 0; k < 2 && err == hipSuccess; ++k) {
    unsigned long long* plane = planes + k * pw;
    if (!srcs[k]) {
      err = hipMemsetAsync(plane, 0, pw * sizeof(uint64_t), e->ustream);
      continue;
    }
    err = hipMalloc(&d_src, c->nvox);
    if (err == hipSuccess) err = hipMemcpy(d_src, srcs[k], c->nvox, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
      hipLaunchKernelGGL(restrict_pack_kernel, dim3((unsigned)wave_blocks), dim3(256), 0,
                         e->ustream, d_src, (long)Z * Y, X, W, plane);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(e->ustream);
    (void)hipFree(d_src);
    d_src = nullptr;
  }
  if (shift_mask && err == hipSuccess) {
    const int Zs = shift_shape[0], Ys = shift_shape[1], Xs = shift_shape[2];
    const size_t ns = (size_t)Zs * Ys * Xs;
    const size_t nax = (size_t)Zs * Ys * W, nay = (size_t)Zs * Y * W;
    err = hipMalloc(&d_src, ns);
    if (err == hipSuccess) err = hipMalloc(&d_ax, nax * sizeof(uint64_t));
    if (err == hipSuccess) err = hipMalloc(&d_ay, nay * sizeof(uint64_t));
    if (err == hipSuccess) err = hipMemcpy(d_src, shift_mask, ns, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
      hipLaunchKernelGGL(restrict_shift_x_kernel,
                         dim3((unsigned)std::min<size_t>((nax + 3) / 4, 8192)), dim3(256),
                         0, e->ustream, d_src, (long)Zs * Ys, Xs, X, W, pre[2], post[2],
                         scale, d_ax);
      hipLaunchKernelGGL(restrict_shift_y_kernel, dim3(grid_for((long)nay)), dim3(256), 0,
                         e->ustream, d_ax, Zs, Ys, Y, W, pre[1], post[1], scale, d_ay);
      hipLaunchKernelGGL(restrict_shift_z_kernel, dim3(grid_for((long)pw)), dim3(256), 0,
                         e->ustream, d_ay, Zs, Z, Y, W, pre[0], post[0], planes);
      err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(e->ustream);
    (void)hipFree(d_src);
    (void)hipFree(d_ax);
    (void)hipFree(d_ay);
    d_src = nullptr;
  }
  if (err == hipSuccess) err = hipStreamSynchronize(e->ustream);
  // the host loop's copy of the pos plane (1 bit / voxel)
  if (err == hipSuccess) {
    try {
      c->restrict_host.resize(pw);
    } catch (const std::bad_alloc&) {
      (void)hipFree(planes);
      return fail(FFN_ERR_ARG, "no host memory for the restriction plane");
    }
    err = hipMemcpy(c->restrict_host.data(), planes, pw * sizeof(uint64_t),
                    hipMemcpyDeviceToHost);
  }
  if (err != hipSuccess) {
    (void)hipFree(planes);
    std::vector<uint64_t>().swap(c->restrict_host);
    return fail(FFN_ERR_HIP, "restriction planes: %s", hipGetErrorString(err));
  }
  c->restrict_planes = planes;
  c->restrict_plane_words = pw;
  c->restrict_row_words = W;
  c->loop.restrict_bits = c->restrict_host.data();
  c->loop.restrict_dims[0] = Z;
  c->loop.restrict_dims[1] = Y;
  c->loop.restrict_dims[2] = X;
  c->loop.restrict_row_words = W;
  return FFN_OK;
}

int ffn_canvas_read_restriction(ffn_canvas* c, const int32_t lo[3],
                                const int32_t hi[3], uint8_t* dst) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (int rc = check_canvas(c)) return rc;
  if (!lo || !hi || !dst) return fail(FFN_ERR_ARG, "null argument");
  if (int rc = check_box(c, lo, hi)) return rc;
  long total = 0;
  const Box b = make_box(c, lo, hi, &total);
  if (total <= 0) return FFN_OK;
  if (!c->restrict_planes) {  // no restrictor: nothing is blocked
    std::memset(dst, 0, (size_t)total);
    return FFN_OK;
  }
  ffn_engine* e = c->engine;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c, true));
  uint8_t* d_out = nullptr;
  HIP_TRY(hipMalloc(&d_out, (size_t)total));
  hipLaunchKernelGGL(restrict_read_kernel, dim3(grid_for(total)), dim3(256), 0,
                     e->ustream, c->restrict_planes, c->restrict_plane_words, c->cy,
                     c->restrict_row_words, b.lo[0], b.lo[1], b.lo[2], b.n[1], b.n[2],
                     total, d_out);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipStreamSynchronize(e->ustream);
  if (err == hipSuccess) err = hipMemcpy(dst, d_out, (size_t)total, hipMemcpyDeviceToHost);
  (void)hipFree(d_out);
  if (err != hipSuccess)
    return fail(FFN_ERR_HIP, "read_restriction: %s", hipGetErrorString(err));
  return FFN_OK;
}

int ffn_canvas_take_restricted_skips(ffn_canvas* c, int64_t* out) {
  if (!c || !out) return fail(FFN_ERR_ARG, "null argument");
  if (c->engine)
    if (int rc = resolve_many_carry(c->engine, c)) return rc;
  *out = c->loop.skip_restricted;
  c->loop.skip_restricted = 0;
  return FFN_OK;
}

int ffn_canvas_read_points(ffn_canvas* c, int n, const int32_t* pos,
                           float* seed_out, int32_t* seg_out) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !pos || !seed_out || !seg_out) return fail(FFN_ERR_ARG, "null argument");
  if (n < 1) return FFN_OK;
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c, true));
  const size_t pb = sizeof(int32_t) * 3 * n;
  const size_t pbr = (pb + 15) & ~(size_t)15;
  int rc = ensure_scratch(e, pbr + 8 * (size_t)n);
  if (rc) return rc;
  char* hs = static_cast<char*>(e->h_scratch);
  char* ds = static_cast<char*>(e->d_scratch);
  std::memcpy(hs, pos, pb);
  HIP_TRY(hipMemcpyAsync(ds, hs, pb, hipMemcpyHostToDevice, e->ustream));
  float* d_seed = reinterpret_cast<float*>(ds + pbr);
  int32_t* d_seg = reinterpret_cast<int32_t*>(ds + pbr + 4 * (size_t)n);
  hipLaunchKernelGGL(points_read_kernel, dim3((n + 63) / 64), dim3(64), 0,
                     e->ustream, c->seed, c->seg, c->cz, c->cy, c->cx, n,
                     reinterpret_cast<const int32_t*>(ds), d_seed, d_seg);
  HIP_TRY(hipMemcpyAsync(hs + pbr, ds + pbr, 8 * (size_t)n, hipMemcpyDeviceToHost,
                         e->ustream));
  HIP_TRY(lock_.wait(e, c));
  std::memcpy(seed_out, hs + pbr, 4 * (size_t)n);
  std::memcpy(seg_out, hs + pbr + 4 * (size_t)n, 4 * (size_t)n);
  return FFN_OK;
}

int ffn_canvas_write_seg_points(ffn_canvas* c, int n, const int32_t* pos,
                                const int32_t* values) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !pos || !values) return fail(FFN_ERR_ARG, "null argument");
  if (n < 1) return FFN_OK;
  for (int k = 0; k < n; ++k)
    if (pos[3 * k] < 0 || pos[3 * k] >= c->cz || pos[3 * k + 1] < 0 ||
        pos[3 * k + 1] >= c->cy || pos[3 * k + 2] < 0 || pos[3 * k + 2] >= c->cx)
      return fail(FFN_ERR_ARG, "point %d outside the canvas", k);
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c));
  if (n == 1) {  // (the -1 marker of a rejected seed: nothing to wait for)
    const size_t ci = ((size_t)pos[0] * c->cy + pos[1]) * c->cx + pos[2];
    hipLaunchKernelGGL(set_seg_point_kernel, dim3(1), dim3(1), 0, e->ustream, c->seg,
                       ci, values[0]);
    HIP_TRY(hipGetLastError());
    HIP_TRY(lock_.end(e, c));
    return FFN_OK;
  }
  const size_t pb = sizeof(int32_t) * 3 * n;
  const size_t pbr = (pb + 15) & ~(size_t)15;
  int rc = ensure_scratch(e, pbr + 4 * (size_t)n);
  if (rc) return rc;
  char* hs = static_cast<char*>(e->h_scratch);
  char* ds = static_cast<char*>(e->d_scratch);
  std::memcpy(hs, pos, pb);
  std::memcpy(hs + pbr, values, 4 * (size_t)n);
  HIP_TRY(hipMemcpyAsync(ds, hs, pbr + 4 * (size_t)n, hipMemcpyHostToDevice,
                         e->ustream));
  hipLaunchKernelGGL(points_write_seg_kernel, dim3((n + 63) / 64), dim3(64), 0,
                     e->ustream, c->seg, c->cy, c->cx, n,
                     reinterpret_cast<const int32_t*>(ds),
                     reinterpret_cast<const int32_t*>(ds + pbr));
  HIP_TRY(lock_.wait(e, c));
  return FFN_OK;
}

int ffn_canvas_any_segmented(ffn_canvas* c, const int32_t lo[3],
                             const int32_t hi[3], int32_t* out) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !lo || !hi || !out) return fail(FFN_ERR_ARG, "null argument");
  // numpy slicing clips to the array bounds (inference.py:575-578)
  int32_t l[3], h[3];
  const int dims[3] = {c->cz, c->cy, c->cx};
  for (int k = 0; k < 3; ++k) {
    l[k] = std::max(lo[k], 0);
    h[k] = std::min(hi[k], dims[k]);
    if (h[k] <= l[k]) {
      *out = 0;
      return FFN_OK;
    }
  }
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c));
  int rc = ensure_scratch(e, 16);
  if (rc) return rc;
  long total;
  Box b = make_box(c, l, h, &total);
  HIP_TRY(hipMemsetAsync(e->d_scratch, 0, 4, e->ustream));
  hipLaunchKernelGGL(any_segmented_kernel, dim3(grid_for(total)), dim3(256), 0,
                     e->ustream, c->seg, b, total,
                     static_cast<int32_t*>(e->d_scratch));
  HIP_TRY(hipMemcpyAsync(e->h_scratch, e->d_scratch, 4, hipMemcpyDeviceToHost,
                         e->ustream));
  HIP_TRY(lock_.wait(e, c));
  *out = *static_cast<int32_t*>(e->h_scratch);
  return FFN_OK;
}

int ffn_canvas_commit_count(ffn_canvas* c, const int32_t lo[3],
                            const int32_t hi[3], float segment_threshold,
                            int32_t max_existing_id, ffn_commit_counts* counts,
                            int32_t max_overlaps, int32_t* overlap_ids,
                            int64_t* overlap_counts) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !lo || !hi || !counts) return fail(FFN_ERR_ARG, "null argument");
  int rc = check_box(c, lo, hi);
  if (rc) return rc;
  if (max_existing_id < 0) max_existing_id = 0;
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c));
  // the turn's count and publish kernels: two launches, the answer polled
  const int novl = overlap_ids && overlap_counts
                       ? std::max(std::min(max_overlaps, max_existing_id), 0) : 0;
  rc = ensure_turn(e, 0, (size_t)max_existing_id + 1, (size_t)novl);
  if (rc) return rc;
  const TurnLayout lay(e->turn_ncap, e->turn_hcap, e->turn_ocap);
  char* ds = static_cast<char*>(e->d_turn);
  auto* d_part = reinterpret_cast<unsigned long long*>(ds + lay.o_part);
  auto* d_hist = reinterpret_cast<unsigned*>(ds + lay.o_hist);
  if (++e->turn_seq == 0) ++e->turn_seq;
  long total;
  Box b = make_box(c, lo, hi, &total);
  const long rows = total > 0 ? (long)b.n[0] * b.n[1] : 0;
  const int xs = row_lanes_log2(b.n[2]);
  const int nparts = rows > 0 ? turn_grid(rows, xs) : 0;
  if (nparts > 0)
    hipLaunchKernelGGL(turn_count_kernel, dim3(nparts), dim3(256), 0, e->ustream, c->seed,
                       c->seg, b, rows, xs, segment_threshold, max_existing_id,
                       max_existing_id < kTurnHistLds ? 1 : 0, d_part, d_hist);
  hipLaunchKernelGGL(turn_publish_kernel, dim3(1), dim3(1024), 0, e->ustream,
                     reinterpret_cast<const TurnRecord*>(ds), d_part, nparts, d_hist,
                     max_existing_id, novl, nullptr, nullptr, nullptr, 0, 0, 0,
                     e->h_turn_dev + lay.w_pub, e->turn_seq);
  HIP_TRY(hipGetLastError());
  const TurnPub pub{e->h_turn + lay.w_pub, e->turn_seq, 0};
  HIP_TRY(lock_.wait_published(e, c, [&] { return pub.arrived(); }));
  e->turn_hist_clean = true;
  counts->raw_segmented_voxels = (int64_t)(pub.at(0) | (uint64_t)pub.at(1) << 32);
  counts->actual_segmented_voxels = (int64_t)(pub.at(2) | (uint64_t)pub.at(3) << 32);
  counts->num_overlapped_ids = pub.overlaps(overlap_ids, overlap_counts);
  return FFN_OK;
}

int ffn_canvas_commit_assign(ffn_canvas* c, const int32_t lo[3],
                             const int32_t hi[3], float segment_threshold,
                             int32_t segment_id) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !lo || !hi) return fail(FFN_ERR_ARG, "null argument");
  int rc = check_box(c, lo, hi);
  if (rc) return rc;
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(lock_.begin(e, c));
  long total;
  Box b = make_box(c, lo, hi, &total);
  if (total > 0)
    hipLaunchKernelGGL(commit_assign_kernel, dim3(grid_for(total)), dim3(256), 0,
                       e->ustream, c->seed, c->seg, b, total, segment_threshold,
                       segment_id);
  HIP_TRY(hipGetLastError());
  HIP_TRY(lock_.end(e, c));
  return FFN_OK;
}

int ffn_canvas_segment_turn(ffn_canvas* c, const ffn_turn_request* rq,
                            const int32_t* cand, ffn_turn_result* out,
                            int32_t max_overlaps, int32_t* overlap_ids,
                            int64_t* overlap_counts, int32_t* cand_flags,
                            float* cand_seed, int32_t* cand_seg) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !rq || !out) return fail(FFN_ERR_ARG, "null argument");
  const int n = rq->num_candidates;
  if (n < 0 || (n > 0 && (!cand || !cand_flags || !cand_seed || !cand_seg)))
    return fail(FFN_ERR_ARG, "candidate arrays");
  int rc = FFN_OK;
  if (rq->do_commit && (rc = check_box(c, rq->lo, rq->hi))) return rc;
  auto inside = [&](const int32_t* p) {
    return p[0] >= 0 && p[0] < c->cz && p[1] >= 0 && p[1] < c->cy && p[2] >= 0 &&
           p[2] < c->cx;
  };
  if (rq->mark_mode && !inside(rq->mark_pos))
    return fail(FFN_ERR_ARG, "marker outside the canvas");
  for (int k = 0; k < n; ++k)
    if (!inside(cand + 3 * k)) return fail(FFN_ERR_ARG, "candidate %d outside the canvas", k);
  for (int a = 0; a < 3; ++a)
    if (rq->min_boundary_dist[a] < 0) return fail(FFN_ERR_ARG, "min_boundary_dist");
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  const long long t_turn0 = steady_ns();
  HIP_TRY(lock_.begin(e, c));
  const int32_t max_id = rq->do_commit ? std::max(rq->max_existing_id, 0) : 0;
  const int novl = rq->do_commit && overlap_ids && overlap_counts
                       ? std::max(std::min(max_overlaps, max_id), 0) : 0;
  rc = ensure_turn(e, (size_t)n, (size_t)max_id + 1, (size_t)novl);
  if (rc) return rc;
  const TurnLayout lay(e->turn_ncap, e->turn_hcap, e->turn_ocap);
  char* ds = static_cast<char*>(e->d_turn);
  const size_t ncap = e->turn_ncap;
  auto* d_rec = reinterpret_cast<TurnRecord*>(ds);
  auto* d_part = reinterpret_cast<unsigned long long*>(ds + lay.o_part);
  auto* d_flag = reinterpret_cast<int*>(ds + lay.o_flag);
  auto* d_cseed = reinterpret_cast<float*>(ds + lay.o_flag + 4 * ncap);
  auto* d_cseg = reinterpret_cast<int32_t*>(ds + lay.o_flag + 8 * ncap);
  auto* d_ci = reinterpret_cast<size_t*>(ds + lay.o_flag + 12 * ncap);
  auto* d_hist = reinterpret_cast<unsigned*>(ds + lay.o_hist);
  if (++e->turn_seq == 0) ++e->turn_seq;
  // the candidates reach the device without a copy operation: the evaluate kernel reads
  // the pinned buffer (the call does not return before the turn has run, so one buffer)
  if (n > 0) std::memcpy(e->h_turn, cand, 12 * (size_t)n);
  long total = 0;
  Box b = make_box(c, rq->lo, rq->hi, &total);
  if (!rq->do_commit) {
    total = 0;
    b.n[0] = b.n[1] = b.n[2] = 0;
  }
  const long rows = total > 0 ? (long)b.n[0] * b.n[1] : 0;
  const int xs = row_lanes_log2(b.n[2]);
  const int nparts = rows > 0 ? turn_grid(rows, xs) : 0;
  const bool has_commit = rq->do_commit || rq->mark_mode;
  if (nparts > 0)
    hipLaunchKernelGGL(turn_count_kernel, dim3(nparts), dim3(256), 0, e->ustream, c->seed,
                       c->seg, b, rows, xs, rq->segment_threshold, max_id,
                       max_id < kTurnHistLds ? 1 : 0, d_part, d_hist);
  if (has_commit)
    hipLaunchKernelGGL(turn_commit_kernel, dim3(std::max(nparts, 1)), dim3(256), 0,
                       e->ustream, c->seed, c->seg, b, rows, xs, rq->segment_threshold,
                       rq->segment_id, (long long)rq->min_segment_size, d_part, nparts,
                       d_rec, rq->mark_pos[0], rq->mark_pos[1], rq->mark_pos[2],
                       rq->mark_mode);
  if (n > 0) {
    hipLaunchKernelGGL(turn_eval_kernel, dim3(n), dim3(64), 0, e->ustream, c->seed,
                       c->seg, c->cz, c->cy, c->cx,
                       reinterpret_cast<const int32_t*>(e->h_turn_dev),
                       rq->min_boundary_dist[0], rq->min_boundary_dist[1],
                       rq->min_boundary_dist[2], d_flag, d_cseed, d_cseg, d_ci,
                       c->restrict_planes, c->restrict_plane_words, c->restrict_row_words);
    // pick, and init_seed at the one picked: the dirty box (or, from half the volume on,
    // everything) back to NaN and the seed point, in the same launch
    long dirty_total = 0;
    Box db = make_box(c, c->dirty_lo, c->dirty_hi, &dirty_total);
    if (!rq->do_init || c->dirty_lo[0] >= c->dirty_hi[0] || dirty_total <= 0) {
      dirty_total = 0;
      db.n[0] = db.n[1] = db.n[2] = 0;
    }
    const long drows = dirty_total > 0 ? (long)db.n[0] * db.n[1] : 0;
    const int dxs = row_lanes_log2(db.n[2]);
    const int clear = !rq->do_init ? 0 : (size_t)dirty_total * 2 >= c->nvox ? 2 : 1;
    const int grid = clear == 2 ? 2048 : clear == 1 ? turn_grid(drows, dxs) : 1;
    uint32_t init_bits;
    std::memcpy(&init_bits, &rq->init_value, 4);
    hipLaunchKernelGGL(turn_pick_clear_kernel, dim3(grid), dim3(256), 0, e->ustream,
                       reinterpret_cast<uint32_t*>(c->seed), c->seg, d_flag, d_ci, n,
                       d_rec, db, drows, dxs, clear, c->nvox, init_bits);
  }
  hipLaunchKernelGGL(turn_publish_kernel, dim3(1), dim3(1024), 0, e->ustream, d_rec,
                     d_part, 0, d_hist, max_id, novl, d_flag, d_cseed, d_cseg, n,
                     has_commit ? 1 : 0, n > 0 ? 1 : 0, e->h_turn_dev + lay.w_pub,
                     e->turn_seq);
  HIP_TRY(hipGetLastError());
  const long long t_turn1 = steady_ns();
  const TurnPub pub{e->h_turn + lay.w_pub, e->turn_seq, (size_t)n};
  HIP_TRY(lock_.wait_published(e, c, [&] { return pub.arrived(); }));
  e->turn_hist_clean = true;
  e->stat_segturn_queue_ns += t_turn1 - t_turn0;
  e->stat_segturn_wait_ns += steady_ns() - t_turn1;
  e->stat_segturn_calls += 1;
  std::memset(out, 0, sizeof(*out));
  out->counts.raw_segmented_voxels = (int64_t)(pub.at(0) | (uint64_t)pub.at(1) << 32);
  out->counts.actual_segmented_voxels = (int64_t)(pub.at(2) | (uint64_t)pub.at(3) << 32);
  out->committed = (int32_t)pub.at(4);
  out->chosen = (int32_t)pub.at(5);
  out->counts.num_overlapped_ids = pub.overlaps(overlap_ids, overlap_counts);
  if (n > 0) {
    for (int k = 0; k < n; ++k) {
      cand_flags[k] = (int32_t)pub.at(8 + (size_t)k);
      const uint32_t sb = pub.at(8 + (size_t)n + k);
      std::memcpy(&cand_seed[k], &sb, 4);
      cand_seg[k] = (int32_t)pub.at(8 + 2 * (size_t)n + k);
    }
    if (rq->do_init && out->chosen >= 0) {
      // as ffn_canvas_init_seed: the volume is clean but for the seed point
      const int32_t* p = cand + 3 * out->chosen;
      const int lo[3] = {p[0], p[1], p[2]};
      const int hi[3] = {p[0] + 1, p[1] + 1, p[2] + 1};
      c->dirty_lo[0] = c->dirty_hi[0] = 0;
      c->mark_dirty(lo, hi);
    }
  }
  return FFN_OK;
}

}  // extern "C"

namespace {

template <typename T>
int box_read(ffn_canvas* c, const T* vol, const int32_t lo[3], const int32_t hi[3],
             T* dst) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !lo || !hi || !dst) return fail(FFN_ERR_ARG, "null argument");
  int rc = check_box(c, lo, hi);
  if (rc) return rc;
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  long total;
  Box b = make_box(c, lo, hi, &total);
  if (total == 0) return FFN_OK;
  if (total == (long)c->nvox) {  // whole volume: straight (blocking) copy
    HIP_TRY(canvas_quiesce(e, c));
    HIP_TRY(hipMemcpy(dst, vol, sizeof(T) * total, hipMemcpyDeviceToHost));
    return FFN_OK;
  }
  HIP_TRY(lock_.begin(e, c));
  rc = ensure_scratch(e, sizeof(T) * total);
  if (rc) return rc;
  hipLaunchKernelGGL((box_read_kernel<T>), dim3(grid_for(total)), dim3(256), 0,
                     e->ustream, vol, b, total, static_cast<T*>(e->d_scratch));
  HIP_TRY(hipMemcpyAsync(e->h_scratch, e->d_scratch, sizeof(T) * total,
                         hipMemcpyDeviceToHost, e->ustream));
  HIP_TRY(lock_.wait(e, c));
  std::memcpy(dst, e->h_scratch, sizeof(T) * total);
  return FFN_OK;
}

template <typename T>
int box_write(ffn_canvas* c, T* vol, const int32_t lo[3], const int32_t hi[3],
              const T* src) {
  UtilLock lock_(c ? c->engine : nullptr);
  if (!c || !lo || !hi || !src) return fail(FFN_ERR_ARG, "null argument");
  int rc = check_box(c, lo, hi);
  if (rc) return rc;
  ffn_engine* e = c->engine;
  if (!e) return fail(FFN_ERR_STATE, "canvas outlived its engine");
  HIP_TRY(hipSetDevice(e->device));
  long total;
  Box b = make_box(c, lo, hi, &total);
  if (total == 0) return FFN_OK;
  if (total == (long)c->nvox) {  // whole volume: straight (blocking) copy
    HIP_TRY(canvas_quiesce(e, c));
    HIP_TRY(hipMemcpy(vol, src, sizeof(T) * total, hipMemcpyHostToDevice));
    return FFN_OK;
  }
  HIP_TRY(lock_.begin(e, c));
  rc = ensure_scratch(e, sizeof(T) * total);
  if (rc) return rc;
  std::memcpy(e->h_scratch, src, sizeof(T) * total);
  HIP_TRY(hipMemcpyAsync(e->d_scratch, e->h_scratch, sizeof(T) * total,
                         hipMemcpyHostToDevice, e->ustream));
  hipLaunchKernelGGL((box_write_kernel<T>), dim3(grid_for(total)), dim3(256), 0,
                     e->ustream, vol, b, total,
                     static_cast<const T*>(e->d_scratch));
  HIP_TRY(lock_.wait(e, c));
  return FFN_OK;
}

}  // namespace

extern "C" {

int ffn_canvas_read_seed(ffn_canvas* c, const int32_t lo[3], const int32_t hi[3],
                         float* dst) {
  return box_read<float>(c, c ? c->seed : nullptr, lo, hi, dst);
}

int ffn_canvas_read_segmentation(ffn_canvas* c, const int32_t lo[3],
                                 const int32_t hi[3], int32_t* dst) {
  return box_read<int32_t>(c, c ? c->seg : nullptr, lo, hi, dst);
}

int ffn_canvas_write_seed(ffn_canvas* c, const int32_t lo[3], const int32_t hi[3],
                          const float* src) {
  if (c && lo && hi) c->mark_dirty(lo, hi);
  return box_write<float>(c, c ? c->seed : nullptr, lo, hi, src);
}

int ffn_canvas_write_segmentation(ffn_canvas* c, const int32_t lo[3],
                                  const int32_t hi[3], const int32_t* src) {
  return box_write<int32_t>(c, c ? c->seg : nullptr, lo, hi, src);
}

}  // extern "C"
