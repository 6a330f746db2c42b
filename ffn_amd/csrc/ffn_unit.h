// Host scaffold shared by the side units of libffn_hip.so (ffn_labels,
// ffn_seeds, ffn_decision, ffn_analysis, ffn_partitions, ffn_coordinates,
// ffn_evaluation, ffn_gradients, ffn_optimizer, ffn_metrics; not part of the C-ABI): the
// error macros, grow-only buffers that free themselves, and the handle base with its create / destroy path
// and event-pair timer.  Host code only.
#ifndef FFN_UNIT_H_
#define FFN_UNIT_H_

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "../../include/ffn_hip.h"
#include "ffn_internal.h"

// HIP call -> FFN_ERR_HIP with the failing expression and its place.
#define U_TRY(expr)                                                           \
  do {                                                                        \
    hipError_t _e = (expr);                                                   \
    if (_e != hipSuccess)                                                     \
      return ffn_set_error(FFN_ERR_HIP, "%s failed: %s (%s:%d)", #expr,       \
                           hipGetErrorString(_e), __FILE__, __LINE__);        \
  } while (0)

// Return on a non-zero return code.
#define U_OK(expr)                 \
  do {                             \
    int _rc = (expr);              \
    if (_rc != FFN_OK) return _rc; \
  } while (0)

namespace ffn_unit {

// Grow-only device (or pinned host) memory owned by a handle.  Freed with the
// handle: unit_destroy() selects the device before it deletes.
template <bool kPinned>
struct Buffer {
  void* p = nullptr;
  size_t bytes = 0;

  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() {
    if (p) (void)release();
  }

  hipError_t release() { return kPinned ? hipHostFree(p) : hipFree(p); }
};
using DevBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

// No-op if `buf` holds `bytes` already; otherwise free, then allocate (the
// contents are not kept).  A request for 0 bytes allocates 16.
template <bool kPinned>
inline int ensure(Buffer<kPinned>& buf, size_t bytes) {
  if (buf.p && buf.bytes >= bytes) return FFN_OK;
  if (buf.p) U_TRY(buf.release());
  buf.p = nullptr;
  buf.bytes = 0;
  if (kPinned)
    U_TRY(hipHostMalloc(&buf.p, bytes ? bytes : 16, hipHostMallocDefault));
  else
    U_TRY(hipMalloc(&buf.p, bytes ? bytes : 16));
  buf.bytes = bytes ? bytes : 16;
  return FFN_OK;
}

// Base of the handle structs.  A unit's buffers are members of the derived
// struct, so deleting a handle frees them before the events and the stream go.
struct Unit {
  int device_id = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  ~Unit() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }

  int timer_start() {
    U_TRY(hipEventRecord(ev0, stream));
    return FFN_OK;
  }

  // Waits for the work queued since timer_start(); writes *ms on success only.
  int timer_stop(double* ms) {
    U_TRY(hipEventRecord(ev1, stream));
    U_TRY(hipEventSynchronize(ev1));
    float t = 0.f;
    U_TRY(hipEventElapsedTime(&t, ev0, ev1));
    *ms = t;
    return FFN_OK;
  }
};

template <typename H>
void unit_destroy(H* h) {
  if (!h) return;
  (void)hipSetDevice(h->device_id);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
}

template <typename H>
int unit_create(int device_id, H** out) {
  if (!out) return ffn_set_error(FFN_ERR_ARG, "out is NULL");
  *out = nullptr;
  int ndev = 0;
  U_TRY(hipGetDeviceCount(&ndev));
  if (device_id < 0 || device_id >= ndev)
    return ffn_set_error(FFN_ERR_ARG, "device %d not present (%d devices)",
                         device_id, ndev);
  U_TRY(hipSetDevice(device_id));
  H* h = new H();
  h->device_id = device_id;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&h->ev0);
  if (e == hipSuccess) e = hipEventCreate(&h->ev1);
  if (e != hipSuccess) {
    unit_destroy(h);
    return ffn_set_error(FFN_ERR_HIP, "stream/event creation failed: %s",
                         hipGetErrorString(e));
  }
  *out = h;
  return FFN_OK;
}

}  // namespace ffn_unit

#endif  // FFN_UNIT_H_
