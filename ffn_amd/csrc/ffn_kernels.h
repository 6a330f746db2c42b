// What every kernel header of the FFN field-of-view engine starts from: the shared
// plain types (ffn_types.h: the activation layout is described there) and the small
// device helpers below.
//
// A kernel header that defines a non-template __global__ function is included by exactly
// ONE translation unit; one that holds templates and __forceinline__ device code only (T)
// by every unit that needs it.  Without relocatable device code a unit that instantiates
// a kernel gets its own device copy of it, so each kernel form is instantiated -- launched,
// given its attributes, asked for its occupancy -- in one unit alone.  All behind this
// header:
//   ffn_conv0a.h (T)        conv0_a in front of the stack: ffn_stack.hip launches its
//                           kernel, the fused step launch of ffn_hip.hip runs its body
//   ffn_hip.hip             ffn_step_kernels.h    faces, paste, the fused step launches
//   ffn_stack.hip           ffn_conv_exact.h      conv_variant 0, 2: exact f32; the head
//   the conv launch layer   ffn_conv_split.h (T)     conv_variant 6 .. 9: fp16 split
//   (ffn_stack_units.h)                              products, FLOW; conv32d's forms are
//                                                    ffn_stack_d.hip's, conv32m / mt's
//                                                    ffn_stack_m.hip's
//                           ffn_conv_resident.h (T)  conv32ps, the stack as one launch:
//                                                    ffn_stack_resident.hip
//                           (in this order: each builds on the one above it)
//   ffn_stack_resident.hip  ffn_conv_half.h       conv32h / conv32hs: two chains per SIMD
//                                                 (behind the two above)
//   ffn_canvas.hip          ffn_canvas_kernels.h  box I/O, commit, segment turn
//                           ffn_restrict_kernels.h  MovementRestrictor planes
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "ffn_types.h"

namespace ffn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// (global address space spelled out: through generic pointers these would be flat
// loads, which the compiler orders against every LDS access)
#define FFN_GLOBAL __attribute__((address_space(1)))

__device__ __forceinline__ bool in_pred_box(const Geom& g, int z, int y, int x) {
  return z >= g.c0[0] && z < g.c1[0] && y >= g.c0[1] && y < g.c1[1] && x >= g.c0[2] &&
         x < g.c1[2];
}

// Bytes of the explicit kernel arguments of a kernel with parameters of types T...: each
// at its natural alignment, in order (the layout of the kernarg segment); or of the kernel
// a function pointer type names.
template <class... T>
constexpr int kernarg_bytes() {
  size_t off = 0;
  ((off = (off + alignof(T) - 1) / alignof(T) * alignof(T) + sizeof(T)), ...);
  return (int)off;
}
template <class F>
struct KernargsOf;
template <class... T>
struct KernargsOf<void (*)(T...)> {
  static constexpr int bytes = kernarg_bytes<T...>();
};

// The kernel arguments of a launch that has just crossed a boundary are cold (the scalar
// cache was invalidated, the host wrote them to device memory), and a kernel with roles and
// branches reads them in STAGES: every s_load behind a branch is its own miss, 0.5 - 1 us
// each, one behind the other (the fused step launch: six stages before its first data load).
// This touches every 64-byte line of the first BYTES of the segment at once and waits for
// them once: one miss, the stages after it hit the scalar cache.
// BYTES comes from the kernel's own parameter types (kernarg_bytes below): a read past
// the explicit arguments is a read of whatever follows the segment.
template <int BYTES>
__device__ __forceinline__ void warm_kernargs() {
  const auto ka = __builtin_amdgcn_kernarg_segment_ptr();
  unsigned sink;
  static_assert(BYTES > 0 && BYTES <= 1024, "");
  // (line L is touched when the segment reaches it: assembler conditionals on BYTES)
#define FFN_KA(OFF) ".if %2 > " #OFF "\n\ts_load_dword %0, %1, " #OFF "\n\t.endif\n\t"
  asm volatile(FFN_KA(0x0) FFN_KA(0x40) FFN_KA(0x80) FFN_KA(0xc0) FFN_KA(0x100) FFN_KA(0x140)
               FFN_KA(0x180) FFN_KA(0x1c0) FFN_KA(0x200) FFN_KA(0x240) FFN_KA(0x280)
               FFN_KA(0x2c0) FFN_KA(0x300) FFN_KA(0x340) FFN_KA(0x380) FFN_KA(0x3c0)
               "s_waitcnt lgkmcnt(0)"
               : "=&s"(sink) : "s"(ka), "n"(BYTES) : "memory");
#undef FFN_KA
}

}  // namespace ffn
