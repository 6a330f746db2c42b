// TEST INFRASTRUCTURE: the library's seed loop (ffn_host::SeedLoop of
// ffn_amd/csrc/ffn_host_loop.h -- what ffn_canvas_segment_all runs over the HIP
// canvas) instantiated over callbacks, the between-segment turn included, so that
// it runs against the emulated device of tests/emulated_device.py without a GPU.
// Built by tests/test_seed_loop.py with g++; never part of the product.
#include <cstddef>

#include "host_loop_restrict_shim.cpp"

extern "C" {

typedef int (*shim_turn_fn)(const ffn_turn_request*, const int32_t*, ffn_turn_result*,
                            int32_t, int32_t*, int64_t*, int32_t*, float*, int32_t*);

struct ShimSeedDevice : ShimDevice {
  shim_turn_fn turn_cb;
  int turn(const ffn_turn_request& rq, const int32_t* cand, ffn_turn_result* out,
           int32_t max_overlaps, int32_t* ids, int64_t* counts, int32_t* flags,
           float* cand_seed, int32_t* cand_seg) {
    return turn_cb(&rq, cand, out, max_overlaps, ids, counts, flags, cand_seed, cand_seg);
  }
};

void* shim_seed_state_create() { return new ffn_host::SeedLoopState(); }
void shim_seed_state_destroy(void* s) { delete static_cast<ffn_host::SeedLoopState*>(s); }

// ffn_canvas_segment_all, argument checks included
int shim_segment_all(void* state, void* seed_state, shim_step_fn step_cb,
                     shim_read_fn read_cb, shim_turn_fn turn_cb,
                     const ffn_seed_loop_args* args, ffn_seed_loop_result* out) {
  if (!ffn_host::seed_loop_args_ok(*args)) return FFN_ERR_ARG;
  ShimSeedDevice dev;
  dev.step_cb = step_cb;
  dev.read_cb = read_cb;
  dev.turn_cb = turn_cb;
  auto& st = *static_cast<ffn_host::SegmentState*>(state);
  auto& sl = *static_cast<ffn_host::SeedLoopState*>(seed_state);
  if (args->resume && !(sl.in_segment && st.active)) return FFN_ERR_STATE;
  ffn_host::SeedLoop<ShimSeedDevice> loop(dev, st, sl, *args, out);
  return loop.run();
}

size_t shim_sizeof_seed_record() { return sizeof(ffn_seed_record); }
size_t shim_sizeof_seed_args() { return sizeof(ffn_seed_loop_args); }
size_t shim_sizeof_seed_result() { return sizeof(ffn_seed_loop_result); }
size_t shim_sizeof_turn_request() { return sizeof(ffn_turn_request); }
// offsets of the last field of each struct: with the sizes, what a mirror gets wrong
size_t shim_offsetof_seed_record_segment() { return offsetof(ffn_seed_record, segment); }
size_t shim_offsetof_seed_args_overlap_counts() {
  return offsetof(ffn_seed_loop_args, overlap_counts);
}
size_t shim_offsetof_seed_args_min_segment_size() {
  return offsetof(ffn_seed_loop_args, min_segment_size);
}
size_t shim_offsetof_seed_result_in_segment() {
  return offsetof(ffn_seed_loop_result, in_segment);
}

}  // extern "C"
