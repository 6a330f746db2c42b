// TEST INFRASTRUCTURE: tests/host_loop_shim.cpp plus the restriction view of
// ffn_host::SegmentState (what ffn_canvas_set_restrictor hands the library's
// loop), so that the restricted loop runs over the emulated device with a bit
// plane built in numpy.  Built by tests/test_restrict_host_loop.py with g++;
// never part of the product.
#include "host_loop_shim.cpp"

extern "C" {

// bits: the pos_blocked plane, [dims[0]][dims[1]][row_words] 64-bit words (bit
// x % 64 of word x / 64); NULL clears it.  The caller keeps `bits` alive.
void shim_state_set_restriction(void* state, const uint64_t* bits,
                                const int32_t* dims, int64_t row_words) {
  auto& st = *static_cast<ffn_host::SegmentState*>(state);
  st.restrict_bits = bits;
  for (int a = 0; a < 3; ++a) st.restrict_dims[a] = bits ? dims[a] : 0;
  st.restrict_row_words = bits ? row_words : 0;
}

int64_t shim_take_restricted_skips(void* state) {
  auto& st = *static_cast<ffn_host::SegmentState*>(state);
  const int64_t n = st.skip_restricted;
  st.skip_restricted = 0;
  return n;
}

}  // extern "C"
