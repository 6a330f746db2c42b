"""The engine's options (ffn_engine_set_option / ffn_engine_get_option, include/ffn_hip.h
and include/ffn_hip_debug.h) are host state behind one table: every name takes what it
took and refuses what it refused before the table existed.  The expectations below are
written out here, from the setter and getter chains the table replaced; nothing is read
from the library's table.  Through the C-ABI, on the smallest engine of the suite.
"""

import ctypes

import pytest

pytestmark = pytest.mark.gpu

FFN_OK, FFN_ERR_ARG = 0, -1

# Plain stores: (name, lo, hi); None = unbounded on that side.
RANGED = [
    ('batch_chunks', 0, 2),
    ('sync_mode', 0, 1),
    ('profile_every', 1, None),
    ('store_policy', 0, 2),
    ('paste_blocks', 0, 1024),
    ('flow_pace', -1, 5000),
    ('flow_pace_spread', -1, 5000),
    ('flow_pace_tail', 0, 5000),
    ('flow', 0, 2),
    ('debug_clock', None, None),
    ('debug_layer', None, None),
    ('ablate', None, None),
    ('flow_debug', None, None),  # (never 2048 here: that value injects a fault)
    ('spec_force_mismatch', None, None),
    ('debug_fused_twice', None, None),
    ('debug_submit_delay_ns', None, None),
]
# a value inside the range that is not the default, for the unbounded ones
LEGAL = {'profile_every': 3, 'debug_clock': 1, 'debug_layer': 5, 'ablate': 8, 'flow_debug': 1,
         'spec_force_mismatch': 2, 'debug_fused_twice': 1, 'debug_submit_delay_ns': 1000}
# Stores of value != 0.
ONOFF = ['tail_batched', 'speculate', 'stack_ahead', 'fuse_head', 'fuse_paste', 'fuse_conv0a']
# Set only: a get does not know the name.
SET_ONLY = ['stat_reset', 'debug_fused_trace']
# Get only: a set does not know the name.
GET_ONLY = [
    'exact_variant', 'flow_auto_off', 'flow_pace_now', 'flow_pace_free_ns', 'flow_pace_best_ns',
    'stat_step_calls', 'stat_step_items', 'stat_hist_0', 'stat_hist_64', 'stat_spec_launched',
    'stat_spec_hits', 'stat_spec_mismatch', 'stat_spec_miss_full', 'stat_spec_miss_short',
    'stat_ahead_used', 'stat_ahead_wasted', 'stat_ahead_aborted', 'stat_many_carried',
    'stat_flow_voids', 'stat_flow_timeouts', 'stat_segturn_calls', 'stat_segturn_queue_ns',
    'stat_segturn_wait_ns', 'stat_turn_count', 'stat_turn_host_ns', 'stat_launch_host_ns',
    'stat_turn_gpu_ns', 'debug_fused_stamp_4', 'debug_fused_stamp_27',
]
# Names neither side knows (prefix getters outside their range included).
REFUSED_GETS = ['no_such_option', '', 'stat_hist_65', 'stat_hist_-1', 'debug_fused_stamp_3',
                'debug_fused_stamp_15', 'debug_fused_stamp_28', 'conv_variant_']


def _engine(depth, weights=True):
  from ffn_amd import engine as hip_engine
  from oracle import ffn_oracle
  eng = hip_engine.HipEngine((33, 33, 33), (8, 8, 8), depth)
  if weights:
    variables = ffn_oracle.random_weights(depth, seed=5, stddev=0.05)
    eng.set_weights(ffn_oracle.weights_blob(variables, depth))
  return eng


def _set(eng, name, value):
  return eng._lib.ffn_engine_set_option(eng._h, name.encode(), int(value))


def _get(eng, name):
  value = ctypes.c_int(-12345)
  rc = eng._lib.ffn_engine_get_option(eng._h, name.encode(), ctypes.byref(value))
  return rc, value.value


def _one_step(eng):
  from ffn_amd import _lib
  from ffn_amd import synthetic
  from oracle import ffn_oracle
  canvas = eng.create_canvas(synthetic.normalize(synthetic.cells_volume((48, 48, 48), seed=3)))
  pos = (24, 24, 24)
  canvas.init_seed(pos, ffn_oracle.f32_logit(0.95))
  req = _lib.StepRequest()
  req.pos[:] = pos
  req.start_pos[:] = pos
  req.num_candidates = 0
  eng.step1(canvas, req,
            _lib.StepParams(ffn_oracle.f32_logit(0.05), ffn_oracle.f32_logit(0.9), 0.0))
  canvas.close()


def test_every_option_takes_and_refuses_what_it_did():
  eng = _engine(3)
  try:
    assert _get(eng, 'flow') == (FFN_OK, 2) and _get(eng, 'conv_variant') == (FFN_OK, 9)

    # stat_reset zeroes the step counters (one single-FoV step made first)
    assert _set(eng, 'stat_reset', 0) == FFN_OK
    _one_step(eng)
    assert _get(eng, 'stat_step_calls') == (FFN_OK, 1)
    assert _get(eng, 'stat_step_items') == (FFN_OK, 1)
    assert _get(eng, 'stat_hist_1') == (FFN_OK, 1)
    assert _set(eng, 'stat_reset', 0) == FFN_OK
    assert _get(eng, 'stat_step_calls') == (FFN_OK, 0)
    assert _get(eng, 'stat_step_items') == (FFN_OK, 0)
    assert _get(eng, 'stat_hist_1') == (FFN_OK, 0)

    # no step runs from here on: options are host state
    for name, lo, hi in RANGED:
      values = {v for v in (lo, hi, LEGAL.get(name)) if v is not None}
      if lo is not None and hi is not None:
        values.add((lo + hi) // 2)
      for v in sorted(values):
        assert _set(eng, name, v) == FFN_OK, (name, v)
        assert _get(eng, name) == (FFN_OK, v), (name, v)
      last = _get(eng, name)[1]
      if lo is not None:
        assert _set(eng, name, lo - 1) == FFN_ERR_ARG, name
      if hi is not None:
        assert _set(eng, name, hi + 1) == FFN_ERR_ARG, name
      assert _get(eng, name) == (FFN_OK, last), name  # a refused set stores nothing
    assert _set(eng, 'flow_debug', 0) == FFN_OK
    for name in ONOFF:
      for v, want in ((0, 0), (7, 1), (-1, 1), (0, 0), (1, 1)):
        assert _set(eng, name, v) == FFN_OK, (name, v)
        assert _get(eng, name) == (FFN_OK, want), (name, v)
    for name in SET_ONLY:
      assert _set(eng, name, 0) == FFN_OK, name
      assert _get(eng, name)[0] == FFN_ERR_ARG, name
    for name in GET_ONLY:
      assert _get(eng, name)[0] == FFN_OK, name
      assert _set(eng, name, 0) == FFN_ERR_ARG, name
    assert _get(eng, 'exact_variant') == (FFN_OK, 2)
    assert _get(eng, 'flow_auto_off') == (FFN_OK, 0)
    for name in REFUSED_GETS:
      assert _get(eng, name)[0] == FFN_ERR_ARG, name
      assert _set(eng, name, 0) == FFN_ERR_ARG, name
    assert _get(eng, 'no_such_option')[0] == FFN_ERR_ARG
    assert b"unknown option 'no_such_option'" in eng._lib.ffn_last_error()

    # conv_variant: the kernels of this FoV, -1 = its exact-f32 one; the removed ones refused
    for v, want in ((8, 8), (6, 6), (7, 7), (0, 0), (2, 2), (9, 9), (-1, 2), (9, 9)):
      assert _set(eng, 'conv_variant', v) == FFN_OK, v
      assert _get(eng, 'conv_variant') == (FFN_OK, want), v
    for v in (1, 3, 4, 5, 11, -2):
      assert _set(eng, 'conv_variant', v) == FFN_ERR_ARG, v
      assert _get(eng, 'conv_variant') == (FFN_OK, 9), v
    assert _set(eng, 'flow', 3) == FFN_ERR_ARG
  finally:
    eng.close()

  # flow hands rows from conv to conv: a depth-1 engine has nothing to hand on
  eng = _engine(1, weights=False)
  try:
    assert _get(eng, 'flow') == (FFN_OK, 0)
    assert _set(eng, 'flow', 2) == FFN_ERR_ARG
    assert _set(eng, 'flow', 1) == FFN_ERR_ARG
    assert _set(eng, 'flow', 0) == FFN_OK
    assert _get(eng, 'flow') == (FFN_OK, 0)
  finally:
    eng.close()
