/*
 * libffn_hip.so -- the lab side of the engine: pacing, ablation and trace options,
 * the "stat_*" counters and the debug readers.  Nothing here is needed to bind the
 * library (ffn_hip.h is); none of these options changes a result.  The names go
 * through ffn_engine_set_option / ffn_engine_get_option like the user's options;
 * every option that holds a value reads back what was set.
 */
#ifndef FFN_HIP_DEBUG_H_
#define FFN_HIP_DEBUG_H_

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- pacing of the resident launch ("flow" 2) -------------------------------
 * "flow_pace" -1..5000: the beat of the resident launch, in 10-ns ticks: conv l of
 *   a workgroup does not start before t0 + l x beat + "flow_pace_spread" x (its
 *   first voxel / V).  -1 (default) = the beat ffn_engine_set_weights MEASURED for
 *   this device (a ladder of beats on noise inputs, confirmed against the
 *   free-running launch in two alternating rounds: ~0.3 s, once per device, depth
 *   and FoV in a process; 0 if no beat wins by 1.5 %), 0 = free-running, > 0 =
 *   that beat.  "flow_pace_spread" -1..5000: -1 (default) = as wide as the beat;
 *   "flow_pace_tail" 0..5000: extra ticks for the tail workgroups.  Timing only:
 *   results are bit-identical under any beat (profiles/r06_pacing.txt).
 * Read-only: "flow_pace_now" (the beat in use), "flow_pace_free_ns" /
 *   "flow_pace_best_ns" (what the measurement saw per stack: free-running, at its
 *   best beat).
 *
 * ---- ablation and experiments ------------------------------------------------
 * "paste_blocks" 0..1024 (0 = automatic: one block per compute unit in the fused
 *   step launch).
 * "ablate" (variant 2): issue-rate experiments of the conv_b launch (8, 16, 24).
 * "flow_debug" 2048: fault injection for tests (a producer stops publishing); its
 *   other bits and "debug_clock" 4 act only in -DFFN_EXPERIMENTS=1 builds.
 * "flow_lab" 0 / 1: the resident stack (conv32ps_kernel) and the fused step launch
 *   (faces_paste_conv0a_kernel) are built twice -- a production form without any of
 *   the run-time plumbing of this header, and a LAB form with all of it.  0
 *   (default): the LAB form runs where one of "debug_clock", "debug_layer",
 *   "flow_debug" is away from its default, for a step traced by
 *   "debug_fused_trace", and in -DFFN_EXPERIMENTS / -DFFN_ABLATE builds; the
 *   production form otherwise.  1: always the LAB form.  Same results bit for bit.
 *   "stat_lab_launches" (read-only, zeroed by "stat_reset"): resident stacks queued
 *   in the LAB form.
 * "spec_force_mismatch" N: the next N steps that match a launch made ahead are
 *   treated as mismatches (test hook of the repeat path).
 * "debug_submit_delay_ns": the host idles this long in front of every step's
 *   launches (what a slower host costs with and without stack_ahead).
 * "debug_fused_twice": the fused step launch is made twice (idempotent), so that a
 *   trace of the second shows what warm caches are worth (nothing:
 *   profiles/r06_turn_around.txt).
 *
 * ---- traces ------------------------------------------------------------------
 * "debug_clock" 1..4 and "debug_layer": what the debug readers below record, and
 *   for which conv launch of the stack.
 * "debug_fused_trace" N (write-only): the N-th next single-FoV step stamps when each
 *   role of its two launches ran; read as "debug_fused_stamp_4" .. "_27", 10-ns
 *   ticks after the stack's first workgroup -- under stack_ahead after the entry of
 *   the step's faces block (tools/gpu_step_trace.py names the slots).
 *
 * ---- counters (read-only) since set_option("stat_reset", 0) -------------------
 * "stat_step_calls", "stat_step_items" (FoVs in them), "stat_hist_<n>" (calls with
 *   n FoVs, n = 0..64);
 * "stat_spec_launched" / "stat_spec_hits" / "stat_spec_mismatch" (conv0_a launches
 *   made ahead, steps that ran on one, steps repeated), "stat_spec_miss_full" /
 *   "stat_spec_miss_short" (launches their step did not run on: hint list full /
 *   short);
 * "stat_ahead_used" / "stat_ahead_wasted" / "stat_ahead_aborted" (stacks queued
 *   ahead that their step used / that no step used / that ended after their first
 *   conv); "stat_many_carried" (batched steps left in flight across a return);
 * "stat_segturn_calls", "stat_segturn_queue_ns" / "stat_segturn_wait_ns"
 *   (ffn_canvas_segment_turn on the host, mean per call);
 * "stat_turn_gpu_ns" / "stat_turn_host_ns" / "stat_launch_host_ns" /
 *   "stat_turn_count" (between two single-FoV steps inside a segment, mean: record
 *   published -> first instruction of the next resident launch as the GPU saw it;
 *   record seen -> that launch queued, and the launch call alone, on the host).
 * Not reset: "stat_flow_timeouts" (polls of the resident launch that gave up, ever)
 *   / "stat_flow_voids" (steps voided by one). */

/* With option "debug_clock" = 1 the compact conv kernel records, for its first
 * workgroup, per wave {shader clock at entry, at main-loop start, at main-loop end,
 * at exit, wall clock (100 MHz) at entry, at exit}. */
int ffn_engine_debug_clocks(ffn_engine* engine, long long* out24);
/* With "debug_clock" = 2 every workgroup of the conv32m / conv32mt launch of layer
 * "debug_layer" also records {wall clock (100 MHz) at entry, at exit, HW_ID,
 * XCC_ID}: out[4 b ..] for blockIdx b < max_wgs <= 4096 (zeros for a block that
 * exited at once).  Clears the records. */
int ffn_engine_debug_workgroups(ffn_engine* engine, long long* out, int max_wgs);
/* With "debug_clock" = 4 every workgroup of a FLOW conv (option "flow" 1 or 2: the
 * resident stack of a single-FoV step) records per conv of the stack six wall-clock
 * stamps (100 MHz): body entry, input tiles seen, first segment landed, tap loop
 * over, stores drained, tiles published.  out[(slot * 64 + conv) * 8 + 0..5] for
 * workgroup slot < max_slots (main chunks first, then the tail chunks).  Clears the
 * records. */
int ffn_engine_debug_flow_trace(ffn_engine* engine, long long* out, int max_slots);

#ifdef __cplusplus
}
#endif
#endif /* FFN_HIP_DEBUG_H_ */
