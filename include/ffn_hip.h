/*
 * libffn_hip.so -- C-ABI of the MI355X (gfx950) flood-filling inference engine.
 *
 * This is the drop-in boundary for the ONE hot path this repository replaces:
 * the FFN field-of-view loop of google/ffn.  Every entry point below names the
 * reference interface (file:line, relative to the google/ffn checkout) whose
 * work it takes over.  The reference is pure Python; its FFI for this path is a
 * ctypes binding (see INTEGRATION.md for the stub a maintainer would add to
 * ffn/inference/executor.py).
 *
 * Conventions: plain C types only; every function returns 0 on success or a
 * negative FFN_ERR_* code (no exceptions cross the ABI); the caller owns all
 * host buffers, the library owns all device memory; one HIP stream per engine;
 * calls on one engine (and on canvases created from it) must be serialised by
 * the caller (the executor's server thread); coordinates are (z, y, x).
 */
#ifndef FFN_HIP_H_
#define FFN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFN_OK 0
#define FFN_ERR_ARG (-1)     /* invalid argument / unsupported geometry      */
#define FFN_ERR_HIP (-2)     /* HIP runtime failure (see ffn_last_error)     */
#define FFN_ERR_STATE (-3)   /* call order violated (e.g. weights not set)   */
#define FFN_ERR_RANGE (-4)   /* conv_variant >= 6 only: an operand left the fp16
                                range; the step changed nothing -- switch to
                                conv_variant -1 (exact f32) and repeat it       */

#define FFN_ERR_FLOW (-5)    /* option flow = 2 only: the resident conv launch
                                timed out waiting for one of its own workgroups
                                (a shared or partitioned GPU); the step changed
                                nothing -- repeat it: the repeat runs one launch
                                per conv (same arithmetic), and after 3 such steps
                                in a row the engine sets flow = 0 by itself      */

#define FFN_MAX_CANDIDATES 16

typedef struct ffn_engine ffn_engine;
typedef struct ffn_canvas ffn_canvas;

/* Thresholds of one FoV step, already in logit space, exactly the f32-rounded
 * values Canvas.__init__ stores (ffn/inference/inference.py:189-195). */
typedef struct ffn_step_params {
  float pad_value;             /* NaN -> pad substitution  (inference.py:406-407) */
  float move_threshold;        /* disco mean test + counters (inference.py:429)   */
  float disco_seed_threshold;  /* < 0 disables the disco bias (inference.py:416)  */
  float deleted_threshold;     /* keep_history (inference.py:420-423): count voxels
                                  with old seed >= this and new logit < 0; NaN =
                                  do not count                                    */
} ffn_step_params;

/* One FoV step request (one entry per canvas in a batched call). */
typedef struct ffn_step_request {
  int32_t pos[3];        /* FoV centre (z, y, x)                               */
  int32_t start_pos[3];  /* segment origin: its logit is returned for the
                            "seed got too weak" test (inference.py:503-505)    */
  int32_t num_candidates;                      /* <= FFN_MAX_CANDIDATES        */
  int32_t candidates[FFN_MAX_CANDIDATES][3];   /* queue-head positions whose
                            post-step seed logit / segment id are wanted
                            (Canvas.is_valid_pos, inference.py:325,341)        */
} ffn_step_request;

/* Everything the Python movement policy needs from one FoV step. */
typedef struct ffn_step_result {
  float   face_score[6];  /* max over each face of the +-delta cuboid, order
                             (z-,z+,y-,y+,x-,x+)  (movement.py:67-87)          */
  int32_t face_index[6];  /* first-occurrence C-order argmax inside the face   */
  int32_t face_seg[6];    /* segmentation[] at each face maximum (the validity
                             test of a freshly queued move, inference.py:341)  */
  float   start_logit;    /* seed[start_pos] after the paste                   */
  uint32_t num_above_move;/* #(logits >= move_threshold) before disco          */
  int32_t disco_applied;  /* 1 if the disco mask was applied                   */
  float   cand_seed[FFN_MAX_CANDIDATES];  /* seed[candidate] after the paste   */
  int32_t cand_seg[FFN_MAX_CANDIDATES];   /* segmentation[candidate]           */
  uint32_t num_deleted;   /* history_deleted entry of this step (see
                             ffn_step_params.deleted_threshold), else 0        */
  int32_t range_error;    /* conv_variant >= 6: 1 = an operand left the fp16 range,
                             the step was NOT pasted (FFN_ERR_RANGE); 2 = the
                             step's conv0_a was a launch made ahead for another
                             position (option "speculate"): NOT pasted either,
                             ffn_canvas_step repeats such a step itself; 3 = the
                             resident conv launch gave up waiting for one of its
                             own workgroups: NOT pasted (FFN_ERR_FLOW)          */
} ffn_step_result;

/* Result of the per-segment commit reduction (inference.py:614-646). */
typedef struct ffn_commit_counts {
  int64_t raw_segmented_voxels;     /* sum(seed[sel] >= segment_threshold)      */
  int64_t actual_segmented_voxels;  /* ... and segmentation[sel] <= 0           */
  int32_t num_overlapped_ids;       /* distinct ids > 0 under the raw mask      */
} ffn_commit_counts;

/* Canvas.segment_at as ONE call: the FoV loop of a segment with the default
 * movement policy, run by the library's host code (ffn_canvas_segment_at). */
typedef struct ffn_segment_params {
  ffn_step_params step;       /* thresholds of every FoV step                   */
  double  score_threshold;    /* FaceMaxMovementPolicy.score_threshold
                                 (movement.py:176,214): logit(move_threshold)  */
  int32_t deltas_zyx[3];      /* policy deltas (model_info.deltas[::-1])        */
  int32_t margin_zyx[3];      /* input_image_size // 2 (inference.py:216)       */
  int32_t shape_zyx[3];       /* canvas shape, for the bounds test              */
  int32_t init_min_pos[3];    /* Canvas._min_pos / _max_pos after reset_state   */
  int32_t init_max_pos[3];    /*   (inference.py:288-310)                       */
  float   initial_start_logit;/* seed[start] if known (init_seed), else NaN     */
  int32_t prefetch;           /* queue-head candidates sent with a step (<= 16) */
  int32_t keep_history;       /* record positions (+ deleted counts)            */
  int64_t max_steps;          /* > 0: return after this many steps (resumable)  */
} ffn_segment_params;

typedef struct ffn_segment_result {
  int64_t num_steps;          /* FoV steps made by this call                    */
  int64_t skip_threshold;     /* counters of Canvas.is_valid_pos                */
  int64_t skip_invalid_pos;
  int64_t gate_rejects;       /* in-bounds entries refused on device state      */
  int64_t queue_len;          /* entries left in the policy queue               */
  int32_t seed_got_too_weak;  /* loop left through inference.py:503-505         */
  int32_t budget_exhausted;   /* max_steps reached; call again with resume = 1  */
  int32_t active;             /* the segment can be resumed                     */
  int32_t start_logit_known;
  float   start_logit;        /* seed[start] after the last step                */
  int32_t min_pos[3];         /* extents of the visited positions               */
  int32_t max_pos[3];
} ffn_segment_result;

/* ---- lifecycle -----------------------------------------------------------
 * Replaces model construction in Runner._init_tf_model
 * (ffn/inference/runner.py:116-163) and ConvStack3DFFNModel.__init__ /
 * define_tf_graph (ffn/training/models/convstack_3d.py:68-95).
 * features must be 32 (the MFMA kernel's N); depth >= 1; fov odd per axis. */
int ffn_engine_create(int device_id, const int32_t fov_zyx[3],
                      const int32_t deltas_zyx[3], int depth, int features,
                      int max_batch, ffn_engine** out);
void ffn_engine_destroy(ffn_engine* engine);

/* Replaces tf.train.Saver().restore (runner.py:98-111).  `blob` holds the TF
 * variables in graph order, each tensor exactly as TensorFlow stores it:
 *   conv0_a W[3][3][3][2][F] b[F], conv0_b W[3][3][3][F][F] b[F],
 *   conv{i}_a W b, conv{i}_b W b  (i = 1..depth-1), conv_lom W[F] b[1].
 * Cost: the repack and upload, plus -- where the resident launch is in use and
 * "flow_pace" is at its default (ffn_hip_debug.h) -- a measurement of that
 * launch's beat, ~0.3 s once per (device, depth, FoV) and process.           */
int ffn_engine_set_weights(ffn_engine* engine, const float* blob, size_t count);
size_t ffn_engine_weight_count(int depth, int features);

/* ---- stateless step == ExecutorClient.predict ----------------------------
 * Replaces BatchExecutor._schedule_batch -> session.run
 * (ffn/inference/executor.py:313-340): logits = seed + conv_stack(image,seed).
 * seed, image, logits_out: host arrays [n][fz][fy][fx] f32, n <= max_batch.   */
int ffn_predict(ffn_engine* engine, int n, const float* seed,
                const float* image, float* logits_out);
/* The same step on DEVICE arrays of the engine's device (same layout, same
 * kernels, same bits): for a caller whose FoVs are already resident, e.g. the
 * training-example loop of ffn_evaluation.h.  Whatever wrote seed_dev and
 * image_dev has completed before the call; the call returns with logits_dev
 * written.  logits_dev may be seed_dev or image_dev.                          */
int ffn_predict_device(ffn_engine* engine, int n, const float* seed_dev,
                       const float* image_dev, float* logits_dev);

/* Conv stack only, on whatever FoVs are resident in the engine's staging
 * buffers (no host traffic) -- the kernel-only leg of bench.py. */
int ffn_forward_resident(ffn_engine* engine, int n, int repeats);

/* ---- device-resident canvas ---------------------------------------------
 * Replaces the numpy state of Canvas (inference.py:224-232): image f32
 * (already normalised as runner.py:383-385), seed f32 (NaN = unvisited),
 * segmentation i32, all kept in HBM for the whole subvolume. */
int ffn_canvas_create(ffn_engine* engine, const float* image_f32,
                      const int32_t shape_zyx[3], ffn_canvas** out);
/* The same from the RAW uint8 image: Runner.make_canvas' normalisation
 * (image.astype(np.float32) - image_mean) / image_stddev (runner.py:383-385)
 * moves into the FoV gather of the first conv (a 256-entry table made with the
 * same two f32 operations), the image stays 1 byte per voxel in HBM (1024^3:
 * 1.07 GB instead of 4.29 GB) and no normalised f32 copy is made on the host.
 * Every result is bit-identical to ffn_canvas_create on the normalised image. */
int ffn_canvas_create_u8(ffn_engine* engine, const uint8_t* image_u8,
                         const int32_t shape_zyx[3], float image_mean,
                         float image_stddev, ffn_canvas** out);
void ffn_canvas_destroy(ffn_canvas* canvas);

/* Canvas.init_seed (inference.py:443-450): seed[:] = NaN; seed[pos] = value. */
int ffn_canvas_init_seed(ffn_canvas* canvas, const int32_t pos[3], float value);

/* Canvas.update_at + FaceMaxMovementPolicy scoring for n canvases at once
 * (inference.py:386-441, movement.py:42-100): gather -> conv stack -> disco ->
 * paste-back -> 6-face argmax, entirely on the GPU. */
int ffn_canvas_step(ffn_engine* engine, int n, ffn_canvas* const* canvases,
                    const ffn_step_request* requests,
                    const ffn_step_params* params, ffn_step_result* results);

/* The same step split in two, so that the host work of one group of canvases
 * (queue bookkeeping in Python) overlaps the GPU work of another: submit
 * enqueues the whole step and returns at once; wait blocks until its results
 * are in host memory.  At most two steps may be in flight per engine and a
 * canvas may be in only one of them; steps execute in submission order.
 * ffn_canvas_step == submit + wait.  Other calls on the engine's canvases are
 * ordered behind the steps in flight (same stream). */
int ffn_canvas_step_submit(ffn_engine* engine, int n,
                           ffn_canvas* const* canvases,
                           const ffn_step_request* requests,
                           const ffn_step_params* params, uint32_t* ticket);
int ffn_canvas_step_wait(ffn_engine* engine, uint32_t ticket,
                         ffn_step_result* results);

/* Canvas.segment_at (inference.py:460-533) with FaceMaxMovementPolicy
 * (movement.py:166-222) and Canvas.is_valid_pos (inference.py:312-346), looped
 * inside the library: pop a position, test it, one ffn_canvas_step, queue the
 * face maxima -- until the queue is empty, the start logit falls below
 * move_threshold, or max_steps.  The seed must have been initialised
 * (ffn_canvas_init_seed) by the caller.  resume = 1 continues a segment that
 * returned with budget_exhausted or with an error (e.g. FFN_ERR_RANGE: switch
 * conv_variant and resume; the voided step is repeated).  The visited positions
 * are those of the Python loop, step for step. */
int ffn_canvas_segment_at(ffn_canvas* canvas, const int32_t start_zyx[3],
                          const ffn_segment_params* params, int resume,
                          ffn_segment_result* result);
/* Config C3 in the library (the reference's client threads + batching server
 * thread, ffn/inference/executor.py:266-340, with the per-canvas policy queues
 * here): the ffn_canvas_segment_at loops of n canvases of one engine advanced
 * TOGETHER, one batched ffn_canvas_step per round over the loops still running.
 * Returns as soon as at least one loop has ended (queue empty, seed too weak, or
 * its max_steps spent in this call): finished[k] = 1 marks it, and the caller
 * finishes that segment and gives the canvas its next one (resume[k] = 0); the
 * others continue with resume[k] = 1, in the next call or a later one.
 * results[k] counts from the START of canvas k's segment over all its calls
 * (budget_exhausted aside).  n <= max_batch, canvases distinct, every
 * params[k].step identical (one engine call = one set of step parameters).  On
 * an error (e.g. FFN_ERR_RANGE) nothing of the failed round was pasted and
 * every prepared position stays pending: deal with it, then call again with
 * resume = 1 for every canvas. */
int ffn_canvas_segment_many(ffn_engine* engine, int n, ffn_canvas* const* canvases,
                            const int32_t (*starts_zyx)[3],
                            const ffn_segment_params* params,
                            const int32_t* resume, ffn_segment_result* results,
                            int32_t* finished);

/* ... with the others' next step left IN FLIGHT when a loop ends (carry != 0):
 * the call queues the batched step the still-running loops have prepared and
 * returns without waiting for it, so that the caller's between-segment work on
 * the canvas that ended (ffn_canvas_segment_turn, its bookkeeping, the next
 * call's arguments) runs under that step instead of in front of it -- what a
 * second group of canvases on a second host thread otherwise provides
 * (executor.py:266-340: the reference's client threads).  The next
 * ffn_canvas_segment_many[_carry] call on the engine waits for the step first and
 * feeds its results to the loops it was made for; so does any entry point that
 * needs one of those canvases' loops earlier (ffn_canvas_segment_at,
 * ffn_canvas_segment_history, ffn_canvas_destroy).  results[k].num_steps counts
 * a carried step once its results are in.  One carried step per engine: meant
 * for ONE driving thread; max_steps budgets are per call and do not see the
 * carried step (callers with budgets pass carry = 0).  carry = 0:
 * ffn_canvas_segment_many. */
int ffn_canvas_segment_many_carry(ffn_engine* engine, int n,
                                  ffn_canvas* const* canvases,
                                  const int32_t (*starts_zyx)[3],
                                  const ffn_segment_params* params,
                                  const int32_t* resume,
                                  ffn_segment_result* results, int32_t* finished,
                                  int32_t carry);
/* keep_history: entries [first, first + n) of the current segment's history
 * (positions zyx, deleted-voxel counts); *total = entries recorded. */
int ffn_canvas_segment_history(ffn_canvas* canvas, size_t first, size_t n,
                               int32_t* pos_zyx, uint32_t* deleted,
                               size_t* total);

/* Point reads used by Canvas.is_valid_pos (inference.py:312-346). */
int ffn_canvas_read_points(ffn_canvas* canvas, int n, const int32_t* pos_zyx,
                           float* seed_out, int32_t* seg_out);
/* segmentation[pos] = value (the -1 "excluded" markers, inference.py:579,604). */
int ffn_canvas_write_seg_points(ffn_canvas* canvas, int n,
                                const int32_t* pos_zyx, const int32_t* values);
/* np.any(segmentation[lo:hi] > 0) -- min_boundary_dist test (inference.py:573-581). */
int ffn_canvas_any_segmented(ffn_canvas* canvas, const int32_t lo[3],
                             const int32_t hi[3], int32_t* out);

/* Segment commit (inference.py:614-646), in two calls so Python keeps the
 * accept/reject decision: count, then (if accepted) assign `segment_id`.
 * overlap_ids/overlap_counts receive up to `max_overlaps` (id, count) pairs in
 * ascending id order (np.unique semantics, ids > 0 only). */
int ffn_canvas_commit_count(ffn_canvas* canvas, const int32_t lo[3],
                            const int32_t hi[3], float segment_threshold,
                            int32_t max_existing_id, ffn_commit_counts* counts,
                            int32_t max_overlaps, int32_t* overlap_ids,
                            int64_t* overlap_counts);
int ffn_canvas_commit_assign(ffn_canvas* canvas, const int32_t lo[3],
                             const int32_t hi[3], float segment_threshold,
                             int32_t segment_id);

/* The between-segment turn of Canvas.segment_all (inference.py:573-660) as one
 * device-side sequence (at most five kernel launches, no copy operation).  Its last
 * kernel publishes the answers into pinned host memory and the call polls for them
 * there, once, instead of waiting on the stream after every question:
 *   1. do_commit: the commit reduction over [lo, hi) (ffn_canvas_commit_count);
 *      if actual_segmented_voxels >= min_segment_size the voxels get segment_id
 *      (inference.py:614-646) and *committed = 1;
 *   2. mark_mode 1: segmentation[mark_pos] = -1 if it is 0 ("weak seed",
 *      inference.py:600-603); 2: the same when step 1 did not commit ("too
 *      small", inference.py:632-636); 0: no marker;
 *   3. the next seeds of the policy, `candidates` in its order (all inside the
 *      canvas): a candidate whose segmentation is > 0 is skipped
 *      (Canvas.is_valid_pos, inference.py:341), one with an id > 0 within
 *      min_boundary_dist (clipped box, inference.py:575-581) is marked -1 and
 *      skipped; the first one that passes is *chosen* (-1: none of them);
 *   4. do_init: Canvas.init_seed(candidates[chosen], init_value)
 *      (inference.py:282-286) when there is one.
 * cand_flags[k]: 0 passed (k = chosen), 1 already segmented, 2 too close (marked),
 * 3 after the chosen one (untouched), 4 vetoed by the canvas' restrictor
 * (ffn_canvas_set_restrictor, not marked); cand_seed / cand_seg: the canvas
 * values at candidate k as step 3 saw them. */
typedef struct ffn_turn_request {
  int32_t do_commit;
  int32_t lo[3], hi[3];
  float   segment_threshold;
  int64_t min_segment_size;
  int32_t segment_id;
  int32_t max_existing_id;
  int32_t mark_mode;
  int32_t mark_pos[3];
  int32_t num_candidates;
  int32_t min_boundary_dist[3];   /* zyx */
  int32_t do_init;
  float   init_value;
} ffn_turn_request;

typedef struct ffn_turn_result {
  ffn_commit_counts counts;       /* zero without do_commit                     */
  int32_t committed;
  int32_t chosen;
} ffn_turn_result;

int ffn_canvas_segment_turn(ffn_canvas* canvas, const ffn_turn_request* request,
                            const int32_t* candidates /* [num_candidates][3] */,
                            ffn_turn_result* result, int32_t max_overlaps,
                            int32_t* overlap_ids, int64_t* overlap_counts,
                            int32_t* cand_flags, float* cand_seed,
                            int32_t* cand_seg);

/* The SEED loop of Canvas.segment_all (inference.py:573-660) inside the library:
 * turn, segment, turn, ... over a list of seeds, with no caller between two
 * segments.  One turn tests the next `turn_candidates` seeds of the list (the
 * window ends in front of a seed whose FoV leaves the canvas, or one it already
 * holds) and initialises the first that passes; ffn_canvas_segment_at runs from
 * it; the weak-seed test (start logit < step.move_threshold, inference.py:600)
 * and the commit box (visited extents +- half_pred, clipped) follow; the NEXT
 * turn commits or marks and tests the following seeds in the same device
 * sequence.  Decisions, device calls and their order are those of
 * DeviceCanvas._turn / _segment_at_native / _commit.
 *
 * A call ends when the list does, or at the first segment boundary at which
 * max_segments attempts have been made, max_ms have passed or the deadline has
 * (never before one attempt, so every call makes progress).  At every FFN_OK
 * return the canvas is BETWEEN TWO SEEDS: the last attempted segment is
 * committed or marked (the last turn of such a call has no candidates), no seed
 * is initialised and none tested ahead -- seeds[0 .. next_seed) are dealt with,
 * the others untouched.  On an error inside a segment (FFN_ERR_RANGE,
 * FFN_ERR_FLOW: ffn_canvas_segment_at) the call returns it with the records
 * made so far and in_segment = 1: deal with it and call again with resume = 1
 * (first_seed = the next_seed returned); that segment's record then comes
 * first and counts every step once. */
#define FFN_SEED_NO_STEPS  0   /* the loop made no step ("num iters was 0")      */
#define FFN_SEED_WEAK      1   /* start logit below move_threshold: marked -1    */
#define FFN_SEED_TOO_SMALL 2   /* < min_segment_size voxels: marked -1           */
#define FFN_SEED_COMMITTED 3   /* voxels assigned segment_id                     */

typedef struct ffn_seed_record {   /* one segment ATTEMPTED                      */
  int32_t pos[3];                  /* its seed                                   */
  int32_t outcome;                 /* FFN_SEED_*                                 */
  int32_t segment_id;              /* committed: its id, else 0                  */
  int32_t num_overlaps;            /* (id, count) pairs of this record, at       */
  int64_t first_overlap;           /*   overlap_ids / _counts[first_overlap ..)  */
  int64_t raw_segmented_voxels;    /* ffn_commit_counts of its commit (0 when    */
  int64_t actual_segmented_voxels; /*   none was tried)                          */
  double  seconds;                 /* wall clock of the attempt, init to loop end */
  ffn_segment_result segment;      /* the loop's tallies, over all its legs      */
} ffn_seed_record;

typedef struct ffn_seed_loop_args {
  const int32_t* seeds;            /* [num_seeds][3] zyx, the policy's list      */
  int64_t num_seeds;
  int64_t first_seed;              /* index to start at                          */
  ffn_segment_params segment;      /* max_steps = 0; init_* and initial_start_logit
                                      are set per segment by the loop            */
  int32_t min_boundary_dist[3];    /* the turn's constants (ffn_turn_request)    */
  float   init_value;              /* init_activation                            */
  float   segment_threshold;
  int32_t half_pred[3];            /* pred_size // 2 (inference.py:608)          */
  int64_t min_segment_size;
  int32_t next_segment_id;         /* id of the next commit; then + 1            */
  int32_t max_existing_id;         /* largest id in the canvas                   */
  int32_t turn_candidates;         /* seeds tested per turn, >= 1                */
  int32_t resume;                  /* 1: finish the segment an error interrupted */
  int32_t max_segments;            /* budget of this call; <= 0: none            */
  int32_t has_deadline;            /* deadline_s is set                          */
  double  max_ms;                  /* <= 0: none                                 */
  double  deadline_s;              /* seconds from the call's start              */
  int32_t max_records;             /* capacity of records (>= 1)                 */
  int32_t reserved;
  ffn_seed_record* records;
  int64_t max_overlaps;            /* capacity of the two arrays below, at least
                                      max_existing_id + 1                        */
  int32_t* overlap_ids;
  int64_t* overlap_counts;
} ffn_seed_loop_args;

typedef struct ffn_seed_loop_result {
  int64_t next_seed;               /* seeds[0 .. next_seed) are consumed         */
  int64_t num_overlaps;            /* pairs written                              */
  int64_t rejected_invalid;        /* seeds refused: FoV outside / segmented,    */
  int64_t rejected_segmented;      /*   of them already segmented (gate rejects) */
  int64_t rejected_restricted;     /*   vetoed by the restrictor,                */
  int64_t rejected_too_close;      /*   within min_boundary_dist (marked -1)     */
  int64_t restricted_skips;        /* ffn_canvas_take_restricted_skips, taken    */
  double  seconds;                 /* wall clock of the call                     */
  int32_t num_records;
  int32_t turns;                   /* turns made                                 */
  int32_t exhausted;               /* the list has ended                         */
  int32_t in_segment;              /* an error left a segment to resume          */
} ffn_seed_loop_result;

int ffn_canvas_segment_all(ffn_canvas* canvas, const ffn_seed_loop_args* args,
                           ffn_seed_loop_result* result);

/* MovementRestrictor (movement.py:247-336) on the canvas.  Two bits per voxel p:
 *   pos_blocked(p)  = mask[p] != 0, or any non-zero voxel of shift_mask (the
 *                     REDUCED, thresholded mask, [Zs][Ys][Xs]) in the box
 *                     z: max(z+pre[0], 0) .. min(z+post[0], Zs-1)   (unscaled),
 *                     y: max(y+pre[1], 0) // scale .. min((y+post[1]) // scale, Ys-1),
 *                     x: the same with pre[2] / post[2] / Xs
 *                     (// = floor division; an empty range: not blocked);
 *   seed_blocked(p) = seed_mask[p] != 0.
 * pre / post (zyx) are the restrictor's shift-mask FoV start and end - 1; post
 * must be >= -1 on every axis.  mask / seed_mask are uint8 volumes of the canvas
 * shape, any of the three may be NULL; all three NULL clears the restrictor.  The
 * arrays are read during the call (a snapshot: later edits of the caller's copy
 * are not seen).  The device keeps both bits as planes of 64 voxels per word
 * along x (<= 2 bits / voxel), the host loop a copy of pos_blocked (1 bit).
 * With a restrictor
 *   - the segment loop (ffn_canvas_segment_at / _segment_many) skips a popped
 *     position that is pos_blocked after the seed-too-weak test, without marking
 *     it visited (inference.py:506-508), and tallies it (below); its hints to the
 *     device leave such positions out;
 *   - ffn_canvas_segment_turn flags a candidate that is not segmented but
 *     pos_blocked or seed_blocked with cand_flags 4 (restricted): skipped, no
 *     -1 marker (inference.py:573-574 come before the too-close test). */
int ffn_canvas_set_restrictor(ffn_canvas* canvas, const uint8_t* mask,
                              const uint8_t* seed_mask, const uint8_t* shift_mask,
                              const int32_t shift_shape[3], const int32_t pre[3],
                              const int32_t post[3], int32_t scale);
/* dst[hi-lo] (C order, uint8): bit 0 pos_blocked, bit 1 seed_blocked; all zero
 * without a restrictor.  The box must lie inside the canvas. */
int ffn_canvas_read_restriction(ffn_canvas* canvas, const int32_t lo[3],
                                const int32_t hi[3], uint8_t* dst);
/* The segment loops' count of positions skipped for pos_blocked
 * ("skip_restriced_pos") since the last call; reads and zeroes it. */
int ffn_canvas_take_restricted_skips(ffn_canvas* canvas, int64_t* count);

/* Box transfers between the canvas and host arrays ([hi-lo] C-order):
 * checkpoint/restore and final save (inference.py:728-821, runner.py:433-482). */
int ffn_canvas_read_seed(ffn_canvas* canvas, const int32_t lo[3],
                         const int32_t hi[3], float* dst);
int ffn_canvas_read_segmentation(ffn_canvas* canvas, const int32_t lo[3],
                                 const int32_t hi[3], int32_t* dst);
int ffn_canvas_write_seed(ffn_canvas* canvas, const int32_t lo[3],
                          const int32_t hi[3], const float* src);
int ffn_canvas_write_segmentation(ffn_canvas* canvas, const int32_t lo[3],
                                  const int32_t hi[3], const int32_t* src);

/* ---- measurement ----------------------------------------------------------
 * HIP-event timing of the dominant kernel (the 32->32 3x3x3 MFMA conv) on the
 * engine's own stream.  mode 0 = off, 1 = one event pair per conv launch,
 * 2 = one event pair around the whole chain of 2*depth-1 conv launches of a
 * step (duration / launches then includes the inter-kernel gaps but not the
 * per-event barrier overhead of mode 1). */
int ffn_engine_set_profiling(ffn_engine* engine, int mode);
int ffn_engine_get_profile(ffn_engine* engine, double* conv_ms_total,
                           int64_t* conv_launches, int reset);
/* The individual event-pair durations (ms) behind ffn_engine_get_profile since
 * its last reset -- one per sampled conv launch (mode 1) or per sampled conv
 * chain of a step (mode 2: 2 depth - 1 launches, or the ONE launch of the
 * resident stack): *n = how many exist, the first min(*n, max_n) are copied. */
int ffn_engine_get_profile_samples(ffn_engine* engine, float* out_ms, int max_n, int* n);
/* A model whose prediction is smaller than the seed it reads (ModelInfo
 * pred_mask_size < input_seed_size; reference ffn/training/model.py:168-183 pads
 * the update with zeros around the centre, ffn/inference/inference.py:218,410-411
 * writes only the centred box): canvas steps (ffn_canvas_step*, segment_at /
 * segment_many) then score the move faces around the CENTRE OF THAT BOX, count
 * logits >= move_threshold and apply the disco bias inside it, and paste only it;
 * ffn_predict still returns the whole FoV (the caller crops).  pred_zyx = the
 * FoV: back to the default.  Deltas must fit the box's half size. */
int ffn_engine_set_pred_size(ffn_engine* engine, const int32_t pred_zyx[3]);
/* ---- options --------------------------------------------------------------
 * The options a user sets; none but "conv_variant" changes a result beyond f32
 * summation order.  The lab's options (pacing, ablation, tracing, "stat_*"
 * counters) and the debug readers are in ffn_hip_debug.h.  An out-of-range value
 * or an unknown name is FFN_ERR_ARG.
 * "conv_variant": the kernel of the 32->32 convs:
 *   0 = simple exact-f32 MFMA conv over padded positions (any FoV that fits the LDS),
 *   2 = exact-f32 MFMA conv over compact chunks, pipelined (bitwise the oracle's
 *       fmaf chain),
 *   6 = conv32d: every f32 product carried as 3 fp16 products (hi + 2^-11 *
 *       residual: 22 mantissa bits, about the rounding noise of an f32 GEMM) on
 *       32x32x16 MFMAs; operands must stay inside the fp16 range, else
 *       FFN_ERR_RANGE,
 *   7 = 6 in 96-voxel chunks (two workgroups per CU; the same bits),
 *   8 = conv32m: the same products, M split over the waves, two workgroups per CU,
 *   9 (default where the FoV has 257 .. 512 chunks of 128 voxels, e.g. 33^3) =
 *       a step of ONE FoV runs conv32mt (conv32m for the first 256 chunks +
 *       32-voxel K-split tail workgroups), a step of several runs conv32m,
 *  10 = a step of ONE FoV on 80-voxel workgroups, two per CU (conv32hs / conv32h;
 *       another summation order than 9, the same tolerance).  Measured SLOWER than
 *       9 at 33^3 (profiles/r06_gate_two_chains.txt): selectable, not a default,
 *  -1 = this FoV's exact-f32 kernel ("exact_variant", read-only: 2 where it fits,
 *       else 0).
 *   (1, 3, 4, 5 were removed in ABI 7; they are in the history up to af82310.)
 * "flow" 0..2: how the 2 depth - 1 convs of a single-FoV step of conv_variant 9
 *   run: 0 = one dependent launch per conv, 1 = the same launches with the flagged
 *   hand-off compiled in, 2 = ONE resident launch whose workgroups hand rows to
 *   each other (conv32ps) -- bit-identical in every mode.  2 is the default where
 *   the device can hold all of the launch's workgroups at once (checked at
 *   ffn_engine_create; else 0, and setting 2 is FFN_ERR_ARG).  A resident launch
 *   that times out voids its step with FFN_ERR_FLOW (see above); after three such
 *   steps in a row the engine sets "flow" = 0 itself ("flow_auto_off", read-only,
 *   reads 1; setting "flow" again re-arms).
 * "batch_chunks" 0..2 (variant 6): the form steps of several FoVs take;
 * "tail_batched" 1 = conv32mt for every step (one arithmetic whatever the batch).
 * "mfma_products" 3 (default) or 1; anything else is FFN_ERR_ARG and stores nothing.
 *   fp16 inference, opt-in: with 1 the 32 -> 32 convs of conv32m / conv32mt compute
 *   sum hi(w) hi(a) in f32 accumulators -- hi() = the operand's fp16 half, i.e. the
 *   f32 value rounded to nearest-even fp16 with |v| < 2^-14 becoming 0 -- and drop the
 *   two cross products that make the default path f32-accurate (one MFMA instead of
 *   three per operand pair, half the LDS fragment reads).  conv0_a, the head, bias, ReLU,
 *   the residual add and the f32 residual stream, gather / faces / paste and the fp16
 *   range guard are unchanged.  It takes effect where a stack runs conv32m or conv32mt
 *   (conv_variant 8 and 9; batched steps of 6 with batch_chunks 2); every other kernel
 *   family -- conv32, conv32c, conv32d in both chunk sizes, conv32h -- ignores it and
 *   computes as always, which is what lets a range-voided step be repeated on the exact
 *   kernel with the option stored.  The one-product kernels exist as per-layer launches
 *   only: a single-FoV step runs conv32mt as under "flow" = 0, never the resident launch.
 *   OUTSIDE the accuracy contract of the default path: the logits differ from f32 by
 *   ~1e-3 .. 1e-2 per step (a thousand times the split kernels' distance), the FoV loop
 *   amplifies that, and whole runs stand to the f32 run at foreground IoU 0.92 .. 0.9999
 *   (250^3 volumes: 0.92 .. 0.93), not >= 0.999.  It pays for
 *   batched steps (0.71 of the time per conv); a single FoV is 10 % slower with it.  Same trade as the reference's half-precision
 *   inference: throughput for a slightly higher merge error rate; the user's choice.
 * "speculate" (default 1): single-FoV steps of the segment loop queue conv0_a of the
 *   NEXT step behind their paste, for the positions the loop expects to pop next; a
 *   step whose launch chose another position pastes nothing and is made again.
 * "stack_ahead" (default 1): ... and that step's resident conv stack right behind
 *   it, before the host has seen this step's record.
 * "fuse_paste" (default 1): faces and paste of a single-FoV step as one launch;
 * "fuse_conv0a" (default 1): the next step's conv0_a in it as well; "fuse_head"
 *   (variant 2): the 1x1x1 head inside the last conv launch.
 * "store_policy" 0..2 (variant 2): write-back, write-through, non-temporal stores.
 * "sync_mode": 1 (default) = a step's wait polls its record in pinned memory,
 *   0 = it blocks on the stream.  "profile_every" N >= 1: the profiler samples one
 *   of every N conv stacks. */
int ffn_engine_set_option(ffn_engine* engine, const char* name, int value);
/* Current value of an option that set_option takes, or of a read-only one. */
int ffn_engine_get_option(ffn_engine* engine, const char* name, int* value);
/* Blocks until all work queued on the engine's stream has finished. */
int ffn_engine_synchronize(ffn_engine* engine);

/* Thread-local description of the last error. */
const char* ffn_last_error(void);
/* ABI version of this header. */
int ffn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FFN_HIP_H_ */
