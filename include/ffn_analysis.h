/*
 * libffn_hip.so, resegmentation analysis -- the per-voxel work of the
 * reference's ffn/inference/resegmentation_analysis.py on the GPU.
 *
 * A resegmentation request leaves one .npz per decision point; evaluating a
 * pair costs the reference four scipy distance transforms over the analysis
 * box plus a dozen full-box reductions (resegmentation_analysis.py:52-86,
 * :225-258), an endpoint one overlap table against the base segmentation
 * (:136-154).  Both are BATCHED here: one call takes n points whose boxes may
 * differ in shape, because a single box is far too small to fill the device.
 *
 * Probabilities never meet float arithmetic on the device: the caller hands in
 * a 256-entry byte table that says which quantised values are "object"
 * (dequantize -> nan_to_num -> >= threshold, computed with numpy), so the masks
 * are numpy's own comparison whatever its promotion rules are.
 *
 * Conventions as in ffn_hip.h / ffn_seeds.h: opaque handle with its own stream
 * and grow-only device scratch, 0 or a negative FFN_ERR_* code, coordinates
 * are (z, y, x), all pointers are host pointers.
 */
#ifndef FFN_ANALYSIS_H_
#define FFN_ANALYSIS_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffn_analyzer ffn_analyzer;

int ffn_analyzer_create(int device_id, ffn_analyzer** out);
void ffn_analyzer_destroy(ffn_analyzer* a);

/* One pair point.  probs: u8 [2, box_zyx] quantised object maps of the two
 * re-grown objects over the resegmentation box; the analysis crop is
 * [off_zyx, off_zyx + shape_zyx) inside it; seg: u64 [shape_zyx], the base
 * segmentation over the analysis crop. */
typedef struct ffn_pair_desc {
  const uint8_t* probs;
  const uint64_t* seg;
  uint64_t id_a, id_b;
  int32_t box_zyx[3];
  int32_t off_zyx[3];
  int32_t shape_zyx[3];
  int32_t reserved;
} ffn_pair_desc;

#define FFN_PAIR_COUNTS 10

/* Per point, with A = table[probs[0]], B = table[probs[1]], S1 = seg == id_a,
 * S2 = seg == id_b over the analysis crop:
 *   counts[10 * i + k], k = 0..9:
 *     |A| |B| |A&B| |A|B| |S1| |S2| |A&S1| |A&S2| |B&S1| |B&S2|   (exact)
 *   max_edt[4 * i + m], m = 0..3 for A, B, S1, S2: the maximum over the crop of
 *     the exact Euclidean distance to the nearest voxel where the mask is 0,
 *     in units of voxel_size_zyx -- max(ffn_seeder_edt(mask)): 0 for an empty
 *     mask, +inf for a mask without a 0 voxel.  Squared distances are summed
 *     x, then y, then z in f64 without contraction (exact for integer voxel
 *     sizes) and the root is taken once, of the maximum.
 * Every axis of a crop is 1..4096 voxels, a crop has < 2^31 voxels.  Points
 * are processed in groups that fit a fixed scratch budget; the call returns
 * when all are done. */
int ffn_analyzer_pair_stats(ffn_analyzer* a, const ffn_pair_desc* points,
                            size_t n, const uint8_t table[256],
                            const double voxel_size_zyx[3], uint64_t* counts,
                            double* max_edt);

/* One endpoint point.  probs: u8 [shape_zyx], the quantised object map; seg:
 * u64 [shape_zyx], the base segmentation over the same box.  has_id != 0: the
 * row of `id` (the seeding segment) is wanted even if nothing overlaps it. */
typedef struct ffn_endpoint_desc {
  const uint8_t* probs;
  const uint64_t* seg;
  uint64_t id;
  int32_t shape_zyx[3];
  int32_t has_id;
} ffn_endpoint_desc;

/* Overlap table of every point against its base segmentation, with
 * new = table[probs]: num_new[i] = |new| of point i, and one row per (point,
 * old id) with at least one voxel where seg == old and new is set -- old = 0
 * included -- and, with has_id, for `id` if it occurs in seg at all:
 *   row_point[r], row_old[r], row_counts[2 * r + 0] = overlapping voxels,
 *   row_counts[2 * r + 1] = voxels with seg == old.
 * Rows come in UNSPECIFIED order.  At most `cap` rows are written; *n_rows is
 * the true count, and the call fails with FFN_ERR_ARG if it exceeds cap (grow
 * the buffers and repeat).  An id of 2^64 - 1 is refused. */
int ffn_analyzer_endpoint_overlaps(ffn_analyzer* a,
                                   const ffn_endpoint_desc* points, size_t n,
                                   const uint8_t table[256], size_t cap,
                                   int32_t* row_point, uint64_t* row_old,
                                   uint32_t* row_counts, uint64_t* num_new,
                                   size_t* n_rows);

/* HIP-event kernel time (uploads excluded) and voxels of the last pair_stats
 * [0] and endpoint_overlaps [1] call, summed over its groups. */
int ffn_analyzer_last_timing(ffn_analyzer* a, double kernel_ms[2],
                             double voxels[2]);

#ifdef __cplusplus
}
#endif
#endif /* FFN_ANALYSIS_H_ */
