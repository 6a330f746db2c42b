/*
 * libffn_hip.so, segmentation metrics -- the integer side of scoring a
 * segmentation against ground truth (doc/manual.md of the reference: "evaluate
 * the resulting segmentations using metrics of interest ... we recommend
 * skeleton metrics"; the reference ships no code for it).  Two calls:
 *
 *   ffn_metrics_contingency
 *       the joint histogram n_ij of (ground-truth id, segment id) over a
 *       volume or a core box of it: what Rand scores, variation of information
 *       and per-object overlap tables are sums over.
 *   ffn_metrics_skeleton
 *       ground-truth skeleton edges classified as omitted / merged / split /
 *       correct against a segmentation, and the summed length of the correct
 *       edges per (skeleton, segment): what edge accuracies and the expected
 *       run length are ratios of.
 *
 * Everything computed on the device is an integer (u64 atomics); the floats are
 * derived from these tables on the host (ffn_amd/metrics.py), so results are
 * bit-reproducible from run to run.
 *
 * Conventions as in ffn_labels.h: plain C types, 0 / negative FFN_ERR_* return
 * codes, ffn_last_error() for the message, caller owns host buffers.  A label
 * volume is a flat C-order zyx array of `elem_bytes` = 4 (uint32 / int32 bit
 * pattern) or 8 (uint64) bytes per voxel, each volume with a width of its own.
 * It is either HOST memory (`on_device` = 0: uploaded whole by the call) or a
 * DEVICE pointer on the handle's device (`on_device` = 1, e.g. the data_ptr of
 * a tensor filled by ffn_labels_copy_canvas or by the device assembly: no
 * voxel goes through the host); the caller synchronises whatever produced a
 * device volume.  Every id must be < 2^32 - 1 (FFN_ERR_ARG otherwise: remap
 * wider ids, and clear a canvas' -1 markers, first).  A box is half-open
 * [lo, hi) zyx inside the volume (FFN_ERR_ARG if not); lo = hi = NULL is the
 * whole volume.  A handle owns one HIP stream and grow-only device scratch;
 * calls on one handle must be serialised.
 */
#ifndef FFN_METRICS_H_
#define FFN_METRICS_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffn_metrics ffn_metrics;

int ffn_metrics_create(int device_id, ffn_metrics** out);
void ffn_metrics_destroy(ffn_metrics* h);

/* Joint histogram of (gt[v], seg[v]) over the voxels v of the box.  With
 * ignore_gt_zero, voxels whose ground truth is 0 count nowhere.  Writes up to
 * `cap` unique pairs in UNSPECIFIED order (the caller sorts); *n_pairs is the
 * true number of unique pairs (FFN_ERR_ARG if > cap).  Tables of sub-boxes
 * whose boxes tile a volume add up to the table of the volume. */
int ffn_metrics_contingency(ffn_metrics* h, const void* gt, int gt_elem_bytes,
                            int gt_on_device, const void* seg,
                            int seg_elem_bytes, int seg_on_device,
                            const int64_t shape_zyx[3], const int64_t box_lo[3],
                            const int64_t box_hi[3], int ignore_gt_zero,
                            size_t cap, uint64_t* pair_gt, uint64_t* pair_seg,
                            uint64_t* pair_count, size_t* n_pairs);

/* ffn_metrics_skeleton: class of an edge (edge_class[e], class_count[c],
 * class_len[c]). */
enum {
  FFN_EDGE_OMITTED = 0,
  FFN_EDGE_MERGED = 1,
  FFN_EDGE_SPLIT = 2,
  FFN_EDGE_CORRECT = 3,
  FFN_EDGE_CLASSES = 4
};

/* Skeleton edges against a segmentation.  Nodes: nodes_zyx[n][3] (int32 voxel
 * coordinates) and node_skeleton[n] (non-zero id of the skeleton the node
 * belongs to, < 2^32 - 1).  Edges: edges[e][2] (node indices; both ends in one
 * skeleton) and edge_len_q[e], the physical length of the edge in fixed point
 * (1/1024 units; computed by the caller, independent of the segmentation).
 * Anything else is FFN_ERR_ARG.
 *
 *   node_seg[k] = seg[node k], 0 if the node lies outside the box.
 *   A MERGER is a segment != 0 in which at least two skeletons have
 *   >= merge_min_nodes (>= 1) nodes each.
 *   An edge is, by the first rule that applies: OMITTED if either end's
 *   segment is 0, MERGED if either end's segment is a merger, SPLIT if the two
 *   segments differ, CORRECT otherwise.
 *   The RUN of (skeleton, segment) is the summed edge_len_q of the skeleton's
 *   correct edges inside the segment (contiguous along the skeleton or not).
 *
 * class_count / class_len: edges and summed edge_len_q per class.  Runs: up to
 * `run_cap` triples, mergers: up to `merger_cap` ids, both in UNSPECIFIED
 * order with the true numbers in *n_runs / *n_mergers (FFN_ERR_ARG if either
 * exceeds its cap).  node_seg (n_nodes) and edge_class (n_edges) are optional
 * (NULL to skip). */
int ffn_metrics_skeleton(ffn_metrics* h, const void* seg, int seg_elem_bytes,
                         int seg_on_device, const int64_t shape_zyx[3],
                         const int64_t box_lo[3], const int64_t box_hi[3],
                         size_t n_nodes, const int32_t* nodes_zyx,
                         const uint32_t* node_skeleton, size_t n_edges,
                         const int32_t* edges, const uint32_t* edge_len_q,
                         uint64_t merge_min_nodes,
                         uint64_t class_count[FFN_EDGE_CLASSES],
                         uint64_t class_len[FFN_EDGE_CLASSES], size_t run_cap,
                         uint64_t* run_skeleton, uint64_t* run_segment,
                         uint64_t* run_len, size_t* n_runs, size_t merger_cap,
                         uint64_t* merger_ids, size_t* n_mergers,
                         uint32_t* node_seg, uint8_t* edge_class);

/* HIP-event time of the kernels (no host<->device copies) of the last call on
 * this handle, and the HBM bytes they are specified to move (algorithmic):
 * contingency: voxels of the box x the two element widths. */
int ffn_metrics_last_timing(ffn_metrics* h, double* kernel_ms,
                            double* algorithmic_bytes);

#ifdef __cplusplus
}
#endif
#endif /* FFN_METRICS_H_ */
