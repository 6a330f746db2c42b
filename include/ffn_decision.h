/*
 * libffn_hip.so, agglomeration decision points -- the step between an assembled
 * segmentation and a ResegmentationRequest: expand every segment into the
 * unlabelled gaps by a Euclidean feature transform, find where two expanded
 * segments touch, and keep per pair of ids the contacts of least distance
 * (the job of find_decision_points in ffn/utils/decision_point.py of the
 * google/ffn checkout; the last choice among equal minima is made on the host,
 * ffn_amd/utils/decision_point.py).
 *
 * Conventions as in ffn_labels.h: plain C types, 0 / negative FFN_ERR_* return
 * codes, ffn_last_error() for the message, (z, y, x) order, the caller owns
 * host buffers.  A handle owns one HIP stream and grow-only device scratch;
 * calls on one handle must be serialised.  Every call returns with its kernels
 * complete.
 *
 * Nearest-segment expansion, exact definition.  voxel_size_xyz is the physical
 * voxel size in x, y, z order (the order of the reference's docstring;
 * `connectomics.segmentation.labels.watershed_expand` itself is not available
 * to this project, so the order is taken from the docstrings); the sampling
 * along the array axes z, y, x is therefore its reverse.
 *   d2(v, u) = ((dx * sx)^2 + (dy * sy)^2) + (dz * sz)^2   in f64:
 * each term is the product delta * s multiplied by itself, the terms are added
 * in that order, nothing is contracted into an FMA.
 *   unlabelled v: edt[v] = sqrt(min over labelled u of d2(v, u)), correctly
 *     rounded; expanded[v] = the SMALLEST id among the labelled voxels at
 *     exactly that minimum d2;
 *   labelled v: its own id, edt 0;
 *   no labelled voxel at all: edt +inf, expanded 0 everywhere;
 *   max_distance >= 0: expanded[v] = 0 where edt[v] > max_distance (edt is not
 *     clipped); max_distance < 0 or NaN: unlimited.
 * When the voxel sizes are integer-valued every d2 is an exact integer in f64
 * and the result is exact and bit-reproducible.  For other voxel sizes the
 * minimum is taken over the rounded partial sums of the three separable
 * passes: "nearest up to f64 rounding".
 */
#ifndef FFN_DECISION_H_
#define FFN_DECISION_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffn_decision ffn_decision;

int ffn_decision_create(int device_id, ffn_decision** out);
void ffn_decision_destroy(ffn_decision* h);

/* Expansion of a HOST label volume of elem_bytes 4 (uint32 / int32 bit
 * pattern) or 8 (uint64); 0 is unlabelled, every id must be < 2^32 - 1 (the
 * Python caller remaps larger ids first).  No axis may be longer than 4096 and
 * the volume must hold fewer than 2^31 voxels.  `expanded` and `edt` stay
 * resident on the handle until the next expansion. */
int ffn_decision_expand(ffn_decision* h, const void* seg, int elem_bytes,
                        const int64_t shape_zyx[3],
                        const double voxel_size_xyz[3], double max_distance);

/* The same for int32 labels in DEVICE memory (values <= 0 are unlabelled); the
 * caller synchronises whatever produced them.  The input is only read. */
int ffn_decision_expand_device(ffn_decision* h, const int32_t* seg_dev,
                               const int64_t shape_zyx[3],
                               const double voxel_size_xyz[3],
                               double max_distance);

/* The same for the segmentation of a live device canvas, read in place. */
int ffn_decision_expand_canvas(ffn_decision* h, ffn_canvas* canvas,
                               const double voxel_size_xyz[3],
                               double max_distance, int64_t shape_zyx_out[3]);

/* Copies the resident results to the host; either pointer may be NULL. */
int ffn_decision_read(ffn_decision* h, uint32_t* expanded, double* edt);

/* Contact scan over the resident expansion cropped to [lo_zyx, hi_zyx) (NULL,
 * NULL: the whole volume).  With the 7 offsets (dz, dy, dx) numbered
 *   0 (0,0,-1)  1 (0,-1,0)  2 (0,-1,-1)  3 (-1,0,0)  4 (-1,0,-1)  5 (-1,-1,0)
 *   6 (-1,-1,-1)
 * voxel i of the crop and its neighbour n at the HIGHER index along every axis
 * whose entry is -1 (n inside the crop) form a candidate where a = expanded[i]
 * and b = expanded[n] are both non-zero and differ: pair (min, max), distance
 * (edt[i] + edt[n]) / 2, coordinate i relative to the crop.  Returned are ALL
 * candidates whose distance equals the minimum of their pair, unsorted; a
 * voxel that qualifies under several offsets appears once per offset.
 * off_zyx holds 4 int32 per candidate: offset number, z, y, x.  *n is the true
 * number of such candidates (FFN_ERR_ARG if > cap; nothing past cap is
 * written). */
int ffn_decision_contact_minima(ffn_decision* h, const int64_t lo_zyx[3],
                                const int64_t hi_zyx[3], size_t cap,
                                uint64_t* pair_a, uint64_t* pair_b,
                                double* dist, int32_t* off_zyx, size_t* n);

/* HIP-event kernel time (no host<->device copies) of the last expansion
 * (index 0) and the last contact scan + reduction (index 1) on this handle,
 * and the HBM bytes each is specified to move (algorithmic). */
int ffn_decision_last_timing(ffn_decision* h, double kernel_ms[2],
                             double algorithmic_bytes[2]);

#ifdef __cplusplus
}
#endif
#endif /* FFN_DECISION_H_ */
