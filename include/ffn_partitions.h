/*
 * libffn_hip.so, local-object-mask partition maps -- the whole-volume step of
 * compute_partitions.py of the google/ffn checkout: for every labelled voxel,
 * the number of equally labelled voxels inside the LOM box around it, turned
 * into a class by a table (the quantised "active fraction"), from which
 * build_coordinates.py balances training examples.
 *
 * Conventions as in ffn_decision.h: plain C types, 0 / negative FFN_ERR_*
 * return codes, ffn_last_error() for the message, (z, y, x) order, the caller
 * owns host buffers.  A handle owns one HIP stream and grow-only device
 * scratch; calls on one handle must be serialised.  Every call returns with
 * its kernels complete.
 *
 * Exact definition.  With the volume seg of shape (Z, Y, X), the radii
 * r = (rz, ry, rx) and V = (2 rz + 1)(2 ry + 1)(2 rx + 1), the output covers
 * the VALID region seg[rz:Z-rz, ry:Y-ry, rx:X-rx]; output voxel o has the
 * centre v = o + r.  A voxel is labelled when its id is a key with a non-zero
 * keep flag (id 0 is never kept).  For a labelled centre
 *   count(v) = #{u : |u - v| <= r on every axis, seg[u] == seg[v]}   (1..V)
 *   partitions(o) = class_of[count(v)];
 * for any other centre count is 0 and partitions is 0.  On top of that
 * partitions(o) = 255 where any voxel of the LOM box of v has a non-zero mask
 * byte, or where v lies in one of the spheres (x, y, z, radius), tested in f64
 * as ((vx - x)^2 + (vy - y)^2) + (vz - z)^2 <= radius * radius with the terms
 * added in that order and nothing contracted into an FMA.  All of it is integer
 * arithmetic (the spheres aside), so results are exact and reproducible.
 */
#ifndef FFN_PARTITIONS_H_
#define FFN_PARTITIONS_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffn_partitions ffn_partitions;

int ffn_partitions_create(int device_id, ffn_partitions** out);
void ffn_partitions_destroy(ffn_partitions* h);

/* Uploads a HOST label volume of elem_bytes 4 (uint32 / int32 bit pattern) or
 * 8 (uint64; any id below 2^64 - 1) with fewer than 2^31 voxels and returns
 * its distinct ids (0 included) with their voxel counts, unsorted.  *n is the
 * true number of ids (FFN_ERR_ARG if > cap; nothing past cap is written).  The
 * volume and the id table stay resident until the next call. */
int ffn_partitions_label_sizes(ffn_partitions* h, const void* seg,
                               int elem_bytes, const int64_t shape_zyx[3],
                               size_t cap, uint64_t* ids, uint64_t* sizes,
                               size_t* n);

/* Partition map of the resident volume.  keys / keep: n_keys ids and their
 * keep flags (ids the volume does not hold are ignored, ids not listed are not
 * kept).  radius_zyx: each 0..32 and 2 r + 1 no longer than its axis.
 * class_of: class_len = V + 1 bytes.  mask: NULL or one byte per voxel of the
 * volume.  spheres: NULL or 4 doubles (x, y, z, radius) each, in coordinates of
 * the input volume.  The result stays resident until the next call. */
int ffn_partitions_compute(ffn_partitions* h, const uint64_t* keys,
                           const uint8_t* keep, size_t n_keys,
                           const int32_t radius_zyx[3], const uint8_t* class_of,
                           size_t class_len, const uint8_t* mask,
                           const double* spheres, size_t n_spheres);

/* Copies the resident result to the host; any pointer may be NULL.
 * partitions and counts have the shape of the valid region; histogram[c] is the
 * number of output voxels of value c (256 entries). */
int ffn_partitions_read(ffn_partitions* h, uint8_t* partitions,
                        uint32_t* counts, uint64_t* histogram);

/* HIP-event kernel time (no host<->device copies) of the last label_sizes
 * (index 0) and the last compute (index 1) on this handle, and the HBM bytes
 * each is specified to move (algorithmic: the labels once, plus for compute
 * one output byte per voxel). */
int ffn_partitions_last_timing(ffn_partitions* h, double kernel_ms[2],
                               double algorithmic_bytes[2]);

#ifdef __cplusplus
}
#endif
#endif /* FFN_PARTITIONS_H_ */
