/*
 * libffn_hip.so, balanced training coordinates -- build_coordinates.py of the
 * google/ffn checkout: from the partition maps of ffn_partitions.h, every
 * class resampled to the size of the largest one, shuffled, and written as
 * (centre, volume name) training examples.
 *
 * Conventions as in ffn_partitions.h: plain C types, 0 / negative FFN_ERR_*
 * return codes, ffn_last_error() for the message, (z, y, x) order unless a
 * name says xyz, the caller owns host buffers.  A handle owns one HIP stream
 * and device storage; calls on one handle must be serialised.  Every call
 * returns with its kernels complete.
 *
 * Exact definition.  Volume i (uint8, already cropped by the margin, C order)
 * contributes, for every class c != 255, the ascending flat indices of its
 * voxels of value c; sorted_c is the concatenation of these lists over the
 * volumes in the order they were added, n_c its length.  With the class order
 * classes[0..K), max_count, one index vector perm_c (a permutation of 0..n_c)
 * per class and `order` (a permutation of 0..K * max_count), output row r is
 *   q = order[r];  k = q / max_count;  t = q % max_count;  c = classes[k];
 *   (i, flat) = sorted_c[perm_c[t % n_c]];
 *   (z, y, x) = flat unravelled in the shape of volume i;
 *   centre_xyz(r) = (mx + x, my + y, mz + z);  volume_index(r) = i.
 * The device draws no random number: the host makes perm_c and order (from
 * numpy's legacy MT19937 stream, to reproduce the reference's sequence).  All
 * of it is integer work; the sorted lists do not depend on the order in which
 * any atomic lands and are byte-identical from run to run.
 *
 * Serialised form.  Row r becomes one TFRecord record,
 *   u64le length | u32le masked_crc32c(those 8 bytes) | payload |
 *   u32le masked_crc32c(payload),
 *   masked(crc) = ((crc >> 15 | crc << 17) + 0xa282ead8) mod 2^32,
 * whose payload is a tf.train.Example in protobuf wire format:
 *   Example{1: Features{1: repeated entry{1: key, 2: Feature}}},
 *   Feature{1: BytesList{1: bytes}, 3: Int64List{1: packed varints}}
 * with the two entries in key order: "center" (the three int64 of centre_xyz),
 * then "label_volume_name" (the name of volume i).  The entries are a protobuf
 * map: TensorFlow's own Python writer promises no order for them and every
 * reader accepts either, so files written here and by the reference hold the
 * same examples but need not be the same bytes.  The bytes are uncompressed;
 * the caller compresses (the reference writes GZIP).
 */
#ifndef FFN_COORDINATES_H_
#define FFN_COORDINATES_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ffn_coordinates ffn_coordinates;

int ffn_coordinates_create(int device_id, ffn_coordinates** out);
void ffn_coordinates_destroy(ffn_coordinates* h);

/* Forgets every volume, the gathered rows and the names. */
int ffn_coordinates_reset(ffn_coordinates* h);

/* Appends a HOST crop (uint8, fewer than 2^31 voxels) as the next volume: a
 * stable counting sort of its flat indices by value.  counts[c] is the number
 * of voxels of value c (256 entries, 255 included); the lists of the classes
 * other than 255 stay resident. */
int ffn_coordinates_add_volume(ffn_coordinates* h, const uint8_t* crop,
                               const int64_t shape_zyx[3],
                               uint64_t counts[256]);

/* Copies the resident list of class `cls` (0..254) of volume `volume` to the
 * host.  *n is its length (FFN_ERR_ARG if > cap; nothing is written then). */
int ffn_coordinates_read_class(ffn_coordinates* h, size_t volume, int cls,
                               size_t cap, uint32_t* flat, size_t* n);

/* Output rows as defined above.  classes: n_classes distinct values below 255,
 * each present in some volume.  perms: the perm_c vectors one after another in
 * the order of `classes` (perms_len = the sum of their n_c).  order: n_rows =
 * n_classes * max_count entries, n_rows < 2^31.  An entry of perms or order
 * out of its range is FFN_ERR_ARG.  The rows stay resident until the next
 * gather or reset. */
int ffn_coordinates_gather(ffn_coordinates* h, const uint8_t* classes,
                           size_t n_classes, uint64_t max_count,
                           const uint32_t* perms, size_t perms_len,
                           const uint32_t* order, size_t n_rows,
                           const int32_t margin_zyx[3]);

/* Copies rows [row0, row0 + n_rows) to the host; either pointer may be NULL.
 * centers_xyz: 3 int32 per row; volume_index: one int32 per row. */
int ffn_coordinates_read(ffn_coordinates* h, size_t row0, size_t n_rows,
                         int32_t* centers_xyz, int32_t* volume_index);

/* The names of the volumes, in the order they were added: the bytes of all of
 * them one after another, name i = bytes[offsets[i] .. offsets[i + 1])
 * (n_names + 1 offsets), none empty.  Kept until the next reset. */
int ffn_coordinates_set_names(ffn_coordinates* h, const uint8_t* bytes,
                              const uint32_t* offsets, size_t n_names);

/* Encodes rows [row0, row0 + n_rows) as TFRecord bytes (see above) into the
 * HOST buffer `out`.  The window is bounded: n_rows times the longest possible
 * record must stay below 2^32 bytes.  *n_bytes is the size of the window
 * (FFN_ERR_ARG if > cap; nothing is written then). */
int ffn_coordinates_serialize(ffn_coordinates* h, size_t row0, size_t n_rows,
                              size_t cap, uint8_t* out, size_t* n_bytes);

/* HIP-event kernel time (no host<->device copies) of the last add_volume
 * (index 0), gather (1) and serialize (2) on this handle, and the HBM bytes
 * each is specified to move (algorithmic: the crop read twice plus one u32 per
 * listed voxel; order, one perm entry, one list entry and 16 bytes out per
 * row; 16 bytes in and the record bytes out per row). */
int ffn_coordinates_last_timing(ffn_coordinates* h, double kernel_ms[3],
                                double algorithmic_bytes[3]);

#ifdef __cplusplus
}
#endif
#endif /* FFN_COORDINATES_H_ */
