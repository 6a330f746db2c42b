/*
 * libffn_hip.so, forward-only evaluation on training examples -- the FoV loop
 * of the google/ffn checkout's train.py (train.py:202-286 example loading,
 * ffn/training/examples.py and mask.py for seed, crops, moves and the seed
 * update, ffn/training/tracker.py EvalTracker.add_patch for the metrics), run
 * without an optimiser.  This unit owns the data and the voxel work of that
 * loop; it knows nothing about the engine.  A driver composes it with
 * ffn_predict_device (ffn_hip.h): gather -> ffn_predict_device -> paste.
 *
 * Conventions as in ffn_coordinates.h: plain C types, 0 / negative FFN_ERR_*
 * return codes, ffn_last_error() for the message, (z, y, x) order unless a
 * name says xyz, the caller owns host buffers.  A handle owns one HIP stream
 * and device storage; calls on one handle must be serialised.  Every call
 * returns with its kernels complete.  Pointers named *_dev are device memory
 * of the handle's device; whatever wrote them has completed before the call.
 *
 * Exact definition.  With the geometry of ffn_evaluation_configure, a slot
 * holds three dense f32 arrays: the seed canvas (canvas_zyx), the image patch
 * (image_patch_zyx) and the label patch (label_patch_zyx).  For a size s the
 * centre index is s / 2 (integer division) and a patch of size s centred on
 * voxel c of a volume starts at c - (s - 1) / 2 (inputs.py:339-345).
 *
 * load.  image[p] = ((float)v - offset) / scale in f32, the subtraction first,
 * both IEEE-rounded (inputs.py:437); v is the volume's u8 or f32 voxel.
 * labels[p] = (l > 0 && l == l_centre) ? 0.95f : 0.05f with l the volume's
 * label at p and l_centre the one at the label patch's centre index, compared
 * as unsigned 64-bit values (4-byte labels are zero-extended).  seed[p] =
 * seed_pad_logit everywhere, seed_centre_logit at the canvas centre index.
 *
 * An offset (x, y, z) addresses, for an array of size S and a crop of size C,
 * the box that starts at S / 2 - C / 2 + offset per axis (mask.crop_and_pad).
 * gather copies that box of the seed canvas (C = input_seed) and of the image
 * patch (C = input_image).  paste overwrites, inside the input_seed box at the
 * offset, the centred pred_mask box (it starts (input_seed - pred_mask) / 2
 * into it; examples.py:143-156) with the logits.  probe_moves reads
 * seed[canvas / 2 + offset] >= seed_threshold and labels[label_patch / 2 +
 * offset] >= label_threshold (examples._eval_move).  score_faces takes the
 * pred_mask box of the seed canvas at the offset and, with c = pred_mask / 2
 * and d = deltas, the working box [c - d, c + d] per axis; face f = 2 * axis +
 * (0 for -d, 1 for +d), axes in z, y, x order, is that box with `axis` fixed at
 * c -/+ d.  Its score is the largest value of the face and its position the
 * first one holding it in C order (np.argmax; the seed holds no NaN), given
 * relative to the box centre: (dz, dy, dx) with the fixed axis at -/+ d
 * (movement.get_scored_move_offsets, which then drops scores below its
 * threshold and axes of delta 0: that is left to the caller).
 *
 * finish.  Over the eval_zyx boxes at offset 0 of the seed canvas (x) and the
 * label patch (z): loss_sum = sum of max(x, 0) - x * z + log1p(exp(-|x|)), the
 * numerically stable form TensorFlow documents for
 * sigmoid_cross_entropy_with_logits, with weight 1, in f32: every thread sums
 * its voxels in index order, then lanes, waves and workgroups are combined as
 * a fixed tree, so the sum is the same from run to run.  counts (tp, tn, fp,
 * fn) with pred = x >= pred_threshold and true = z > 0.5f are exact.  The loss
 * weights of an unaugmented example are all 1, so no voxel is masked and
 * *masked is 0.
 */
#ifndef FFN_EVALUATION_H_
#define FFN_EVALUATION_H_

#include <stddef.h>
#include <stdint.h>

#include "ffn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FFN_EVALUATION_MAX_SLOTS 32
/* ffn_evaluation_paste: how logits_dev is laid out. */
#define FFN_EVALUATION_LOGITS_PRED 0 /* dense [n][pred_mask]                  */
#define FFN_EVALUATION_LOGITS_FOV 1  /* dense [n][input_seed], what
                                        ffn_predict_device writes; the centred
                                        pred_mask box of it is read           */

typedef struct ffn_evaluation ffn_evaluation;

typedef struct ffn_evaluation_geometry {
  int32_t input_seed_zyx[3];
  int32_t input_image_zyx[3];
  int32_t pred_mask_zyx[3];
  int32_t deltas_zyx[3];
  int32_t canvas_zyx[3];      /* train.py:177-179 */
  int32_t image_patch_zyx[3]; /* train.py:172-174 */
  int32_t label_patch_zyx[3]; /* train.py:162-164 */
  int32_t eval_zyx[3];        /* train.py:167-169 */
  int32_t slots;              /* 1 .. FFN_EVALUATION_MAX_SLOTS */
} ffn_evaluation_geometry;

int ffn_evaluation_create(int device_id, ffn_evaluation** out);
void ffn_evaluation_destroy(ffn_evaluation* h);

/* Sets the geometry and allocates the slots (their contents are undefined
 * until loaded).  Every size is positive; per axis pred_mask <= input_seed with
 * an even difference, input_seed <= canvas, input_image <= image_patch,
 * pred_mask <= label_patch, and eval <= canvas and <= label_patch.  Volumes
 * are kept. */
int ffn_evaluation_configure(ffn_evaluation* h,
                             const ffn_evaluation_geometry* geometry);

/* Three device arrays owned by the handle, valid until the next configure or
 * destroy, for a driver that has no allocator of its own: seed [slots]
 * [input_seed], image [slots][input_image] (the outputs of gather) and logits
 * [slots][input_seed] (what ffn_predict_device writes and paste reads). */
int ffn_evaluation_io_buffers(ffn_evaluation* h, float** seed_dev,
                              float** image_dev, float** logits_dev);

/* Forgets every volume. */
int ffn_evaluation_reset(ffn_evaluation* h);

/* Copies a HOST image (image_elem 1 = uint8, 4 = f32) and HOST labels
 * (label_elem 4 or 8 bytes, unsigned) of one shape to the device, where they
 * stay; *index is the volume's number. */
int ffn_evaluation_add_volume(ffn_evaluation* h, const void* image,
                              int image_elem, const void* labels,
                              int label_elem, const int64_t shape_zyx[3],
                              int32_t* index);

/* Fills slots[k] from volumes[k] around centres_xyz[3 k ..] for k < n, in one
 * launch (n <= slots, the slots distinct).  If any patch leaves its volume the
 * call is FFN_ERR_ARG and no slot is touched. */
int ffn_evaluation_load(ffn_evaluation* h, int n, const int32_t* slots,
                        const int32_t* volumes, const int32_t* centres_xyz,
                        const float* offsets, const float* scales,
                        float seed_pad_logit, float seed_centre_logit);

/* n (slot, offset) pairs, any number, in one launch -> valid[k], wanted[k]
 * (0 / 1).  An offset outside the canvas or the label patch is FFN_ERR_ARG. */
int ffn_evaluation_probe_moves(ffn_evaluation* h, size_t n,
                               const int32_t* slots, const int32_t* offsets_xyz,
                               float seed_threshold, float label_threshold,
                               uint8_t* valid, uint8_t* wanted);

/* seed_out_dev: [n][input_seed], image_out_dev: [n][input_image], f32, entry k
 * from slots[k] at offsets_xyz[3 k ..]; n <= slots.  A box that leaves the
 * canvas or the image patch is FFN_ERR_ARG; nothing is written then. */
int ffn_evaluation_gather(ffn_evaluation* h, int n, const int32_t* slots,
                          const int32_t* offsets_xyz, float* seed_out_dev,
                          float* image_out_dev);

/* The seed update; the slots distinct, n <= slots. */
int ffn_evaluation_paste(ffn_evaluation* h, int n, const int32_t* slots,
                         const int32_t* offsets_xyz, const float* logits_dev,
                         int logits_layout);

/* scores: 6 per entry; positions_zyx: 6 x 3 per entry.  deltas <= pred_mask / 2
 * per axis, else FFN_ERR_ARG. */
int ffn_evaluation_score_faces(ffn_evaluation* h, int n, const int32_t* slots,
                               const int32_t* offsets_xyz, float* scores,
                               int32_t* positions_zyx);

/* counts: tp, tn, fp, fn. */
int ffn_evaluation_finish(ffn_evaluation* h, int slot, float pred_threshold,
                          float* loss_sum, int64_t counts[4], int64_t* masked);

/* Whole arrays of a slot to / from the host (canvas, label patch, image patch
 * sizes).  write_seed replaces the seed canvas. */
int ffn_evaluation_read_seed(ffn_evaluation* h, int slot, float* out);
int ffn_evaluation_read_labels(ffn_evaluation* h, int slot, float* out);
int ffn_evaluation_read_image(ffn_evaluation* h, int slot, float* out);
int ffn_evaluation_write_seed(ffn_evaluation* h, int slot, const float* in);

/* HIP-event kernel time (no host<->device copies) of the last load (index 0),
 * probe_moves (1), gather (2), paste (3), score_faces (4) and finish (5) on
 * this handle, and the bytes each is specified to move (algorithmic: load, the
 * volume voxels read and the three arrays written; probe, 8 bytes read per
 * pair; gather and paste, every f32 once in and once out; score_faces, the six
 * faces; finish, the two eval boxes). */
int ffn_evaluation_last_timing(ffn_evaluation* h, double kernel_ms[6],
                               double algorithmic_bytes[6]);

/* ---- what a training loop needs on top of the above (train.py:252-274) ----
 *
 * load_augmented is load followed by train.py's PermuteAndReflect on the image
 * and the label patch.  perms holds 3 int32 per entry: the source axis of each
 * output axis in zyx numbering (np.transpose); reflects 3 uint8 per entry, 0 or
 * 1.  With P the array load writes, the slot holds flip(transpose(P, perm),
 * axes with reflect = 1): out[i] = P[k] with j_a = reflect[a] ? S_a - 1 - i_a :
 * i_a and k[perm[a]] = j_a.  The box, the normalisation and the local object
 * mask (against the label at the centre index of the untransformed patch) are
 * load's; the seed canvas is load's fresh one, untransformed.  The identity
 * writes what load writes, bit for bit.  FFN_ERR_ARG with no slot touched: a
 * perm that is no permutation of 0, 1, 2; a reflect that is not 0 or 1; an axis
 * a with perm[a] != a whose image-patch or label-patch size differs from that
 * of axis perm[a]; any of load's own errors.  One launch. */
int ffn_evaluation_load_augmented(ffn_evaluation* h, int n,
                                  const int32_t* slots, const int32_t* volumes,
                                  const int32_t* centres_xyz,
                                  const float* offsets, const float* scales,
                                  const int32_t* perms, const uint8_t* reflects,
                                  float seed_pad_logit,
                                  float seed_centre_logit);

/* gather, and into labels_out_dev [n][pred_mask] the pred_mask box of the
 * label patch at the offset (it starts at label_patch / 2 - pred_mask / 2 +
 * offset per axis; examples.py:65), in one launch.  A box that leaves its
 * array is FFN_ERR_ARG; nothing is written then. */
int ffn_evaluation_gather_train(ffn_evaluation* h, int n, const int32_t* slots,
                                const int32_t* offsets_xyz, float* seed_out_dev,
                                float* image_out_dev, float* labels_out_dev);

/* A fourth device array beside those of ffn_evaluation_io_buffers, with their
 * lifetime: labels [slots][pred_mask], the third output of gather_train. */
int ffn_evaluation_io_labels(ffn_evaluation* h, float** labels_dev);

/* As last_timing, of the last load_augmented (index 0; bytes as load) and
 * gather_train (1; every f32 once in and once out). */
int ffn_evaluation_last_timing_train(ffn_evaluation* h, double kernel_ms[2],
                                     double algorithmic_bytes[2]);

/* ---- section augmentations (ffn/training/augmentation.py: misalignment,
 * missing_section, out_of_focus_section, grayscale_perturb) --------------------
 *
 * load_sections is load_augmented with a plan per entry that is carried out
 * between reading the volume and load's normalisation.  The plan holds
 * decisions only (the caller samples them); the voxel work is the device's.
 * All image arithmetic is f32 on the voxel converted to f32, i.e. what the
 * reference's functions compute when they are handed the patch cast to
 * float32.  (Handed a uint8 patch they truncate after every operation; that
 * is NOT reproduced.)  In this order:
 *
 * 1. Misalignment, on the image and the labels.  An array whose slot size
 *    ("final" size) is (Z, Hf, Wf) is taken from the volume as the box of
 *    size (Z, H, W) = (Z, Hf + 2 margin_y, Wf + 2 margin_x) around the same
 *    centre voxel.  M is the per-axis maximum of the two boxes (image,
 *    labels), z included.  Section z of an array is moved when, with zp = z +
 *    (M_z - Z) / 2, zp == z0 (kind 1, slip) or zp >= z0 (kind 2,
 *    translation).  Final index y reads the box at row
 *      clamp(p - (M_y - H) / 2, 0, H - 1),  p = y + (M_y - Hf) / 2,
 *    with p replaced by (p - dy) mod M_y in a moved section; x likewise with
 *    (p + dx) mod M_x.  Divisions are integer; mod is non-negative.  This is
 *    np.roll(., dy, y) and np.roll(., -dx, x) on the arrays edge-padded to M,
 *    then the centre crop, as the reference's misalignment() does it.  No
 *    read leaves the box.  labels[p] is load's soft 0.95 / 0.05 of the label
 *    at the mapped index against the label at the centre index of the final,
 *    unmoved label patch.
 * 2. Missing section, image only, final image-patch coordinates: a voxel (y,
 *    x) of section z selected by blank_mask becomes blank_value.  Mask bit 0
 *    selects [0:sy, 0:sx], bit 1 [sy:, 0:sx], bit 2 [0:sy, sx:], bit 3 [sy:,
 *    sx:] with (sy, sx) the split point (_quadrant_replace); a whole section
 *    is bit 3 with the split point (0, 0).
 * 3. Out of focus: a voxel selected by blur_mask takes the value of the
 *    Gaussian blur of its section as it is after step 2.  The blur is
 *    scipy.ndimage.gaussian_filter's: radius r = (int)(4 sigma + 0.5) from
 *    blur_sigma widened to double, weights w_k = exp(-k^2 / (2 sigma^2)) / sum
 *    in double (computed by the library on the host), along y, the result
 *    rounded to f32, then along x, rounded to f32; boundary `reflect` (d c b
 *    a | a b c d | d c b a, period 2 n, so r may exceed the plane).  One
 *    output is w_0 v_0 + sum for k = r .. 1 of (v_-k + v_+k) w_k, every
 *    operation a double one, in this order, none contracted.  r == 0 is the
 *    identity.
 * 4. Grayscale, where gray = 1: n = v / 255; a = n * contrast; a = a +
 *    brightness; c = min(max(a, 0), 1); v = powf(c, gamma) * 255.  Every
 *    operation up to c is one IEEE f32 operation (no fused multiply-add), so c
 *    is what numpy computes; powf is the device's; the last product is an
 *    IEEE f32 one.
 * Then load's (v - offset) / scale, then load_augmented's transform of the
 * image and label patches.  The seed canvas is load's.
 *
 * A plan of zeros writes what load_augmented writes, bit for bit.
 *
 * FFN_ERR_ARG, no slot touched: whatever load_augmented refuses; a negative
 * margin, or one above 4096 (the largest size configure takes); kind not 0,
 * 1, 2; z0 outside [0, M_z); |dy| > M_y or |dx| > M_x; a mask above 15 or a
 * gray above 1; a split point outside [0, Hf] x [0, Wf]; a blur_sigma that is
 * negative or NaN or gives r > 31 (any sigma above 16, an infinite one
 * included, is refused before r is formed); with gray = 1 a gamma <= 0 or a
 * contrast, brightness or gamma that is not finite; an enlarged box
 * that leaves its volume; a blur (a non-zero blur_mask with r > 0) on an
 * image plane of more than 128 x 128 = 16384 voxels (the section and its
 * intermediate stay in the 160 KiB of LDS; larger planes are refused, not
 * tiled).
 *
 * Two launches: the augmented, untransformed patches go to scratch owned by
 * the handle, then load_augmented's transposing copy fills the slots. */
#define FFN_EVALUATION_MAX_BLUR_RADIUS 31
#define FFN_EVALUATION_MAX_BLUR_PLANE 16384

typedef struct ffn_evaluation_section_plan { /* one per entry */
  int32_t margin_yx[2];
  int32_t kind; /* 0 none, 1 slip, 2 translation */
  int32_t z0, dy, dx;
  float blank_value;
  float blur_sigma;
} ffn_evaluation_section_plan;

typedef struct ffn_evaluation_section { /* one per entry and image section */
  uint8_t blank_mask, blur_mask; /* 4 quadrant bits each */
  uint8_t gray;                  /* 0 / 1 */
  uint8_t reserved;              /* 0 */
  int32_t blank_yx[2], blur_yx[2]; /* split points */
  float contrast, brightness, gamma;
} ffn_evaluation_section;

/* plans: n entries; sections: dense [n][image_patch_zyx[0]]. */
int ffn_evaluation_load_sections(
    ffn_evaluation* h, int n, const int32_t* slots, const int32_t* volumes,
    const int32_t* centres_xyz, const float* offsets, const float* scales,
    const int32_t* perms, const uint8_t* reflects,
    const ffn_evaluation_section_plan* plans,
    const ffn_evaluation_section* sections, float seed_pad_logit,
    float seed_centre_logit);

/* As last_timing_train, of the last load_sections: index 0 the whole call
 * (both launches; bytes as load), index 1 its first launch alone, the section
 * kernel (the volume voxels of the two final patches read, their two f32
 * arrays written). */
int ffn_evaluation_last_timing_sections(ffn_evaluation* h, double kernel_ms[2],
                                        double algorithmic_bytes[2]);

#ifdef __cplusplus
}
#endif
#endif /* FFN_EVALUATION_H_ */
