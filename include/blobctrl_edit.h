/* The inputs of an edit, built on the device (blobctrl_amd/edit_inputs.py): what stands between a clean SAM mask and the pipeline call -
 * the filled ellipses of `blob_edit.ellipse_mask`, painted over a request batch, the first / last set column of every mask row (all the
 * convex hull and the bounding box need), and the object cut out onto a white canvas.  A header of its own beside blobctrl_masks.h.  These
 * entry points are DIRECT launches on the caller's stream: they are not recordable plan ops, have no BC_OP_* code and never appear in a
 * .bcplan file.  0 on success, 1 on bad arguments (bc_last_error(); nothing is launched then), 2 when a launch fails.
 *
 * Results are THE SAME BYTES as the host functions of blobctrl_amd/blob_edit.py give.  The integer kernels are exact by construction.  The
 * ellipse predicate evaluates the host function's expressions in its order in fp64, with multiply-add contraction off, true division and no
 * transcendental on the device (the caller hands over cos and sin): every operation is one correctly rounded IEEE-754 operation on both
 * sides, so every intermediate is the same double.
 *
 * An ellipse is six doubles: xc, yc, a, b, cos t, sin t - centre, SEMI-axes (already floored: a = max(d1 / 2, 1e-9)), and the rotation,
 * prepared exactly as `ellipse_mask` prepares them.  All six must be finite and a, b > 0; the library cannot see them (they are in device
 * memory), the Python layer refuses others. */
#ifndef BLOBCTRL_EDIT_H
#define BLOBCTRL_EDIT_H
#include "blobctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest H and W any entry point below takes (so H * W <= 2^28 and a pixel index fits an int; offsets into a batch are 64-bit). */
#define BC_EDIT_MAX_DIM 16384

/* `blob_edit.ellipse_mask`, batched: mask[i][y][x] = 255 where the closed pixel square [x - 0.5, x + 0.5] x [y - 0.5, y + 0.5] meets the
 * filled ellipse i, else 0.  ell fp64 [n][6] (8-byte aligned), mask uint8 [n][H][W] (any alignment); every byte of mask is written. */
int bc_ellipse_cover(const double* ell, int n, int H, int W, unsigned char* mask, bc_stream stream);

/* Paint k ellipses over each of n images, in place: images uint8 [n][H][W][3]; image i takes ellipse (i, j) in colour rgb[i][j] for
 * j = 0 .. k - 1 in that order, so a pixel ends in the colour of the LAST ellipse that covers it and is not touched when none does.  ell
 * fp64 [n][k][6], rgb uint8 [n][k][3].  The predicate is bc_ellipse_cover's.  k = 2 with white then black is
 * `composite_mask_and_image(ellipse_mask(target), composite_mask_and_image(ellipse_mask(start), image, white), black)` for a whole batch. */
int bc_ellipse_paint(unsigned char* images, int n, int H, int W, const double* ell, const unsigned char* rgb, int k, bc_stream stream);

/* out[i][y] = (first, last) set column of row y of mask i, (-1, -1) for an empty row.  masks uint8 [n][H][W], non-zero = set, any base
 * alignment and any W (rows are generally not aligned); out int32 [n][H][2], every word written, nothing to zero beforehand, no atomics. */
int bc_mask_row_extents(const unsigned char* masks, int n, int H, int W, int* out, bc_stream stream);

/* `blob_edit.object_region_from_mask`, batched: out[i] = a white canvas with the pixels of box i = (x, y, w, h) of `image` pasted at
 * ((H - h) / 2, (W - w) / 2), white where mask i is zero.  image uint8 [H][W][3], masks uint8 [n][H][W], boxes int32 [n][4] IN DEVICE
 * MEMORY, out uint8 [n][H][W][3], every byte written.  A box that leaves the frame reads nothing outside it (those pixels stay white). */
int bc_mask_cutout(const unsigned char* image, const unsigned char* masks, const int* boxes, int n, int H, int W, unsigned char* out,
                   bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
