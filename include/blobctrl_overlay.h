/* Zoomed ("only masked") edits on the device (blobctrl_amd/overlay.py): the bounds of a mask, Pillow's Gaussian blur of a mask, and the
 * paste of an edit's result back over the original through that mask - `get_crop_region`, `blur` and `apply_overlay` of
 * D/image_processor.py:VaeImageProcessor.  A header of its own beside blobctrl_resample.h.  These entry points are DIRECT launches on the
 * caller's stream: they are not recordable plan ops, have no BC_OP_* code and never appear in a .bcplan file.  0 on success, 1 on bad
 * arguments (bc_last_error(); nothing is launched then), 2 when a launch fails.
 *
 * Everything here is Pillow's own 8-bit integer arithmetic, so results are THE SAME BYTES as Pillow's, with no tolerance.  Images are
 * uint8 at any base alignment and any W; offsets into a batch are 64-bit; H and W are at most BC_EDIT_MAX_DIM. */
#ifndef BLOBCTRL_OVERLAY_H
#define BLOBCTRL_OVERLAY_H
#include "blobctrl_edit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest integer box radius R the blur launches take: that of `GaussianBlur(64)` (box radius 63.5).  It follows from the LDS budget of
 * the column launch: a tile of 64 columns x (64 rows + a halo of 3 (R + 1) rows on both sides), twice (the passes alternate between two
 * buffers), is 64 x 448 x 2 = 56 KiB at R = 63, inside the 64 KiB a workgroup may declare statically. */
#define BC_BLUR_MAX_R 63

/* Three passes of Pillow's box blur (BoxBlur.c:ImagingLineBoxBlur8) along every ROW of src uint8 [n][H][W] -> dst uint8 [n][H][W], in one
 * launch.  One pass over a line of W pixels, with the edge pixels repeated:
 *     out[x] = ((sum of in[x - R .. x + R]) * ww + (in[x - R - 1] + in[x + R + 1]) * fw + 2^23) >> 24       (32-bit unsigned)
 * and a uint8 line between passes.  R in [0, BC_BLUR_MAX_R]; ww, fw >= 0 with (2 R + 1) ww + 2 fw <= 2^24 (so nothing overflows) are
 * Pillow's weights, which the caller computes in float32 as Pillow does.  dst must not overlap src.  Every byte of dst is written. */
int bc_box_blur3_rows(const unsigned char* src, int n, int H, int W, int R, int ww, int fw, unsigned char* dst, bc_stream stream);

/* The same three passes along every COLUMN.  `ImageFilter.GaussianBlur` is bc_box_blur3_rows followed by bc_box_blur3_cols. */
int bc_box_blur3_cols(const unsigned char* src, int n, int H, int W, int R, int ww, int fw, unsigned char* dst, bc_stream stream);

/* out[i] = (first column, last column, first row, last row) holding a non-zero pixel of mask i, four -1 for an empty mask.  masks uint8
 * [n][H][W]; extents int32 [n][H][2] is workspace (bc_mask_row_extents' output, which this entry point launches first and then reduces);
 * out int32 [n][4], every word written, no atomics.  Both int32 arrays aligned to 4 bytes. */
int bc_mask_bounds(const unsigned char* masks, int n, int H, int W, int* extents, int* out, bc_stream stream);

/* `apply_overlay` once init, mask and result share a frame: for i < n, every pixel (Y, X) and channel c
 *     d = patch[i][Y - y][X - x][c] inside the patch's rectangle, 0 outside it
 *     m' = 255 - mask[Y][X];   a = DIV255(m' * 255);   p = DIV255(m' * init[Y][X][c])        DIV255(v) = ((v + 128 >> 8) + v + 128) >> 8
 *     u = min(255, 255 * p / a)                                                               (the RGBa -> RGBA conversion)
 *     coef1 = a * 255 * 255 * 128 / (a * 255 + 255 * (255 - a));   coef2 = 255 * 128 - coef1      (alpha_composite, 7 precision bits)
 *     t = u * coef1 + d * coef2 + (0x80 << 7);   out[i][Y][X][c] = a == 0 ? d : (((t >> 8) + t) >> 8) >> 7
 * init uint8 [H][W][3], mask uint8 [H][W], patches uint8 [n][h][w][3] placed at column x, row y; the rectangle must lie inside the frame
 * (x, y >= 0, x + w <= W, y + h <= H; the whole frame for a result that is not cropped).  out uint8 [n][H][W][3], every byte written; it
 * must not overlap an input. */
int bc_overlay_composite(const unsigned char* init, const unsigned char* mask, const unsigned char* patches, int n, int H, int W, int h, int w,
                         int x, int y, unsigned char* out, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
