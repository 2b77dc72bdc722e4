/* Pillow's 8-bit image resize on the device (blobctrl_amd/resample.py): the resampling in front of DINOv2, SAM and the VAE.  A header of its
 * own beside blobctrl_edit.h.  These entry points are DIRECT launches on the caller's stream: they are not recordable plan ops, have no
 * BC_OP_* code and never appear in a .bcplan file.  0 on success, 1 on bad arguments (bc_last_error(); nothing is launched then), 2 when a
 * launch fails.
 *
 * The algorithm is Pillow's `ImagingResample` for 8-bit channels: a separable convolution, the horizontal pass first into a uint8
 * intermediate, the vertical pass second.  Each pass is driven by two tables the caller computes on the host, as Pillow does
 * (`resample_tables`), and hands over IN DEVICE MEMORY:
 *     bounds int32 [out][2]       (first source index, number of taps) of every output index
 *     coeffs int32 [out][ksize]   the taps in units of 2^-22
 * and computes  out = clamp((2^21 + sum_{k < min(taps, ksize)} coeffs[o][k] * in[first + k]) >> 22, 0, 255)  in 32-bit integers - the
 * same bytes as Pillow, with no tolerance.  The library cannot inspect a table, so the kernels guard every source index: a tap outside the
 * input contributes nothing and reads nothing (the Python layer never produces one).  The sum wraps modulo 2^32 where a table lets it
 * overflow; Pillow's tables keep 255 * sum |coeffs| + 2^21 below 2^31.
 *
 * Images are interleaved uint8 [n][H][W][3] at any alignment; the tables and the fp32 arrays are aligned to 4 bytes.  Offsets are 64-bit. */
#ifndef BLOBCTRL_RESAMPLE_H
#define BLOBCTRL_RESAMPLE_H
#include "blobctrl_edit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The horizontal pass, for the rows the vertical pass will read and the columns of the requested window:
 *   tmp[i][r][x][c] = pass(src[i][r0 + r][.][c]; output index x0 + x)    for i < n, r < rows, x < cw, c < 3
 * src uint8 [n][H][W][3]; bounds_x, coeffs_x the tables of W -> ow; [r0, r0 + rows) inside [0, H); [x0, x0 + cw) inside [0, ow);
 * tmp uint8 [n][rows][cw][3], every byte written.  H, W, ow <= BC_EDIT_MAX_DIM. */
int bc_resample_horizontal(const unsigned char* src, int n, int H, int W, int r0, int rows, const int* bounds_x, const int* coeffs_x,
                           int ksize, int ow, int x0, int cw, unsigned char* tmp, bc_stream stream);

/* The vertical pass with one of two epilogues.  in uint8 [n][IH][IW][3] is either the intermediate of the horizontal pass (IH = rows,
 * IW = cw, its row 0 standing for source row r0, xin0 = 0) or, when the width does not change, the source itself (IH = H, IW = W, r0 = 0,
 * xin0 = x0).  For output rows [y0, y0 + ch) of the resized frame of oh rows, and cw columns from column xin0 of `in`:
 *   v[i][y][x][c] = pass(in[i][. - r0][xin0 + x][c]; output index y0 + y)
 * bounds_y, coeffs_y are the tables of the source height -> oh; a tap whose row falls outside [r0, r0 + IH) contributes nothing.
 *   out_u8  != NULL:  out_u8 uint8 [n][ch][cw][3] = v, every byte written (out_f32 and lut must be NULL; PH, PW are ignored).
 *   out_f32 != NULL:  out_f32 fp32 planar [n][3][PH][PW], PH >= ch, PW >= cw: lut[c][v] at rows < ch and columns < cw, 0.0f in the rest
 *                     of the frame (SAM's padding), every element written.  lut fp32 [3][256] in device memory: the caller's
 *                     normalisation of every byte value, so the device does no floating-point arithmetic at all. */
int bc_resample_vertical(const unsigned char* in, int n, int IH, int IW, int r0, int xin0, const int* bounds_y, const int* coeffs_y,
                         int ksize, int oh, int y0, int ch, int cw, unsigned char* out_u8, float* out_f32, const float* lut, int PH, int PW,
                         bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
