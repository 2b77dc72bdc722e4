/* Entry points of the Segment-Anything path (blobctrl_amd/sam.py): SAM's attention form - windowed attention over zero-padded windows
 * with the decomposed relative-position bias - and the small launches around it that no entry point of include/blobctrl_hip.h
 * expresses.  A header of its own beside that one; all launches are recordable plan ops (BC_OP_ATTENTION_RELPOS .. BC_OP_MASK_STATS in the
 * BC_OP_* table there).  SAM segments are recorded and replayed in-process only: these ops are never written to a .bcplan file.
 * Conventions as in blobctrl_hip.h: fp16 activations, fp32 accumulation, all work on the caller's stream, 0 on success. */
#ifndef BLOBCTRL_SAM_H
#define BLOBCTRL_SAM_H
#include "blobctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* softmax(scale * Q K^T + bias) V with bias[q][k] = rel_h[q][kh(k)] + rel_w[q][kw(k)].  Keys lie on a Kh x Kw grid (k = kh * Kw + kw),
 * queries on a Qh x Qw grid (q = qh * Qw + qw); the two grids must be the same.
 *   rel_h[q][j] = sum_c Q[q][c] * Rh[qh - j + Kh - 1][c]      (the UNSCALED query; `scale` applies to Q K^T only)
 *   rel_w[q][j] = sum_c Q[q][c] * Rw[qw - j + Kw - 1][c]
 * Rh fp16 [2 Kh - 1][d], Rw fp16 [2 Kw - 1][d]: one table pair per launch, shared by all heads and images.
 * Q / K / Vt / O and their strides as in bc_attention (Vt zero padded to Kh * Kw rounded up to 64); d in {40, 64, 80}.  Keys past
 * Kh * Kw in the last 64-key tile are masked (never read); the bias is added in fp32 before the row maximum.
 * rel = fp32 scratch [B][heads][Qh * Qw][Kh + Kw]: a small launch in front of the attention kernel fills it (already in log2 units). */
int bc_attention_relpos(const bc_half* Q, const bc_half* K, const bc_half* Vt, bc_half* O, int B, int heads, int d, int Qh, int Qw,
                        int Kh, int Kw, int ldq, int ldk, int ldvt, int ldo, long long q_bstride, long long k_bstride,
                        long long vt_bstride, long long o_bstride, float scale, const bc_half* Rh, const bc_half* Rw, float* rel,
                        bc_stream stream);

/* Token rows x [B][H * W][C] -> windows out [B * nWh * nWw][ws * ws][C], nWh = ceil(H / ws), nWw = ceil(W / ws); rows of the bottom /
 * right padding are written as zeros (the reference attends to them).  C a multiple of 8. */
int bc_window_partition(const bc_half* x, int B, int H, int W, int C, int ws, bc_half* out, bc_stream stream);
/* The inverse with the residual: out[b][h][w][:] = win[window of (h, w)][...][:] + res[b][h][w][:]; padded rows are dropped. */
int bc_window_unpartition(const bc_half* win, const bc_half* res, int B, int H, int W, int C, int ws, bc_half* out, bc_stream stream);

/* out[b][t][:] = x[b][t][:] + pos[t][:]  (x fp16 [B][T][D], pos fp32 [T][D]): the absolute position embedding behind the patch GEMM. */
int bc_add_pos(const bc_half* x, const float* pos, int B, int T, int D, bc_half* out, bc_stream stream);
/* out[r][:] = a[r][:] + b[r % b_rows][:]  (fp16, C a multiple of 8): tokens + their positional encoding in the mask decoder. */
int bc_add_rows(const bc_half* a, const bc_half* b, int rows, int b_rows, int C, bc_half* out, bc_stream stream);
/* An activation in place over n fp16 elements (n a multiple of 8): act 0 = exact-erf GELU, 1 = ReLU. */
int bc_act_rows(bc_half* x, long long n, int act, bc_stream stream);

/* F.interpolate(mode="bilinear", align_corners=False) of the crop [0, crop_h) x [0, crop_w) of src fp32 [NC][H][W] to [NC][Ho][Wo].
 * threshold_on == 0: out is fp32; else out is uint8, 1 where the value is > threshold. */
int bc_bilinear_resize_f32(const float* src, int NC, int H, int W, int crop_h, int crop_w, int Ho, int Wo, int threshold_on,
                           float threshold, void* out, bc_stream stream);

/* The decoder's token rows: out fp16 [ntok + npts + 1][C], C = 2 F.  Rows 0 .. ntok-1 = tokens fp32 [ntok][C] (iou + mask tokens); then one
 * row per point: sin | cos of 2 pi ((2 (x + 0.5) / size - 1, 2 (y + 0.5) / size - 1) . gauss), gauss fp32 [2][F], plus label_embed[label]
 * (fp32 [2][C], labels 0 / 1; a label of -1 gives not_a_point instead); the last row = not_a_point fp32 [C] (the padding point the prompt
 * encoder appends when no box is given).  points fp32 [npts][2] (x, y in the input frame) and labels int32 [npts] are device buffers. */
int bc_sam_tokens(const float* tokens, int ntok, const float* points, const int* labels, int npts, const float* gauss, int F,
                  const float* label_embed, const float* not_a_point, float size, bc_half* out, bc_stream stream);

/* Low-res mask logits, the hypernetwork product behind the upscaler: up fp16 [B * h * w * 16][C2] (row = ((pixel * 2 + dy) * 2 + dx) * 4 +
 * dy2 * 2 + dx2: the two 2x2 stride-2 transposed convolutions run as GEMMs whose sub-pixels stay rows), hyper fp16 [B][ntok][ldh]
 * -> out fp32 [B][ntok][4 h][4 w], out[b][t][4 y + 2 dy + dy2][4 x + 2 dx + dx2] = sum_c hyper[b][t][c] * up[row][c]. */
int bc_sam_masks(const bc_half* up, int C2, const bc_half* hyper, int ldh, int B, int h, int w, int ntok, float* out, bc_stream stream);

/* ---- batched prompts and automatic mask generation (BC_OP_SAM_TOKENS_BATCH, BC_OP_MASK_STATS; in-process only like the ops above) ---- */

/* bc_sam_tokens for B prompt sets at once: points fp32 [B][npts][2], labels int32 [B][npts] -> out fp16 [B][ntok + npts + 1][C].  The
 * arithmetic per row is that of bc_sam_tokens; prompt 0 is bit-identical to what bc_sam_tokens writes for the same points. */
int bc_sam_tokens_batch(const float* tokens, int ntok, const float* points, const int* labels, int B, int npts, const float* gauss, int F,
                        const float* label_embed, const float* not_a_point, float size, bc_half* out, bc_stream stream);

/* What SamAutomaticMaskGenerator needs of a mask's logits, in one pass over them: logits fp32 [n][H][W] -> out int32 [n][7] =
 *   count(v > t + o), count(v > t - o), count(v > t), then the inclusive bounding box x0, y0, x1, y1 of v > t (0, 0, 0, 0 when empty).
 * The comparisons are strict and in fp32 against t, fl32(t + o) and fl32(t - o), so the counts are exact and the result does not depend on
 * how the launch splits a mask.  H, W arbitrary with H * W < 2^31 - 2^14; partial = int32 scratch [n][bc_mask_stats_chunks(H, W)][7]
 * (written, then read by the combining launch; no zeroing needed). */
int bc_mask_stats_chunks(int H, int W);                       /* workgroups per mask; -1 if the mask is too large */
int bc_mask_stats(const float* logits, int n, int H, int W, float threshold, float offset, int* partial, int* out, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
