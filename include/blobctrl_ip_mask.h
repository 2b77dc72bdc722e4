/* IP-Adapter masks: an image prompt confined to a region, per image (cross_attention_kwargs={"ip_adapter_masks": ...};
 * IPAdapterAttnProcessor2_0, D/models/attention_processor.py:3776-3849, and IPAdapterMaskProcessor.downsample, D/image_processor.py:969-1029).
 * A header of its own beside include/blobctrl_ip.h.  bc_attention_ip_masked is a recordable plan op, recorded and replayed in-process only
 * like bc_attention_ip; bc_ip_mask_downsample is a direct launch on the caller's stream.
 * Conventions as in blobctrl_hip.h: fp16 activations, fp32 accumulation, all work on the caller's stream, 0 on success. */
#ifndef BLOBCTRL_IP_MASK_H
#define BLOBCTRL_IP_MASK_H
#include "blobctrl_ip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An enum of its own: BC_OP_IP_END (54) closes include/blobctrl_ip.h and stays refused by bc_plan_add_op. */
enum { BC_OP_ATTENTION_IP_MASKED = BC_OP_IP_END + 1, BC_OP_IP_MASK_END };

/* O[b, r, h * d + j] += w * sum_i m[i, r] * sum_t softmax_t(qk_scale * <Q[b, r, h, :], K[b, i * Tp + t, h, :]>) * V[b, i * Tp + t, h * d + j]
 *     i = 0 .. images - 1,   t = 0 .. Tp - 1 (Tp = tokens_per_image),   images * Tp <= BC_ATTENTION_IP_MAX_T,   in place on O.
 * Not bc_attention_ip times a mask: every image has a softmax of ITS OWN over its Tp keys, where bc_attention_ip runs one softmax over
 * all images * Tp keys.
 *   Q, K, V, O, ldq, ldkv, ldo, d, qk_scale, w   as for bc_attention_ip (T = images * Tp rows of K and V per batch element), every rule:
 *                                      in place on O, *w == 0 returns before anything is read, strided Q, nothing outside the view is
 *                                      touched, O read as fp16, summed in fp32, rounded once at the store.
 *   mask fp16 [images][ldm]            m[i, r] for the rows_per_batch query rows of ONE batch element, shared by every batch element (the
 *                                      reference repeats one mask over the batch); ldm >= rows_per_batch; 2-byte aligned.  Any value: the
 *                                      bicubic downsampling of bc_ip_mask_downsample overshoots [0, 1].
 * The weight of image i on row r, m[i, r] / (the softmax denominator of image i), is formed in fp32 and meets the fp32 sum of
 * probabilities x V of that image before anything is rounded; no per-image result exists in fp16.
 * A query row whose mask is exactly zero (+0 or -0) for every image is neither read from Q nor touched in O, and a workgroup whose whole
 * row block is such rows returns before it stages K and V. */
int bc_attention_ip_masked(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d,
                           int images, int tokens_per_image, int ldq, int ldkv, int ldo, float qk_scale, const float* w, const bc_half* mask,
                           int ldm, bc_stream stream);

/* The kernels behind bc_attention_ip_masked by name, as bc_attention_ip_path / bc_attention_ip_with name those of bc_attention_ip:
 *   path 0   the scalar kernel: its online softmax runs once per image; any Tp.
 *   path 1   MFMA tiles: Tp = 16, 32, 48 or 64 only.  A 16-key tile belongs to one image; the tiles of an image normalise together and the
 *            mask value of the lane's row scales P in front of the P.V product.  Path 1 with another Tp is an argument error.
 * bc_attention_ip_masked_path names the path bc_attention_ip_masked runs: bc_attention_ip_path's measured classes at images x Tp keys
 * where Tp is a multiple of 16, 0 everywhere else (profiles/ip_adapter_masks.md).
 * Plain entry points for measurements and tests: NOT plan ops, no BC_OP_* code. */
int bc_attention_ip_masked_path(int d, int images, int tokens_per_image, int rows_per_batch, int heads);
int bc_attention_ip_masked_with(int path, const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads,
                                int d, int images, int tokens_per_image, int ldq, int ldkv, int ldo, float qk_scale, const float* w,
                                const bc_half* mask, int ldm, bc_stream stream);

/* IPAdapterMaskProcessor.downsample for one attention level: F.interpolate(mask, size=(mask_h, mask_w), mode="bicubic") - align_corners
 * False, no antialiasing, A = -0.75, source indices clamped at the borders, overshoot outside [0, 1] kept - flattened to rows.
 *   mask   fp32 (is_u8 == 0) or uint8 (is_u8 != 0; the byte's value is the mask's value) [images][H][W], dense
 *   out    fp16 [images][ldo]: out[i][r] = the interpolated value for r < mask_h * mask_w, +0 for mask_h * mask_w <= r < rows;
 *          ldo >= rows, mask_h * mask_w <= rows.  Columns from `rows` on are not touched.
 * The host chooses mask_h and mask_w (the reference's formula: blobctrl_amd.ip_masks.mask_grid).  Taps and weights are computed in double:
 * the launch runs once per edit and level.  A direct launch: NOT a plan op, no BC_OP_* code. */
int bc_ip_mask_downsample(const void* mask, int is_u8, int images, int H, int W, int mask_h, int mask_w, int rows, bc_half* out, int ldo,
                          bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
