/* Masked edits (the four-channel inpainting path of D/pipelines/stable_diffusion/pipeline_stable_diffusion_inpaint.py:1272-1285): after
 * every scheduler step the latents outside the mask are replaced by the original image's latents, noised to the next timestep.  The step
 * of a blend plan and the mask at latent resolution.  A header of its own beside include/blobctrl_pag.h.  Both entry points are
 * recordable plan ops, recorded and replayed in-process only.
 * Conventions as in blobctrl_hip.h: fp32 latents and tables, all work on the caller's stream, 0 on success. */
#ifndef BLOBCTRL_BLEND_H
#define BLOBCTRL_BLEND_H
#include "blobctrl_pag.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An enum of its own: BC_OP_PAG_END (62) closes include/blobctrl_pag.h and stays refused by bc_plan_add_op. */
enum { BC_OP_BLEND_SCHEDULER_STEP = BC_OP_PAG_END + 1, BC_OP_BLEND_MASK, BC_OP_BLEND_END };

/* The step of a blend plan: bc_pag_scheduler_step's crop, guidance and scheduler step (one table: coef fp32 [nsteps][16], the guidance
 * scale in column 11), then, last - behind the noise and third-order terms, which are part of the scheduler step's result -
 *     p  = a * image[i] + s * bnoise[i]             (a, s) = blend_table[*step_idx], fp32 [nsteps][2]
 *     x' = (1 - m) * p + m * x'                     m = mask[b][y][x], one value for the 4 channels of a latent pixel
 * evaluated in fp32, rounded operation by operation in the written order: where m == 0 the stored value is exactly a * image + s *
 * bnoise, where m == 1 exactly what the step without the blend stores.  hist and eps_out hold what they hold without the blend.
 *   pag_table  fp32 [nsteps], or NULL for no perturbed-attention term: eps then holds [uncond | cond] (2B images), or with single != 0
 *              the B images themselves, as bc_cfg_scheduler_step / bc_scheduler_step_single read them
 *   image      fp32 [B][4][h][w], the latents to keep     bnoise  fp32 [B][4][h][w], the edit's start noise (before init_noise_sigma)
 *   mask       fp32 [B][h][w], 1 = repaint, 0 = keep; values between blend
 * noise, third, single as in bc_pag_scheduler_step; a step index outside [0, nsteps) leaves every buffer as it is.
 * BC_OP_BLEND_SCHEDULER_STEP. */
int bc_blend_scheduler_step(const float* eps, float* latents, const float* coef, int* step_idx, float* hist, const float* pag_table,
                            const float* image, const float* bnoise, const float* mask, const float* blend_table, int B, int h, int w,
                            const float* noise, int nsteps, int third, int single, float* eps_out, int advance, bc_stream stream);

/* A uint8 mask at image resolution to the fp32 mask of the step: out[i][y][x] = mask[i][8y][8x] >= 128 ? 1 : 0 - the reference's
 * mask_processor (do_binarize: 0.5 of [0, 1]) followed by prepare_mask_latents' nearest F.interpolate, which reads the top-left pixel of
 * every 8 x 8 cell.  mask uint8 [n][H][W] with H % 8 == 0 and W % 8 == 0, out fp32 [n][H / 8][W / 8].  BC_OP_BLEND_MASK. */
int bc_blend_mask(const unsigned char* mask, float* out, int n, int H, int W, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
