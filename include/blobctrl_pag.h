/* Perturbed-attention guidance (PAG; D/pipelines/pag/pag_utils.py, PAGCFGIdentitySelfAttnProcessor2_0 / PAGIdentitySelfAttnProcessor2_0
 * in D/models/attention_processor.py): the identity "attention" of the perturbed images and the guidance + scheduler step of a PAG plan.
 * A header of its own beside include/blobctrl_tiny_vae.h.  Both entry points are recordable plan ops, recorded and replayed in-process only.
 * Conventions as in blobctrl_hip.h: fp16 activations, fp32 latents and tables, all work on the caller's stream, 0 on success. */
#ifndef BLOBCTRL_PAG_H
#define BLOBCTRL_PAG_H
#include "blobctrl_tiny_vae.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An enum of its own: BC_OP_TINY_VAE_END (59) closes include/blobctrl_tiny_vae.h and stays refused by bc_plan_add_op. */
enum { BC_OP_ATTENTION_IDENTITY = BC_OP_TINY_VAE_END + 1, BC_OP_PAG_SCHEDULER_STEP, BC_OP_PAG_END };

/* The self-attention of a perturbed image is the identity map on its values: out[b * HW + p][c] = vt[b][c][p] for images b in [b0, B),
 * tokens p in [0, HW), channels c in [0, C) - a transpose copy, every stored value bit-equal to the fp16 V element.
 *   vt   fp16 [B][C][ldvt], the V^T every self-attention path produces (batch stride C * ldvt); ldvt >= HW, ldvt % 8 == 0.  Its pad
 *        columns HW .. ldvt may be read and are never stored anywhere.
 *   out  fp16 [B * HW][ldo], ldo >= C, ldo % 8 == 0: rows [b0 * HW, B * HW), columns [0, C) are written; no row of an image < b0 and no
 *        column >= C is touched.
 *   C % 8 == 0, 0 <= b0 <= B (b0 == B: nothing to do), both pointers 16-byte aligned.  In a PAG layer bc_attention runs on the first b0
 *   images of the same buffers.  BC_OP_ATTENTION_IDENTITY. */
int bc_attention_identity(const bc_half* vt, bc_half* out, int B, int b0, int HW, int C, int ldvt, int ldo, bc_stream stream);

/* The step of a PAG plan: crop, guidance and scheduler step of bc_scheduler_step_requests' body (one table: coef fp32 [nsteps][16]) with
 * the perturbed-attention term, s = pag_table[*step_idx], pag_table fp32 [nsteps]:
 *   single == 0: eps token-major [3B][h][2w][4] = [uncond | cond | perturbed], e = e_u + g * (e_c - e_u) + s * (e_c - e_p), g = column 11
 *                of the current coef row;
 *   single != 0: eps [2B][h][2w][4] = [cond | perturbed], e = e_c + s * (e_c - e_p); column 11 is not read.
 * Evaluated in fp32 in the written order, then the unchanged step arithmetic.  noise != NULL adds cf[12] * noise[step] (fp32
 * [nsteps][B][4][h][w]), third != 0 adds cf[13] * x0_{i-2}; a step index outside [0, nsteps) leaves every buffer as it is.
 * BC_OP_PAG_SCHEDULER_STEP. */
int bc_pag_scheduler_step(const float* eps, float* latents, const float* coef, int* step_idx, float* hist, const float* pag_table, int B,
                          int h, int w, const float* noise, int nsteps, int third, int single, float* eps_out, int advance,
                          bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
