/* AutoencoderTiny (TAESD) decoder: the 3x3 convolution of its five layer forms and the latent prologue (blobctrl_amd/tiny_vae.py;
 * D/models/autoencoders/autoencoder_tiny.py, vae.py:899-982 DecoderTiny, unet_2d_blocks.py AutoencoderTinyBlock).
 * A header of its own beside include/blobctrl_ip_mask.h.  Both entry points are recordable plan ops, recorded and replayed in-process only.
 * Conventions as in blobctrl_hip.h: fp16 activations, fp32 accumulation, all work on the caller's stream, 0 on success. */
#ifndef BLOBCTRL_TINY_VAE_H
#define BLOBCTRL_TINY_VAE_H
#include "blobctrl_ip_mask.h"

#ifdef __cplusplus
extern "C" {
#endif

/* An enum of its own: BC_OP_IP_MASK_END (56) closes include/blobctrl_ip_mask.h and stays refused by bc_plan_add_op. */
enum { BC_OP_TINY_CONV3X3 = BC_OP_IP_MASK_END + 1, BC_OP_TINY_LATENTS_IN, BC_OP_TINY_VAE_END };

/* Output modes of bc_tiny_conv3x3 */
enum {
    BC_TINY_OUT_F16 = 0,   /* fp16 NHWC [B][H][W][64]                                                  (Co = 64) */
    BC_TINY_OUT_IMAGE = 1, /* fp32 NCHW [B][3][H][W]: v = 2 y - 1                                       (Co = 3)  */
    BC_TINY_OUT_U8 = 2     /* uint8 [B][H][W][3]: round_half_even(clamp(v / 2 + 0.5, 0, 1) * 255)       (Co = 3)  */
};

/* One 3x3, pad-1, stride-1 convolution: y[b, oy, ox, co] = bias[co] + sum_{ky, kx, ci} w[co][ky][kx][ci] * x'[b, oy + ky - 1, ox + kx - 1, ci],
 * x' zero outside the H x W output domain.  H x W is the OUTPUT size; with up == 0 the input has the same size and x' = x, with up != 0 the
 * input is [B][H / 2][W / 2][Ci] (H and W even) and x'[b, y, x] = x[b, y >> 1, x >> 1]: the nearest-2x upsample applied on the read, the
 * zero padding applied in the upsampled domain.
 *   x      fp16 NHWC, dense (pixel stride Ci), 16-byte aligned.  Ci = 8 or 64.
 *   w      fp16 [Co'][3][3][Ci] (weights.pack_conv3x3), 16-byte aligned; Co' = 64 with Co = 64, Co' = 8 with Co = 3 (rows 3 .. 7 are padding
 *          of the weights only and never reach an output).
 *   bias   fp32 [Co], or null (no bias).
 *   skip   fp16 [B][H][W][64] added in fp32 before the ReLU, or null; Co = 64 only.
 *   relu   != 0: max(., 0) last, before the rounding to fp16; Co = 64 only.
 *   out    out_mode BC_TINY_OUT_F16 with Co = 64 (16-byte aligned), BC_TINY_OUT_IMAGE (4-byte aligned) or BC_TINY_OUT_U8 with Co = 3.
 *          In the uint8 mode v is formed first and then every operation runs in fp32 in the order written above: the multiplications and
 *          divisions by 2 are exact, so the bytes are those of the fp32 image quantised the same way.
 * The five forms of the decoder: in (Ci 8, bias, relu), block a / b (bias, relu), block c (bias, skip, relu), up (up, no bias), out (Co 3).
 * Refused: Ci = 8 with up or skip; Co = 3 with Ci = 8, up, skip or relu; a Co and an out_mode that do not go together; an odd H or W with up.
 * Arbitrary B, H, W >= 1; nothing outside x's B * Hin * Win * Ci elements, w, bias and skip is
 * read, nothing outside the B * H * W * Co outputs is written.  `skip` and `x` may not overlap `out`. */
typedef struct bc_tiny_conv_args {
    const bc_half* x;
    const bc_half* w;
    const float* bias;
    const bc_half* skip;
    void* out;
    int B, H, W;
    int Ci, Co;
    int up, relu, out_mode;
} bc_tiny_conv_args;

int bc_tiny_conv3x3(const bc_tiny_conv_args* args, bc_stream stream);

/* The same launch with its arguments flat, in the struct's order: the form the plan runtime records (BC_OP_TINY_CONV3X3). */
int bc_tiny_conv3x3_flat(const bc_half* x, const bc_half* w, const float* bias, const bc_half* skip, void* out, int B, int H, int W, int Ci,
                         int Co, int up, int relu, int out_mode, bc_stream stream);

/* z fp32 NCHW [B][4][h][w] -> fp16 NHWC [B][h][w][8]: channels 0 .. 3 = tanh(z / 3) * 3 (vae.py:963), channels 4 .. 7 = +0.
 * out 16-byte aligned.  BC_OP_TINY_LATENTS_IN. */
int bc_tiny_latents_in(const float* z, int B, int h, int w, bc_half* out, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
