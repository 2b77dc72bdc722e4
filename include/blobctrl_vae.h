/*
 * blobctrl_vae.h  --  C ABI of the tiled-VAE helpers of libblobctrl_hip.so (MI355X, gfx950).
 *
 * Same conventions as blobctrl_hip.h: plain C, device pointers, int status (0 = ok, bc_last_error() has the message), the caller's
 * hipStream_t last, no allocation and no synchronisation.  These entry points are NOT recordable plan ops: a tiled encode / decode is
 * driven from the host (one cached plan per tile shape, one blend launch per tile), so they live outside blobctrl_hip.h and outside
 * the BC_OP_* table.
 */
#ifndef BLOBCTRL_VAE_H
#define BLOBCTRL_VAE_H

#include "blobctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Layout of one tile's source and of the stitched result. */
enum {
    BC_VAE_TILE_DECODE = 0,  /* src fp32 NHWC [B][th][tw][3] (a decode plan's image);   out fp32 NCHW [B][3][H][W]            */
    BC_VAE_TILE_ENCODE = 1   /* src fp16 NHWC [B][th][tw][8] (an encode plan's moments); out fp16 NHWC [B][H*W][8]            */
};

/* ---------------------------------------------------------------------------------------------------------------
 * Blend one tile with its neighbours, keep it, and scatter its cropped part into the result.
 * Replaces: blend_v / blend_h and the crop + torch.cat of tiled_encode / tiled_decode
 *           (D/models/autoencoders/autoencoder_kl.py:328-338, 374-387, 425-438).
 * Tiles are processed in row-major order; for the element (b, y, x, c) of the tile, in fp32:
 *   v = src[b][y][x][c]
 *   if (above && y < ev)  v = above[b][ha - ev + y][x][c] * (1 - y / ev) + v * (y / ev)
 *   if (left  && x < eh)  v = left[b][y][wl - eh + x][c] * (1 - x / eh) + v * (x / eh)
 *   keep[b][y][x][c] = v                                         (what later neighbours read as `above` / `left`)
 *   if (y < ch && x < cw) out[b, oy + y, ox + x, c] = v          (in the layout of `mode`)
 * The weights are formed in double and rounded to fp32 once; each product and the sum round to fp32 (no fused multiply-add): the
 * arithmetic of the reference's `a * (1 - y / e) + b * (y / e)` on fp32 tensors.
 *   above : the kept tile of the previous tile row, fp32 NHWC [B][ha][tw][C] (same width as this tile), or NULL
 *   left  : the kept tile to the left,               fp32 NHWC [B][th][wl][C] (same height as this tile), or NULL
 *   keep  : fp32 NHWC [B][th][tw][C]
 *   ev, eh: blend extents, already clamped by the caller: 0 <= ev <= min(ha, th), 0 <= eh <= min(wl, tw); ignored without a neighbour
 *   (oy, ox), (ch, cw): origin of the tile in the result and the cropped size written there: ch <= th, cw <= tw, inside [H][W]
 * All buffers 16-byte aligned; `keep` and `out` overlap nothing else.  Refused (return 1) before anything is launched otherwise.
 * --------------------------------------------------------------------------------------------------------------- */
int bc_vae_tile_blend(const void* src, const float* above, const float* left, float* keep, void* out, int mode, int B, int th, int tw,
                      int ha, int wl, int ev, int eh, int oy, int ox, int ch, int cw, int H, int W, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
