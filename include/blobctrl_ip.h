/* Entry point of the IP-Adapter path: the decoupled image cross-attention that follows the text cross-attention of every attn2
 * (IPAdapterAttnProcessor2_0, D/models/attention_processor.py:3851-3868: hidden_states + scale * ip_hidden_states in front of to_out).
 * A header of its own beside include/blobctrl_hip.h.  The launch is a recordable plan op; like the SAM ops it is recorded and replayed
 * in-process only and never written to a .bcplan file.
 * Conventions as in blobctrl_hip.h: fp16 activations, fp32 accumulation, all work on the caller's stream, 0 on success. */
#ifndef BLOBCTRL_IP_H
#define BLOBCTRL_IP_H
#include "blobctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Extension headers continue the BC_OP_* numbering from the base header's BC_OP_COUNT; that enum itself is closed. */
enum { BC_OP_ATTENTION_IP = BC_OP_COUNT, BC_OP_IP_END };

#define BC_ATTENTION_IP_MAX_T 64

/* O[b, r, h * d + j] += w * sum_t softmax_t(qk_scale * <Q[b, r, h, :], K[b, t, h, :]>) * V[b, t, h * d + j],   in place on O.
 *   Q fp16 [B * rows_per_batch][ldq]   (a strided view is fine: only the first C = heads * d columns of a row are read)
 *   K, V fp16 [B][T][ldkv]             row-major per image, NO transposed V; 1 <= T <= BC_ATTENTION_IP_MAX_T
 *   O fp16 [B * rows_per_batch][ldo]   read as fp16, summed in fp32 with the attention result, rounded once at the store
 *   d in {8, 16, 32, 40, 64, 80, 160}  (the head sizes of bc_attention); ldq, ldkv, ldo >= C and multiples of 8; 16-byte aligned bases
 *   w                                  ONE fp32 read on the device: a captured graph follows set_ip_adapter_scale without re-recording.
 *                                      With *w == 0 the launch returns without reading or writing O (the reference skips such an adapter).
 * Scores, softmax and the sum over t are fp32.  Q and O are touched once, 16 bytes per lane; K and V of the image sit in LDS. */
int bc_attention_ip(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d, int T,
                    int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream);

/* Two kernels stand behind bc_attention_ip, with one contract (every word above holds for both):
 *   path 0   the scalar kernel: lanes along channels, keys four at a time through shuffle reductions; any T.  Made for T = 4.
 *   path 1   MFMA tiles: a wave owns 16 query rows of one head, scores and P.V by v_mfma; T = 16, 32, 48 or 64 only.
 * bc_attention_ip_path names the path bc_attention_ip runs for a shape - a table of measured classes (profiles/ip_adapter_plus.md); it is 0
 * for every T that is not a multiple of 16.  bc_attention_ip_with launches the named path: bc_attention_ip(...) is
 * bc_attention_ip_with(bc_attention_ip_path(d, T, rows_per_batch, heads), ...).  Path 1 with another T, or a path other than 0 and 1, is an
 * argument error before any launch.  Plain entry points for measurements and tests: NOT plan ops, no BC_OP_* code. */
int bc_attention_ip_path(int d, int T, int rows_per_batch, int heads);
int bc_attention_ip_with(int path, const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d,
                         int T, int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
