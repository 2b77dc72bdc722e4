/* Entry points for request batches whose requests run their OWN schedules (own step count, guidance scale, control window): the
 * per-image forms of the scheduler step, of the scaled input assemblies and of the time-embedding table of include/blobctrl_hip.h.
 * A header of its own beside that one; all four are recordable plan ops (BC_OP_SCHEDULER_STEP_REQUESTS .. BC_OP_TIMESTEP_EMBEDDING_ROWS
 * in the BC_OP_* table there, plan file version 8).  Tables are laid out per request: coef fp32 [B][nsteps][16], the column layout at
 * the top of blobctrl_amd/schedulers.py with column 15 = "this request has finished". */
#ifndef BLOBCTRL_REQUESTS_H
#define BLOBCTRL_REQUESTS_H
#include "blobctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The two scaled assemblies for a batch of edit REQUESTS that run their own schedules (own step counts, own sigmas): coef is fp32
 * [Blat][nsteps][16], one table per request, and image b of the output divides its noisy latents by column 14 of row *step_idx of table
 * b % Blat.  A row whose column 14 is 0 means "do not divide" (a finished request's row holds 1); a step index outside [0, nsteps)
 * gives the unscaled output, as the `_scaled` forms do. */
int bc_assemble_input_requests(const float* latents, int Blat, const float* img_lat, const float* score, const float* feat,
                               int Bimg, int F, int Bout, int h, int w, int Cpad, int dup_score, const float* coef, const int* step_idx,
                               int nsteps, bc_half* X, bc_stream stream);
int bc_assemble_input_im2col_requests(const float* latents, int Blat, const float* img_lat, const float* score, int Bimg, int Bout,
                                      int h, int w, int dup_score, const float* coef, const int* step_idx, int nsteps, bc_half* X,
                                      bc_stream stream);

/* One timestep per row: out [rows][dim], row r uses t_rows[r] (fp32 [rows]) and, when cond != NULL (fp32 [cond_rows][dim]), adds cond row
 * r % cond_rows.  The arithmetic is that of the table forms above (fp32 without cond, fp64 rounded once with it): the same t gives the
 * same bits.  The time-embedding table of a batch of edit requests with their own schedules, t_rows = [step][image]. */
int bc_timestep_embedding_rows(const float* t_rows, int rows, int dim, const float* cond, int cond_rows, bc_half* out, bc_stream stream);

/* The step of a batch of edit REQUESTS with their own tables: coef fp32 [B][nsteps][16], image b applies row *step_idx of table b - its
 * own coefficients and its own guidance scale (column 11, always read from the row).  Column 15 != 0 marks a request that has
 * finished: nothing of image b is read from eps and nothing of it is written (latents, the three hist slots and eps_out keep their
 * bits, whatever eps holds).  single != 0: eps is [B][h][2w][4] (a single-pass plan, no guidance arithmetic), else [2B][h][2w][4].
 * noise / third as in bc_scheduler_step_single (noise fp32 [nsteps][B][4][h][w]); a step index outside [0, nsteps) leaves every buffer
 * as it is and `advance` still counts. */
int bc_scheduler_step_requests(const float* eps, float* latents, const float* coef, int* step_idx, float* hist, int B, int h, int w,
                               const float* noise, int nsteps, int third, int single, float* eps_out, int advance, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
