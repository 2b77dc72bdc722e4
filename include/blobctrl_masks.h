/* Connected components of binary masks and the small-region removal on top of them (blobctrl_amd/masks.py): what turns a raw SAM mask
 * into one blob - `segment_anything.utils.amg.remove_small_regions` without the trip to the host.  A header of its own beside
 * blobctrl_sam.h.  These entry points are DIRECT launches on the caller's stream: they are not recordable plan ops, have no BC_OP_* code and
 * never appear in a .bcplan file.  Everything is integer arithmetic: results are exact and do not depend on how a launch splits an image
 * over workgroups or in which order workgroups run.  0 on success, 1 on bad arguments (bc_last_error(); nothing is launched then).
 *
 * How it runs (csrc/mask_regions.hip): (1) every 32 x 64 tile is labelled by one workgroup in LDS - a union-find whose links only ever point
 * to a smaller index, so the root of a component is its minimum - and written as global raster indices; (2) the pixels on tile borders
 * merge the tiles' trees with agent-scope atomic minima; (3) every pixel is replaced by its root.  A launch boundary is the only
 * synchronisation between the phases; no workgroup waits for another. */
#ifndef BLOBCTRL_MASKS_H
#define BLOBCTRL_MASKS_H
#include "blobctrl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* labels[k][i] = the smallest raster index y * W + x of the 8-connected component that pixel i of mask k belongs to, among the pixels
 * with (mask != 0) == (fg != 0); -1 for the other pixels.  masks uint8 / bool bytes [n][H][W] (any base alignment), labels int32
 * [n][H][W]; H * W < 2^31.  Masks never mix: the last pixel of mask k and the first of mask k + 1 are no neighbours, nor are column W - 1
 * and column 0 of the next row. */
int bc_mask_label(const unsigned char* masks, int n, int H, int W, int fg, int* labels, bc_stream stream);

/* segment_anything.utils.amg.remove_small_regions on n masks, in place.  mode 0 = "holes": every 8-connected component of ZERO pixels with
 * fewer than area_thresh pixels is set (to 1).  mode 1 = "islands": every 8-connected component of SET pixels with fewer than area_thresh
 * pixels is cleared; if that would clear every component of a non-empty mask, the largest one stays (ties: the one whose first pixel in
 * raster order comes first).  The comparison is strict (area < area_thresh).  labels, areas: int32 scratch [n][H][W] each (no zeroing by
 * the caller; both are overwritten).  out int32 [n][6] = changed (0 / 1), then area, x0, y0, x1, y1 (inclusive box, 0 0 0 0 when empty) of
 * the mask AS IT LEAVES.  `changed` is the package's flag: 1 when the mask has a component below the threshold in the colour the mode
 * works on - which, in mode 1, includes a lone speck that then stays as "the largest". */
int bc_mask_remove_small(unsigned char* masks, int n, int H, int W, int area_thresh, int mode, int* labels, int* areas, int* out,
                         bc_stream stream);

/* One launch group of bc_mask_remove_small on the same arguments, for measuring where its time goes (tools/mask_regions_probe.py): phase
 * 0 = tile labelling (with the tiles' own pixel counts), 1 = border merge, 2 = flatten + component areas, 3 = the per-mask reduction over
 * roots (largest component, any small one), 4 = apply + the statistics of `out`.  Running phases 0 .. 4 in order IS bc_mask_remove_small;
 * a phase on its own is meaningful only after the ones before it (it reads what they left in labels, areas and out; on scratch that holds
 * anything else the indices it follows are not checked).  A MEASURING AID, outside the compatibility promise of the two entry points above:
 * the phases, their number and what each leaves in the scratch arrays may change with the implementation. */
#define BC_MASK_REGION_PHASES 5
int bc_mask_remove_small_phase(unsigned char* masks, int n, int H, int W, int area_thresh, int mode, int* labels, int* areas, int* out,
                               int phase, bc_stream stream);

#ifdef __cplusplus
}
#endif
#endif
