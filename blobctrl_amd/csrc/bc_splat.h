// The per-pixel Gaussian-blob score, shared by every rasteriser kernel (elementwise.hip: splat_kernel, blobviz.hip:
// splat_maps_kernel) so that their results agree bit for bit.
#pragma once
#include "bc_common.h"

// 8 doubles per blob image: xs, ys, cov00, cov01, cov10, cov11, size, unused.  Travels as a kernel argument.
struct SplatParams { double v[16 * 8]; };

// blobctrl/utils/utils.py:120-135 / 145-172 for one blob per image, fp64 like the reference (numpy float64 -> torch float64).
//   delta = (grid - mu*(W,H)) / (W,H) ; m = delta^T cov^-1 delta ; s = min(1, 2*sigmoid(-m)) ; s = 1e-6f if size < 0.5
__device__ __forceinline__ double bc_splat_score(const double* p, int gx, int gy, int h, int w) {
    const double xs = p[0], ys = p[1], a = p[2], b = p[3], c = p[4], d = p[5], size = p[6];
    const double dx = ((double)gx - xs * (double)w) / (double)w;      // ut:151-153
    const double dy = ((double)gy - ys * (double)h) / (double)h;
    // solve [[a b][c d]] z = delta  (ut:156, torch.linalg.solve = LU with partial pivoting)
    double z0, z1;
    if (fabs(a) >= fabs(c)) {
        const double f = c / a;
        const double u = d - f * b;
        z1 = (dy - f * dx) / u;
        z0 = (dx - b * z1) / a;
    } else {
        const double f = a / c;
        const double u = b - f * d;
        z1 = (dx - f * dy) / u;
        z0 = (dy - d * z1) / c;
    }
    const double m = dx * z0 + dy * z1;
    double s = 1.0 / (1.0 + exp(m));                                  // sigmoid(-m)  ut:162
    s = fmin(2.0 * s, 1.0);                                           // ut:163
    if (size < 0.5) s = (double)1e-6f;                                // ut:165-172 (float32 constant in the reference)
    return s;
}
