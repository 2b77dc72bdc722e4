// The inputs of an edit on the device (include/blobctrl_edit.h): filled ellipses, row extents of masks, the object cut-out.  gfx950.
//
//   ei_cover     `blob_edit.ellipse_mask` per pixel.  The predicate below is that function's arithmetic, expression by expression, in
//                fp64 with contraction OFF: numpy rounds after every multiply and every add, and a fused multiply-add would round once
//                where it rounds twice.  Division is `/` (correctly rounded without fast-math), cos and sin come from the host.  The one
//                liberty taken is the order of EVALUATION, never of arithmetic: a pixel whose centre is inside the ellipse, or that
//                holds the ellipse's centre, is covered whatever the edge passes say, so they are skipped for it.
//   ei_paint     the same predicate for k ellipses of a pixel, walked from the last ellipse to the first: the last one that covers the
//                pixel decides its colour, so the walk stops at the first hit.
//   ei_extents   first / last set column of every mask row.  A wave takes a row, or one of 2 or 4 chunks of a wide row: byte loads up to
//                the first 16-byte boundary, 16-byte loads while a whole vector fits, byte loads for the rest; min / max over the wave
//                by shuffles and over the chunks of a row through LDS.  Integer, no atomics, every output word written exactly once.
//   ei_cutout    `blob_edit.object_region_from_mask`: one thread per output pixel.
#include "bc_common.h"
#include "../../include/blobctrl_edit.h"

// numpy does not contract a * b + c; neither may this file (the default for device code is to contract)
#pragma clang fp contract(off)

namespace {

constexpr int EI_THREADS = 256;
constexpr int EI_PER = 4;                             // pixels per thread in ei_cover (one 32-bit store where the address allows it)
constexpr int EI_WAVES = EI_THREADS / 64;

struct Ellipse6 { double xc, yc, a, b, ct, st; };

__device__ __forceinline__ Ellipse6 ei_load(const double* __restrict__ e) { return {e[0], e[1], e[2], e[3], e[4], e[5]}; }

// image offset from the ellipse centre -> unit-disc coordinates (u along the first axis, v along the second)
__device__ __forceinline__ void ei_to_disc(const Ellipse6& e, double x, double y, double& u, double& v) {
#pragma clang fp contract(off)
    u = (x * e.ct + y * e.st) / e.a;
    v = (-x * e.st + y * e.ct) / e.b;
}

// np.minimum / np.maximum: a NaN operand gives NaN (fmin / fmax would drop it), so an ellipse that overflows decides as on the host
__device__ __forceinline__ double ei_min(double a, double b) { return a != a ? a : b != b ? b : a < b ? a : b; }
__device__ __forceinline__ double ei_max(double a, double b) { return a != a ? a : b != b ? b : a > b ? a : b; }

// the squared distance from the origin to the segment p -> q, as `ellipse_mask` computes it
__device__ __forceinline__ double ei_edge(double pu, double pv, double qu, double qv) {
#pragma clang fp contract(off)
    const double eu = qu - pu, ev = qv - pv;
    const double tt = ei_min(ei_max(-(pu * eu + pv * ev) / ei_max(eu * eu + ev * ev, 1e-300), 0.0), 1.0);
    const double du = pu + tt * eu, dv = pv + tt * ev;
    return du * du + dv * dv;
}

// does the closed pixel square centred at (x, y) meet the filled ellipse?
__device__ __forceinline__ bool ei_covers(const Ellipse6& e, int x, int y) {
#pragma clang fp contract(off)
    const double X = (double)x - e.xc, Y = (double)y - e.yc;
    double cu, cv;
    ei_to_disc(e, X, Y, cu, cv);
    if (cu * cu + cv * cv <= 1.0) return true;                           // the pixel centre is inside
    if (fabs(X) <= 0.5 && fabs(Y) <= 0.5) return true;                   // the ellipse centre is in the pixel square
    double u0, v0, u1, v1, u2, v2, u3, v3;
    ei_to_disc(e, X + -0.5, Y + -0.5, u0, v0);
    ei_to_disc(e, X + 0.5, Y + -0.5, u1, v1);
    ei_to_disc(e, X + 0.5, Y + 0.5, u2, v2);
    ei_to_disc(e, X + -0.5, Y + 0.5, u3, v3);
    double best = ei_edge(u0, v0, u1, v1);
    best = ei_min(best, ei_edge(u1, v1, u2, v2));
    best = ei_min(best, ei_edge(u2, v2, u3, v3));
    best = ei_min(best, ei_edge(u3, v3, u0, v0));
    return best <= 1.0;
}

__global__ __launch_bounds__(EI_THREADS) void ei_cover_kernel(const double* __restrict__ ell, int W, int HW, int chunks,
                                                              unsigned char* __restrict__ mask) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p0 = (c * EI_THREADS + (int)threadIdx.x) * EI_PER;          // < HW + 1024 <= 2^28 + 1024
    if (p0 >= HW) return;
    const Ellipse6 e = ei_load(ell + (long long)i * 6);
    unsigned char* dst = mask + (long long)i * HW + p0;
    int y = p0 / W, x = p0 - y * W;
    const int cnt = min(EI_PER, HW - p0);
    unsigned v = 0;
    for (int j = 0; j < cnt; ++j) {
        if (ei_covers(e, x, y)) v |= 255u << (8 * j);
        if (++x == W) { x = 0; ++y; }
    }
    if (cnt == EI_PER && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        *reinterpret_cast<unsigned*>(dst) = v;
    } else {
        for (int j = 0; j < cnt; ++j) dst[j] = (unsigned char)(v >> (8 * j));
    }
}

__global__ __launch_bounds__(EI_THREADS) void ei_paint_kernel(unsigned char* __restrict__ images, int W, int HW, int chunks,
                                                              const double* __restrict__ ell, const unsigned char* __restrict__ rgb, int k) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p = c * EI_THREADS + (int)threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    for (int j = k - 1; j >= 0; --j) {                                     // the last ellipse that covers the pixel wins
        const long long ej = (long long)i * k + j;
        if (!ei_covers(ei_load(ell + ej * 6), x, y)) continue;
        unsigned char* dst = images + ((long long)i * HW + p) * 3;
        const unsigned char* col = rgb + ej * 3;
        dst[0] = col[0]; dst[1] = col[1]; dst[2] = col[2];
        return;
    }
}

// first / last non-zero byte of a little-endian word holding columns x .. x + 3
__device__ __forceinline__ void ei_word(unsigned w, int x, int& lo, int& hi) {
    if (w == 0) return;
    lo = min(lo, x + ((__ffs((int)w) - 1) >> 3));
    hi = max(hi, x + ((31 - __clz((int)w)) >> 3));
}

// A workgroup of EI_WAVES waves takes EI_WAVES / wpr rows; wave w takes chunk w % wpr of row w / wpr, columns [chunk * span, + span) of W.
__global__ __launch_bounds__(EI_THREADS) void ei_extents_kernel(const unsigned char* __restrict__ masks, long long rows, int W, int wpr, int span,
                                                                int* __restrict__ out) {
    __shared__ int part[EI_WAVES][2];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int chunk = wave % wpr;
    const long long row = (long long)blockIdx.x * (EI_WAVES / wpr) + wave / wpr;
    int lo = 0x7fffffff, hi = -1;
    if (row < rows) {
        const unsigned char* src = masks + row * W;
        const int c0 = min(W, chunk * span), c1 = min(W, c0 + span);
        // [c0, a0) up to the first 16-byte boundary, [a0, a1) whole vectors, [a1, c1) the rest: both ragged ends are under 16 bytes
        const int a0 = min(c1, c0 + (int)((16 - (reinterpret_cast<uintptr_t>(src + c0) & 15)) & 15));
        const int a1 = a0 + ((c1 - a0) & ~15);
        if (lane < 16) {
            const int x = c0 + lane;
            if (x < a0 && src[x]) { lo = min(lo, x); hi = max(hi, x); }
        } else if (lane < 32) {
            const int x = a1 + lane - 16;
            if (x < c1 && src[x]) { lo = min(lo, x); hi = max(hi, x); }
        }
        for (int x = a0 + lane * 16; x < a1; x += 64 * 16) {
            const uint4 v = bc_ld16(src + x);
            ei_word(v.x, x, lo, hi); ei_word(v.y, x + 4, lo, hi); ei_word(v.z, x + 8, lo, hi); ei_word(v.w, x + 12, lo, hi);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d, 64));
            hi = max(hi, __shfl_xor(hi, d, 64));
        }
    }
    if (lane == 0) { part[wave][0] = lo; part[wave][1] = hi; }
    __syncthreads();
    if (row < rows && chunk == 0 && lane == 0) {
        for (int j = 1; j < wpr; ++j) { lo = min(lo, part[wave + j][0]); hi = max(hi, part[wave + j][1]); }
        out[row * 2] = hi < 0 ? -1 : lo;
        out[row * 2 + 1] = hi;
    }
}

__global__ __launch_bounds__(EI_THREADS) void ei_cutout_kernel(const unsigned char* __restrict__ image, const unsigned char* __restrict__ masks,
                                                               const int* __restrict__ boxes, int H, int W, int HW, int chunks,
                                                               unsigned char* __restrict__ out) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p = c * EI_THREADS + (int)threadIdx.x;
    if (p >= HW) return;
    const int Y = p / W, X = p - Y * W;
    const int* box = boxes + (long long)i * 4;
    const int bx = box[0], by = box[1], bw = box[2], bh = box[3];
    // the box lands at ((H - h) // 2, (W - w) // 2); this output pixel shows source pixel (sy, sx) when that lies in the box AND in the frame
    const long long sy = (long long)Y - ((long long)H - bh) / 2 + by, sx = (long long)X - ((long long)W - bw) / 2 + bx;
    unsigned char r = 255, g = 255, b = 255;
    if (bw > 0 && bh > 0 && sy >= by && sy < (long long)by + bh && sx >= bx && sx < (long long)bx + bw && sy >= 0 && sy < H && sx >= 0 && sx < W) {
        const long long s = sy * W + sx;
        if (masks[(long long)i * HW + s]) {
            const unsigned char* px = image + s * 3;
            r = px[0]; g = px[1]; b = px[2];
        }
    }
    unsigned char* dst = out + ((long long)i * HW + p) * 3;
    dst[0] = r; dst[1] = g; dst[2] = b;
}

struct EditGeom {
    int HW, chunks;                                    // chunks of EI_THREADS threads per image
};

// everything a launch below relies on; 1 with bc_last_error() set when the arguments are bad
int ei_geometry(const char* who, int n, int H, int W, int per_thread, EditGeom& g) {
    BC_CHECK_ARG(n > 0 && H > 0 && W > 0, "%s: bad args (n, H, W <= 0)", who);
    BC_CHECK_ARG(H <= BC_EDIT_MAX_DIM && W <= BC_EDIT_MAX_DIM, "%s: a frame of %d x %d exceeds the limit of %d a side", who, H, W, BC_EDIT_MAX_DIM);
    g.HW = H * W;
    g.chunks = bc_ceil_div(g.HW, (long long)EI_THREADS * per_thread);
    BC_CHECK_ARG((long long)n * g.chunks <= 0x7fffffffll, "%s: %d frames of %d x %d exceed the grid", who, n, H, W);
    return 0;
}

}  // namespace

extern "C" int bc_ellipse_cover(const double* ell, int n, int H, int W, unsigned char* mask, bc_stream stream) {
    BC_CHECK_ARG(ell && mask, "bc_ellipse_cover: bad args (null pointer)");
    BC_CHECK_ARG((reinterpret_cast<uintptr_t>(ell) & 7) == 0, "bc_ellipse_cover: ell must be aligned to 8 bytes");
    EditGeom g;
    if (ei_geometry("bc_ellipse_cover", n, H, W, EI_PER, g)) return 1;
    hipLaunchKernelGGL(ei_cover_kernel, dim3(n * g.chunks), dim3(EI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), ell, W, g.HW, g.chunks, mask);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_ellipse_paint(unsigned char* images, int n, int H, int W, const double* ell, const unsigned char* rgb, int k, bc_stream stream) {
    BC_CHECK_ARG(images && ell && rgb, "bc_ellipse_paint: bad args (null pointer)");
    BC_CHECK_ARG(k > 0, "bc_ellipse_paint: k = %d ellipses per image (it must be >= 1)", k);
    BC_CHECK_ARG((reinterpret_cast<uintptr_t>(ell) & 7) == 0, "bc_ellipse_paint: ell must be aligned to 8 bytes");
    EditGeom g;
    if (ei_geometry("bc_ellipse_paint", n, H, W, 1, g)) return 1;
    BC_CHECK_ARG((long long)n * k <= 0x7fffffffll, "bc_ellipse_paint: %d x %d ellipses", n, k);
    hipLaunchKernelGGL(ei_paint_kernel, dim3(n * g.chunks), dim3(EI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), images, W, g.HW, g.chunks,
                       ell, rgb, k);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_mask_row_extents(const unsigned char* masks, int n, int H, int W, int* out, bc_stream stream) {
    BC_CHECK_ARG(masks && out, "bc_mask_row_extents: bad args (null pointer)");
    BC_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "bc_mask_row_extents: out must be aligned to 4 bytes");
    EditGeom g;
    if (ei_geometry("bc_mask_row_extents", n, H, W, 1, g)) return 1;
    // one wave reads 1024 bytes a pass: rows up to that wide take a wave each, wider ones 2 or 4 (chunks of a multiple of 16 columns)
    const int wpr = W <= 1024 ? 1 : W <= 2048 ? 2 : 4;
    const int span = (bc_ceil_div(W, wpr) + 15) & ~15;
    const long long rows = (long long)n * H;
    const long long blocks = (rows + EI_WAVES / wpr - 1) / (EI_WAVES / wpr);
    BC_CHECK_ARG(blocks <= 0x7fffffffll, "bc_mask_row_extents: %d masks of %d rows exceed the grid", n, H);
    hipLaunchKernelGGL(ei_extents_kernel, dim3((unsigned)blocks), dim3(EI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), masks, rows, W, wpr,
                       span, out);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_mask_cutout(const unsigned char* image, const unsigned char* masks, const int* boxes, int n, int H, int W, unsigned char* out,
                              bc_stream stream) {
    BC_CHECK_ARG(image && masks && boxes && out, "bc_mask_cutout: bad args (null pointer)");
    BC_CHECK_ARG((reinterpret_cast<uintptr_t>(boxes) & 3) == 0, "bc_mask_cutout: boxes must be aligned to 4 bytes");
    EditGeom g;
    if (ei_geometry("bc_mask_cutout", n, H, W, 1, g)) return 1;
    hipLaunchKernelGGL(ei_cutout_kernel, dim3(n * g.chunks), dim3(EI_THREADS), 0, reinterpret_cast<hipStream_t>(stream), image, masks, boxes, H, W,
                       g.HW, g.chunks, out);
    BC_CHECK_LAUNCH();
    return 0;
}
