// Zoomed edits on the device (include/blobctrl_overlay.h): a mask's bounds, Pillow's Gaussian blur of a mask, the paste-back.  gfx950.
//
//   ov_blur_rows   three BoxBlur.c line passes along a row, in LDS.  A workgroup takes a stretch of OV_STRETCH pixels of one row and
//                  stages it with a halo of 3 (R + 1) pixels a side - index g of the line holds pixel clamp(g, 0, W - 1), which is how
//                  the passes repeat the edge.  Pass p is computed for the stretch and what is left of the halo, (3 - p)(R + 1) a side;
//                  a position outside the line takes the value of the clamped position (the NEXT pass repeats the edge of this pass's
//                  output, not of the source).  A thread takes OV_RUN consecutive positions: one window sum, then it slides.  Integer
//                  sums are exact in any order, so this is Pillow's running accumulator.  The third pass stores to memory.
//   ov_blur_cols   the same for a tile of 64 columns x 64 rows: lanes along x, so every load and store of a wave is one row segment
//                  of 64 consecutive bytes, and a column's passes walk LDS with a stride of 64 bytes (4 lanes share a bank word).
//   ov_bounds      the second launch of bc_mask_bounds: min / max over the row extents of a mask, one workgroup per mask.
//   ov_composite   apply_overlay's pixel arithmetic, four pixels a thread (three 32-bit stores where the address allows it).
#include "bc_common.h"
#include "../../include/blobctrl_overlay.h"

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_WAVES = OV_THREADS / 64;
constexpr int OV_HALO = 3 * (BC_BLUR_MAX_R + 1);                  // the largest halo a side
constexpr int OV_STRETCH = 1024;                                  // pixels of a row a workgroup produces
constexpr int OV_RUN = 4;                                         // consecutive positions a thread produces in a row pass
constexpr int OV_TILE = 64;                                       // columns and rows of a column tile
constexpr int OV_COL_RUN = 8;
constexpr int OV_COL_ROWS = OV_TILE + 2 * OV_HALO;                // rows of a staged column tile (448)
constexpr int OV_PER = 4;                                         // pixels per thread in ov_composite
static_assert(2 * OV_COL_ROWS * OV_TILE <= 64 * 1024, "the column tile must fit the static LDS limit (BC_BLUR_MAX_R)");

// One pass for positions g0 .. g0 + cnt - 1 of a line of `len` pixels.  in[(g - base) * ES] holds the previous pass's value at clamp(g);
// the result goes to out[(g - obase) * OS].  The caller guarantees clamp(g) +- (R + 1) is inside `in` (see the ranges in the kernels).
template <int ES>
__device__ __forceinline__ void ov_run(const unsigned char* in, int base, unsigned char* out, int obase, int OS, int g0, int cnt, int len,
                                       int R, unsigned ww, unsigned fw) {
    unsigned acc = 0;
    int prev = 0;
    for (int k = 0; k < cnt; ++k) {
        const int g = g0 + k;
        const int gc = min(max(g, 0), len - 1);
        const unsigned char* c = in + (gc - base) * ES;
        if (k == 0) {
            for (int j = -R; j <= R; ++j) acc += c[j * ES];
        } else if (gc != prev) {                                          // gc == prev + 1: slide the window by one
            acc += c[R * ES];
            acc -= c[(-R - 1) * ES];
        }
        prev = gc;
        const unsigned far = (unsigned)c[(-R - 1) * ES] + (unsigned)c[(R + 1) * ES];
        out[(g - obase) * OS] = (unsigned char)((acc * ww + far * fw + (1u << 23)) >> 24);
    }
}

__global__ __launch_bounds__(OV_THREADS) void ov_blur_rows_kernel(const unsigned char* __restrict__ src, int W, int stretches, int R, unsigned ww,
                                                                  unsigned fw, unsigned char* __restrict__ dst) {
    __shared__ unsigned char bufA[OV_STRETCH + 2 * OV_HALO], bufB[OV_STRETCH + 2 * OV_HALO];
    const long long line = blockIdx.x / stretches;
    const int x0 = (int)(blockIdx.x - line * stretches) * OV_STRETCH;
    const int S = min(OV_STRETCH, W - x0), step = R + 1, base = x0 - 3 * step;
    const unsigned char* row = src + line * W;
    for (int i = threadIdx.x; i < S + 6 * step; i += OV_THREADS) bufA[i] = row[min(max(base + i, 0), W - 1)];
    __syncthreads();
    for (int p = 1; p <= 3; ++p) {
        const int lo = x0 - (3 - p) * step, count = S + 2 * (3 - p) * step;
        const unsigned char* in = (p & 1) ? bufA : bufB;
        unsigned char* out = p == 3 ? dst + line * W : ((p & 1) ? bufB : bufA);
        const int obase = p == 3 ? 0 : base;
        for (int r = threadIdx.x; r * OV_RUN < count; r += OV_THREADS)
            ov_run<1>(in, base, out, obase, 1, lo + r * OV_RUN, min(OV_RUN, count - r * OV_RUN), W, R, ww, fw);
        __syncthreads();
    }
}

__global__ __launch_bounds__(OV_THREADS) void ov_blur_cols_kernel(const unsigned char* __restrict__ src, int H, int W, int tx, int ty, int R,
                                                                  unsigned ww, unsigned fw, unsigned char* __restrict__ dst) {
    __shared__ unsigned char bufA[OV_COL_ROWS * OV_TILE], bufB[OV_COL_ROWS * OV_TILE];
    const int per = tx * ty;
    const long long img = blockIdx.x / per;
    const int t = (int)(blockIdx.x - img * per), by = t / tx, bx = t - by * tx;
    const int col = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = bx * OV_TILE + col, y0 = by * OV_TILE;
    const int S = min(OV_TILE, H - y0), step = R + 1, base = y0 - 3 * step;
    const bool live = x < W;
    const unsigned char* plane = src + img * H * W;
    for (int i = wave; i < S + 6 * step; i += OV_WAVES)
        bufA[i * OV_TILE + col] = live ? plane[(long long)min(max(base + i, 0), H - 1) * W + x] : (unsigned char)0;
    __syncthreads();
    for (int p = 1; p <= 3; ++p) {
        const int lo = y0 - (3 - p) * step, count = S + 2 * (3 - p) * step;
        const unsigned char* in = ((p & 1) ? bufA : bufB) + col;
        unsigned char* out = p == 3 ? dst + img * H * W + x : ((p & 1) ? bufB : bufA) + col;
        const int obase = p == 3 ? 0 : base, OS = p == 3 ? W : OV_TILE;
        if (live)
            for (int r = wave; r * OV_COL_RUN < count; r += OV_WAVES)
                ov_run<OV_TILE>(in, base, out, obase, OS, lo + r * OV_COL_RUN, min(OV_COL_RUN, count - r * OV_COL_RUN), H, R, ww, fw);
        __syncthreads();
    }
}

__global__ __launch_bounds__(OV_THREADS) void ov_bounds_kernel(const int* __restrict__ ext, int H, int* __restrict__ out) {
    __shared__ int part[OV_WAVES][4];
    const int* e = ext + (long long)blockIdx.x * H * 2;
    int x0 = 0x7fffffff, x1 = -1, r0 = 0x7fffffff, r1 = -1;
    for (int y = threadIdx.x; y < H; y += OV_THREADS) {
        const int last = e[2 * y + 1];
        if (last >= 0) { x0 = min(x0, e[2 * y]); x1 = max(x1, last); r0 = min(r0, y); r1 = max(r1, y); }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        x0 = min(x0, __shfl_xor(x0, d, 64)); x1 = max(x1, __shfl_xor(x1, d, 64));
        r0 = min(r0, __shfl_xor(r0, d, 64)); r1 = max(r1, __shfl_xor(r1, d, 64));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = x0; part[wave][1] = x1; part[wave][2] = r0; part[wave][3] = r1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < OV_WAVES; ++j) {
            x0 = min(x0, part[j][0]); x1 = max(x1, part[j][1]); r0 = min(r0, part[j][2]); r1 = max(r1, part[j][3]);
        }
        int* o = out + (long long)blockIdx.x * 4;
        const bool none = x1 < 0;
        o[0] = none ? -1 : x0; o[1] = x1; o[2] = none ? -1 : r0; o[3] = r1;
    }
}

__device__ __forceinline__ unsigned ov_div255(unsigned v) { return (((v + 128) >> 8) + v + 128) >> 8; }

// one channel of apply_overlay: init byte c under inverted-mask alpha a (premultiplied p), composited onto the opaque byte d
__device__ __forceinline__ unsigned ov_pixel(unsigned c, unsigned mi, unsigned a, unsigned d) {
    if (a == 0) return d;
    const unsigned p = ov_div255(mi * c);
    const unsigned u = min(255u, 255u * p / a);
    const unsigned outa255 = a * 255 + 255 * (255 - a);
    const unsigned coef1 = a * 255 * 255 * 128 / outa255;                 // a <= 255: a * 255 * 255 * 128 < 2^31
    const unsigned coef2 = 255 * 128 - coef1;
    const unsigned t = u * coef1 + d * coef2 + (0x80u << 7);
    return (((t >> 8) + t) >> 8) >> 7;
}

__global__ __launch_bounds__(OV_THREADS) void ov_composite_kernel(const unsigned char* __restrict__ init, const unsigned char* __restrict__ mask,
                                                                  const unsigned char* __restrict__ patches, int W, int HW, int chunks, int h,
                                                                  int w, int px, int py, unsigned char* __restrict__ out) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p0 = (c * OV_THREADS + (int)threadIdx.x) * OV_PER;          // < HW + 1024 <= 2^28 + 1024
    if (p0 >= HW) return;
    const unsigned char* patch = patches + (long long)i * h * w * 3;
    unsigned char* dst = out + ((long long)i * HW + p0) * 3;
    const int cnt = min(OV_PER, HW - p0);
    int Y = p0 / W, X = p0 - Y * W;
    unsigned char v[OV_PER * 3] = {};
    for (int j = 0; j < cnt; ++j) {
        const unsigned mi = 255u - mask[p0 + j], a = ov_div255(mi * 255u);
        const unsigned char* ci = init + (long long)(p0 + j) * 3;
        const int sx = X - px, sy = Y - py;
        const bool inside = sx >= 0 && sx < w && sy >= 0 && sy < h;
        const unsigned char* d = patch + ((long long)sy * w + sx) * 3;       // dereferenced only when inside
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) v[j * 3 + ch] = (unsigned char)ov_pixel(ci[ch], mi, a, inside ? d[ch] : 0u);
        if (++X == W) { X = 0; ++Y; }
    }
    if (cnt == OV_PER && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        unsigned* d32 = reinterpret_cast<unsigned*>(dst);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            d32[k] = (unsigned)v[4 * k] | ((unsigned)v[4 * k + 1] << 8) | ((unsigned)v[4 * k + 2] << 16) | ((unsigned)v[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < cnt * 3; ++k) dst[k] = v[k];
    }
}

bool ov_apart(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return pa + (uintptr_t)na <= pb || pb + (uintptr_t)nb <= pa;
}

// the frame and the weights of a blur launch; 1 with bc_last_error() set when they are bad
int ov_blur_args(const char* who, const unsigned char* src, const unsigned char* dst, int n, int H, int W, int R, int ww, int fw) {
    BC_CHECK_ARG(src && dst, "%s: bad args (null pointer)", who);
    BC_CHECK_ARG(n > 0 && H > 0 && W > 0, "%s: bad args (n, H, W <= 0)", who);
    BC_CHECK_ARG(H <= BC_EDIT_MAX_DIM && W <= BC_EDIT_MAX_DIM, "%s: a frame of %d x %d exceeds the limit of %d a side", who, H, W, BC_EDIT_MAX_DIM);
    BC_CHECK_ARG(R >= 0 && R <= BC_BLUR_MAX_R, "%s: box radius R = %d is outside 0 .. %d", who, R, BC_BLUR_MAX_R);
    BC_CHECK_ARG(ww >= 0 && fw >= 0 && (long long)(2 * R + 1) * ww + 2ll * fw <= (1ll << 24),
                 "%s: weights ww = %d, fw = %d with R = %d exceed 2^24 in sum (or are negative)", who, ww, fw, R);
    const long long bytes = (long long)n * H * W;
    BC_CHECK_ARG(ov_apart(dst, bytes, src, bytes), "%s: dst overlaps src", who);
    return 0;
}

}  // namespace

extern "C" int bc_box_blur3_rows(const unsigned char* src, int n, int H, int W, int R, int ww, int fw, unsigned char* dst, bc_stream stream) {
    if (ov_blur_args("bc_box_blur3_rows", src, dst, n, H, W, R, ww, fw)) return 1;
    const int stretches = bc_ceil_div(W, OV_STRETCH);
    const long long blocks = (long long)n * H * stretches;
    BC_CHECK_ARG(blocks <= 0x7fffffffll, "bc_box_blur3_rows: %d frames of %d x %d exceed the grid", n, H, W);
    hipLaunchKernelGGL(ov_blur_rows_kernel, dim3((unsigned)blocks), dim3(OV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, W, stretches, R,
                       (unsigned)ww, (unsigned)fw, dst);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_box_blur3_cols(const unsigned char* src, int n, int H, int W, int R, int ww, int fw, unsigned char* dst, bc_stream stream) {
    if (ov_blur_args("bc_box_blur3_cols", src, dst, n, H, W, R, ww, fw)) return 1;
    const int tx = bc_ceil_div(W, OV_TILE), ty = bc_ceil_div(H, OV_TILE);
    const long long blocks = (long long)n * tx * ty;
    BC_CHECK_ARG(blocks <= 0x7fffffffll, "bc_box_blur3_cols: %d frames of %d x %d exceed the grid", n, H, W);
    hipLaunchKernelGGL(ov_blur_cols_kernel, dim3((unsigned)blocks), dim3(OV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, H, W, tx, ty, R,
                       (unsigned)ww, (unsigned)fw, dst);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_mask_bounds(const unsigned char* masks, int n, int H, int W, int* extents, int* out, bc_stream stream) {
    BC_CHECK_ARG(masks && extents && out, "bc_mask_bounds: bad args (null pointer)");
    BC_CHECK_ARG((reinterpret_cast<uintptr_t>(extents) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                 "bc_mask_bounds: extents and out must be aligned to 4 bytes");
    BC_CHECK_ARG(n > 0 && H > 0 && W > 0, "bc_mask_bounds: bad args (n, H, W <= 0)");
    BC_CHECK_ARG(H <= BC_EDIT_MAX_DIM && W <= BC_EDIT_MAX_DIM, "bc_mask_bounds: a frame of %d x %d exceeds the limit of %d a side", H, W,
                 BC_EDIT_MAX_DIM);
    if (const int rc = bc_mask_row_extents(masks, n, H, W, extents, stream)) return rc;
    hipLaunchKernelGGL(ov_bounds_kernel, dim3(n), dim3(OV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), extents, H, out);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_overlay_composite(const unsigned char* init, const unsigned char* mask, const unsigned char* patches, int n, int H, int W, int h,
                                    int w, int x, int y, unsigned char* out, bc_stream stream) {
    BC_CHECK_ARG(init && mask && patches && out, "bc_overlay_composite: bad args (null pointer)");
    BC_CHECK_ARG(n > 0 && H > 0 && W > 0, "bc_overlay_composite: bad args (n, H, W <= 0)");
    BC_CHECK_ARG(H <= BC_EDIT_MAX_DIM && W <= BC_EDIT_MAX_DIM, "bc_overlay_composite: a frame of %d x %d exceeds the limit of %d a side", H, W,
                 BC_EDIT_MAX_DIM);
    BC_CHECK_ARG(h > 0 && w > 0 && x >= 0 && y >= 0 && (long long)x + w <= W && (long long)y + h <= H,
                 "bc_overlay_composite: a patch of %d x %d at (%d, %d) leaves the frame of %d x %d", h, w, x, y, H, W);
    const int HW = H * W;
    const int chunks = bc_ceil_div(HW, (long long)OV_THREADS * OV_PER);
    BC_CHECK_ARG((long long)n * chunks <= 0x7fffffffll, "bc_overlay_composite: %d frames of %d x %d exceed the grid", n, H, W);
    const long long bytes = (long long)n * HW * 3;
    BC_CHECK_ARG(ov_apart(out, bytes, init, (long long)HW * 3) && ov_apart(out, bytes, mask, HW) &&
                 ov_apart(out, bytes, patches, (long long)n * h * w * 3), "bc_overlay_composite: out overlaps an input");
    hipLaunchKernelGGL(ov_composite_kernel, dim3(n * chunks), dim3(OV_THREADS), 0, reinterpret_cast<hipStream_t>(stream), init, mask, patches, W, HW,
                       chunks, h, w, x, y, out);
    BC_CHECK_LAUNCH();
    return 0;
}
