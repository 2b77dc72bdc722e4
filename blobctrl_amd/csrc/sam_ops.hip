// The small launches of the Segment-Anything path (include/blobctrl_sam.h): window partition / unpartition with the zero padding the
// reference attends to, position adds, the point-prompt Fourier embedding, the mask pixel shuffle and the bilinear resizes of
// SamPredictor.predict (transformers modeling_sam.py SamVisionLayer / SamPromptEncoder / SamMaskDecoder; the reference app's
// segmentation(), scripts/blobctrl_app.py:1019-1043).  All of them are bandwidth-trivial: one thread per 16-byte chunk or per output element.
#include "bc_common.h"
#include "../../include/blobctrl_sam.h"

namespace {

__device__ __forceinline__ uint4 add_h8(uint4 a, uint4 b) {
    const h16* x = reinterpret_cast<const h16*>(&a);
    const h16* y = reinterpret_cast<const h16*>(&b);
    uint4 r;
    h16* o = reinterpret_cast<h16*>(&r);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (h16)((float)x[e] + (float)y[e]);
    return r;
}

__global__ __launch_bounds__(256) void window_partition_kernel(const h16* __restrict__ x, int H, int W, int C8, int ws, int nWh, int nWw,
                                                               long long total, h16* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % C8);
    long long row = idx / C8;
    const int j = (int)(row % ws); row /= ws;
    const int i = (int)(row % ws); row /= ws;
    const int wx = (int)(row % nWw); row /= nWw;
    const int wy = (int)(row % nWh);
    const long long b = row / nWh;
    const int h = wy * ws + i, w = wx * ws + j;
    uint4 v = make_uint4(0, 0, 0, 0);                       // a padded row is a real row of zeros
    if (h < H && w < W) v = bc_ld16(x + (((b * H + h) * W + w) * C8 + ch) * 8);
    bc_st16(out + idx * 8, v);
}

__global__ __launch_bounds__(256) void window_unpartition_kernel(const h16* __restrict__ win, const h16* __restrict__ res, int H, int W, int C8,
                                                                 int ws, int nWh, int nWw, long long total, h16* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % C8);
    long long row = idx / C8;
    const int w = (int)(row % W); row /= W;
    const int h = (int)(row % H);
    const long long b = row / H;
    const long long wrow = (((b * nWh + h / ws) * nWw + w / ws) * ws + h % ws) * ws + w % ws;
    bc_st16(out + idx * 8, add_h8(bc_ld16(win + (wrow * C8 + ch) * 8), bc_ld16(res + idx * 8)));
}

__global__ __launch_bounds__(256) void add_pos_kernel(const h16* __restrict__ x, const float* __restrict__ pos, long long TD, long long total,
                                                      h16* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    out[idx] = (h16)((float)x[idx] + pos[idx % TD]);
}

__global__ __launch_bounds__(256) void add_rows_kernel(const h16* __restrict__ a, const h16* __restrict__ b, int C8, long long b_chunks,
                                                       long long total, h16* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    bc_st16(out + idx * 8, add_h8(bc_ld16(a + idx * 8), bc_ld16(b + (idx % b_chunks) * 8)));
}

__global__ __launch_bounds__(256) void act_rows_kernel(h16* __restrict__ x, long long total, int act) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    uint4 v = bc_ld16(x + idx * 8);
    h16* e = reinterpret_cast<h16*>(&v);
#pragma unroll
    for (int k = 0; k < 8; ++k) e[k] = act ? (h16)fmaxf((float)e[k], 0.f) : (h16)bc_gelu_f((float)e[k]);
    bc_st16(x + idx * 8, v);
}

// ATen's upsample_bilinear2d arithmetic (align_corners = false): scale = in / out in fp32, src = scale (dst + 0.5) - 0.5 clamped at 0
__device__ __forceinline__ void bilinear_tap(int dst, float scale, int in, int& i0, int& step, float& l1) {
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    step = i0 < in - 1 ? 1 : 0;
    l1 = s - (float)i0;
}

__global__ __launch_bounds__(256) void bilinear_resize_kernel(const float* __restrict__ src, int H, int W, int ch, int cw, int Ho, int Wo,
                                                              long long total, int thr_on, float thr, void* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int x = (int)(idx % Wo), y = (int)((idx / Wo) % Ho);
    const long long nc = idx / ((long long)Wo * Ho);
    int y0, ys, x0, xs;
    float ly, lx;
    bilinear_tap(y, (float)ch / (float)Ho, ch, y0, ys, ly);
    bilinear_tap(x, (float)cw / (float)Wo, cw, x0, xs, lx);
    const float* p = src + (nc * H + y0) * W + x0;
    const float v = (1.f - ly) * ((1.f - lx) * p[0] + lx * p[xs]) + ly * ((1.f - lx) * p[(long long)ys * W] + lx * p[(long long)ys * W + xs]);
    if (thr_on) reinterpret_cast<unsigned char*>(out)[idx] = v > thr ? 1 : 0;
    else reinterpret_cast<float*>(out)[idx] = v;
}

__global__ __launch_bounds__(256) void sam_tokens_kernel(const float* __restrict__ tokens, int ntok, const float* __restrict__ points,
                                                         const int* __restrict__ labels, int npts, const float* __restrict__ gauss, int F,
                                                         const float* __restrict__ label_embed, const float* __restrict__ not_a_point, float size,
                                                         h16* __restrict__ out) {
    const int Cc = 2 * F, rows = ntok + npts + 1;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * Cc) return;
    const int r = idx / Cc, c = idx % Cc;
    float v;
    if (r < ntok) {
        v = tokens[r * Cc + c];
    } else if (r == rows - 1) {
        v = not_a_point[c];
    } else {
        const int p = r - ntok, f = c < F ? c : c - F;
        // fp64: the Gaussian matrix has entries of the order of 100, so the angle runs to thousands of radians
        const double cx = 2.0 * (((double)points[2 * p] + 0.5) / (double)size) - 1.0, cy = 2.0 * (((double)points[2 * p + 1] + 0.5) / (double)size) - 1.0;
        const double ang = 6.283185307179586 * (cx * (double)gauss[f] + cy * (double)gauss[F + f]);
        const int lab = labels[p];
        v = (float)(c < F ? sin(ang) : cos(ang)) + ((lab == 0 || lab == 1) ? label_embed[lab * Cc + c] : 0.f);
        if (lab == -1) v = not_a_point[c];
    }
    out[idx] = (h16)v;
}

__global__ __launch_bounds__(256) void sam_masks_kernel(const h16* __restrict__ up, int C2, const h16* __restrict__ hyper, int ldh, int h, int w,
                                                        int ntok, long long total, float* __restrict__ out) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int X = (int)(idx % (4 * w)), Y = (int)((idx / (4 * w)) % (4 * h));
    const int tok = (int)((idx / ((long long)16 * w * h)) % ntok);
    const long long b = idx / ((long long)16 * w * h * ntok);
    const long long pix = (b * h + Y / 4) * w + X / 4;
    const long long row = ((pix * 2 + ((Y >> 1) & 1)) * 2 + ((X >> 1) & 1)) * 4 + (Y & 1) * 2 + (X & 1);
    const h16* u = up + row * C2;
    const h16* hy = hyper + (b * ntok + tok) * ldh;
    float acc = 0.f;
    for (int c = 0; c < C2; ++c) acc = fmaf((float)hy[c], (float)u[c], acc);
    out[idx] = acc;
}

inline int blocks_for(long long total) { return (int)((total + 255) / 256); }

}  // namespace

#define SAM_LAUNCH(kernel, total, ...)                                                                              \
    do {                                                                                                            \
        BC_CHECK_ARG((total) > 0 && (total) <= (1ll << 38), "%s: bad element count", #kernel);                     \
        hipLaunchKernelGGL(kernel, dim3(blocks_for(total)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), __VA_ARGS__); \
        BC_CHECK_LAUNCH();                                                                                          \
        return 0;                                                                                                   \
    } while (0)

extern "C" int bc_window_partition(const bc_half* x, int B, int H, int W, int C, int ws, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(x && out && B > 0 && H > 0 && W > 0 && ws > 0 && C > 0 && C % 8 == 0, "bc_window_partition: bad args (C must be a multiple of 8)");
    const int nWh = bc_ceil_div(H, ws), nWw = bc_ceil_div(W, ws);
    const long long total = (long long)B * nWh * nWw * ws * ws * (C / 8);
    SAM_LAUNCH(window_partition_kernel, total, reinterpret_cast<const h16*>(x), H, W, C / 8, ws, nWh, nWw, total, reinterpret_cast<h16*>(out));
}

extern "C" int bc_window_unpartition(const bc_half* win, const bc_half* res, int B, int H, int W, int C, int ws, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(win && res && out && B > 0 && H > 0 && W > 0 && ws > 0 && C > 0 && C % 8 == 0, "bc_window_unpartition: bad args (C must be a multiple of 8)");
    const int nWh = bc_ceil_div(H, ws), nWw = bc_ceil_div(W, ws);
    const long long total = (long long)B * H * W * (C / 8);
    SAM_LAUNCH(window_unpartition_kernel, total, reinterpret_cast<const h16*>(win), reinterpret_cast<const h16*>(res), H, W, C / 8, ws, nWh, nWw,
               total, reinterpret_cast<h16*>(out));
}

extern "C" int bc_add_pos(const bc_half* x, const float* pos, int B, int T, int D, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(x && pos && out && B > 0 && T > 0 && D > 0, "bc_add_pos: bad args");
    const long long total = (long long)B * T * D;
    SAM_LAUNCH(add_pos_kernel, total, reinterpret_cast<const h16*>(x), pos, (long long)T * D, total, reinterpret_cast<h16*>(out));
}

extern "C" int bc_add_rows(const bc_half* a, const bc_half* b, int rows, int b_rows, int C, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(a && b && out && rows > 0 && b_rows > 0 && rows % b_rows == 0 && C > 0 && C % 8 == 0, "bc_add_rows: bad args (C must be a multiple of 8)");
    const long long total = (long long)rows * (C / 8);
    SAM_LAUNCH(add_rows_kernel, total, reinterpret_cast<const h16*>(a), reinterpret_cast<const h16*>(b), C / 8, (long long)b_rows * (C / 8), total,
               reinterpret_cast<h16*>(out));
}

extern "C" int bc_act_rows(bc_half* x, long long n, int act, bc_stream stream) {
    BC_CHECK_ARG(x && n > 0 && n % 8 == 0 && (act == 0 || act == 1), "bc_act_rows: bad args (n must be a multiple of 8, act 0 or 1)");
    const long long total = n / 8;
    SAM_LAUNCH(act_rows_kernel, total, reinterpret_cast<h16*>(x), total, act);
}

extern "C" int bc_bilinear_resize_f32(const float* src, int NC, int H, int W, int crop_h, int crop_w, int Ho, int Wo, int threshold_on,
                                      float threshold, void* out, bc_stream stream) {
    BC_CHECK_ARG(src && out && NC > 0 && H > 0 && W > 0 && Ho > 0 && Wo > 0, "bc_bilinear_resize_f32: bad args");
    BC_CHECK_ARG(crop_h > 0 && crop_h <= H && crop_w > 0 && crop_w <= W, "bc_bilinear_resize_f32: crop %d x %d outside the %d x %d source", crop_h, crop_w, H, W);
    const long long total = (long long)NC * Ho * Wo;
    SAM_LAUNCH(bilinear_resize_kernel, total, src, H, W, crop_h, crop_w, Ho, Wo, total, threshold_on, threshold, out);
}

extern "C" int bc_sam_tokens(const float* tokens, int ntok, const float* points, const int* labels, int npts, const float* gauss, int F,
                             const float* label_embed, const float* not_a_point, float size, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(tokens && points && labels && gauss && label_embed && not_a_point && out && ntok > 0 && npts > 0 && F > 0 && size > 0.f,
                 "bc_sam_tokens: bad args");
    const long long total = (long long)(ntok + npts + 1) * 2 * F;
    SAM_LAUNCH(sam_tokens_kernel, total, tokens, ntok, points, labels, npts, gauss, F, label_embed, not_a_point, size, reinterpret_cast<h16*>(out));
}

extern "C" int bc_sam_masks(const bc_half* up, int C2, const bc_half* hyper, int ldh, int B, int h, int w, int ntok, float* out, bc_stream stream) {
    BC_CHECK_ARG(up && hyper && out && B > 0 && h > 0 && w > 0 && ntok > 0 && C2 > 0 && ldh >= C2, "bc_sam_masks: bad args");
    const long long total = (long long)B * ntok * 16 * h * w;
    SAM_LAUNCH(sam_masks_kernel, total, reinterpret_cast<const h16*>(up), C2, reinterpret_cast<const h16*>(hyper), ldh, h, w, ntok, total, out);
}
