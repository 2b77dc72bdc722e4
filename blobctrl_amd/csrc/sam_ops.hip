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

// sam_tokens_kernel with a leading prompt index: the same expressions in the same order, so prompt 0 is bit-identical to what that kernel writes
__global__ __launch_bounds__(256) void sam_tokens_batch_kernel(const float* __restrict__ tokens, int ntok, const float* __restrict__ points,
                                                               const int* __restrict__ labels, int npts, const float* __restrict__ gauss, int F,
                                                               const float* __restrict__ label_embed, const float* __restrict__ not_a_point,
                                                               float size, long long total, h16* __restrict__ out) {
    const int Cc = 2 * F, rows = ntok + npts + 1;
    const long long gidx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gidx >= total) return;
    const long long b = gidx / ((long long)rows * Cc);
    const int idx = (int)(gidx - b * rows * Cc);
    points += b * npts * 2;
    labels += b * npts;
    const int r = idx / Cc, c = idx % Cc;
    float v;
    if (r < ntok) {
        v = tokens[r * Cc + c];
    } else if (r == rows - 1) {
        v = not_a_point[c];
    } else {
        const int p = r - ntok, f = c < F ? c : c - F;
        const double cx = 2.0 * (((double)points[2 * p] + 0.5) / (double)size) - 1.0, cy = 2.0 * (((double)points[2 * p + 1] + 0.5) / (double)size) - 1.0;
        const double ang = 6.283185307179586 * (cx * (double)gauss[f] + cy * (double)gauss[F + f]);
        const int lab = labels[p];
        v = (float)(c < F ? sin(ang) : cos(ang)) + ((lab == 0 || lab == 1) ? label_embed[lab * Cc + c] : 0.f);
        if (lab == -1) v = not_a_point[c];
    }
    out[gidx] = (h16)v;
}

// ---- bc_mask_stats: per mask, three counts and the bounding box of v > t.  All integers, so any split of a mask over workgroups and any
// order of combining gives the same result: a workgroup reduces MS_CHUNK elements (registers -> wave shuffles -> LDS across its waves)
// and stores seven partials; one wave per mask combines the partials in a second launch.  No atomics, nothing to zero.
constexpr int MS_THREADS = 256, MS_CHUNK = 16384;          // elements of one mask per workgroup (a multiple of 4 * MS_THREADS)
constexpr int MS_EMPTY_LO = 0x7fffffff, MS_EMPTY_HI = -1;

struct MaskAcc {
    int hi, lo, area, x0, y0, x1, y1;
};

__device__ __forceinline__ void ms_take(float v, int x, int y, float t_hi, float t_lo, float t, MaskAcc& a) {
    a.hi += v > t_hi ? 1 : 0;
    a.lo += v > t_lo ? 1 : 0;
    if (v > t) {
        a.area += 1;
        a.x0 = min(a.x0, x); a.x1 = max(a.x1, x);
        a.y0 = min(a.y0, y); a.y1 = max(a.y1, y);
    }
}

__device__ __forceinline__ void ms_wave_reduce(MaskAcc& a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.hi += __shfl_xor(a.hi, d, 64);
        a.lo += __shfl_xor(a.lo, d, 64);
        a.area += __shfl_xor(a.area, d, 64);
        a.x0 = min(a.x0, __shfl_xor(a.x0, d, 64)); a.y0 = min(a.y0, __shfl_xor(a.y0, d, 64));
        a.x1 = max(a.x1, __shfl_xor(a.x1, d, 64)); a.y1 = max(a.y1, __shfl_xor(a.y1, d, 64));
    }
}

template <bool VEC>
__global__ __launch_bounds__(MS_THREADS) void mask_stats_partial_kernel(const float* __restrict__ logits, int HW, int W, float t_hi, float t_lo,
                                                                        float t, int chunks, int* __restrict__ partial) {
    const long long m = blockIdx.x / chunks;                            // grid = n * chunks workgroups, a mask's chunks side by side
    const int chunk = blockIdx.x % chunks;
    const float* src = logits + m * HW;
    const int lo = chunk * MS_CHUNK, hi = min(HW, lo + MS_CHUNK);      // (HW <= INT_MAX - MS_CHUNK: checked by the caller)
    MaskAcc a = {0, 0, 0, MS_EMPTY_LO, MS_EMPTY_LO, MS_EMPTY_HI, MS_EMPTY_HI};
    if constexpr (VEC) {                                                // HW % 4 == 0 and a 16-byte aligned base: every mask starts aligned
        for (int e = lo + 4 * (int)threadIdx.x; e < hi; e += 4 * MS_THREADS) {
            const float4 v = *reinterpret_cast<const float4*>(src + e);
            int y = e / W, x = e - y * W;
            const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ms_take(vv[j], x, y, t_hi, t_lo, t, a);
                if (++x == W) { x = 0; ++y; }
            }
        }
    } else {
        for (int e = lo + (int)threadIdx.x; e < hi; e += MS_THREADS) {
            const int y = e / W;
            ms_take(src[e], e - y * W, y, t_hi, t_lo, t, a);
        }
    }
    ms_wave_reduce(a);
    __shared__ int part[MS_THREADS / 64][7];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = a.hi; part[wave][1] = a.lo; part[wave][2] = a.area;
        part[wave][3] = a.x0; part[wave][4] = a.y0; part[wave][5] = a.x1; part[wave][6] = a.y1;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const int k = threadIdx.x;
        int r = part[0][k];
#pragma unroll
        for (int w = 1; w < MS_THREADS / 64; ++w) r = k < 3 ? r + part[w][k] : k < 5 ? min(r, part[w][k]) : max(r, part[w][k]);
        partial[(m * chunks + chunk) * 7 + k] = r;
    }
}

__global__ __launch_bounds__(64) void mask_stats_combine_kernel(const int* __restrict__ partial, int chunks, int* __restrict__ out) {
    const long long m = blockIdx.x;
    MaskAcc a = {0, 0, 0, MS_EMPTY_LO, MS_EMPTY_LO, MS_EMPTY_HI, MS_EMPTY_HI};
    for (int c = threadIdx.x; c < chunks; c += 64) {
        const int* p = partial + (m * chunks + c) * 7;
        a.hi += p[0]; a.lo += p[1]; a.area += p[2];
        a.x0 = min(a.x0, p[3]); a.y0 = min(a.y0, p[4]); a.x1 = max(a.x1, p[5]); a.y1 = max(a.y1, p[6]);
    }
    ms_wave_reduce(a);
    if (threadIdx.x == 0) {
        int* o = out + m * 7;
        const bool any = a.area > 0;                                     // an empty mask has the box 0, 0, 0, 0
        o[0] = a.hi; o[1] = a.lo; o[2] = a.area;
        o[3] = any ? a.x0 : 0; o[4] = any ? a.y0 : 0; o[5] = any ? a.x1 : 0; o[6] = any ? a.y1 : 0;
    }
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

extern "C" int bc_sam_tokens_batch(const float* tokens, int ntok, const float* points, const int* labels, int B, int npts, const float* gauss,
                                   int F, const float* label_embed, const float* not_a_point, float size, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(tokens && points && labels && gauss && label_embed && not_a_point && out && B > 0 && ntok > 0 && npts > 0 && F > 0 && size > 0.f,
                 "bc_sam_tokens_batch: bad args");
    BC_CHECK_ARG((long long)(ntok + npts + 1) * 2 * F <= 0x7fffffffll, "bc_sam_tokens_batch: the rows of one prompt must fit 2^31 elements");
    const long long total = (long long)B * (ntok + npts + 1) * 2 * F;
    SAM_LAUNCH(sam_tokens_batch_kernel, total, tokens, ntok, points, labels, npts, gauss, F, label_embed, not_a_point, size, total,
               reinterpret_cast<h16*>(out));
}

extern "C" int bc_mask_stats_chunks(int H, int W) {
    if (H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffll - MS_CHUNK) return -1;
    return (int)(((long long)H * W + MS_CHUNK - 1) / MS_CHUNK);
}

extern "C" int bc_mask_stats(const float* logits, int n, int H, int W, float threshold, float offset, int* partial, int* out, bc_stream stream) {
    BC_CHECK_ARG(logits && partial && out && n > 0 && H > 0 && W > 0, "bc_mask_stats: bad args");
    const int chunks = bc_mask_stats_chunks(H, W);
    BC_CHECK_ARG(chunks > 0, "bc_mask_stats: a mask of %d x %d does not fit 2^31 elements", H, W);
    BC_CHECK_ARG((long long)n * chunks <= 0x7fffffffll, "bc_mask_stats: %d masks of %d chunks exceed the grid", n, chunks);
    BC_CHECK_ARG(offset >= 0.f && threshold == threshold && offset == offset, "bc_mask_stats: the offset must be >= 0 and no NaN");
    // the two outer thresholds are the fp32 roundings of the sums: what comparing an fp32 tensor with the scalar t +- o does
    const float t_hi = (float)((double)threshold + (double)offset), t_lo = (float)((double)threshold - (double)offset);
    const int HW = H * W;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool vec = HW % 4 == 0 && reinterpret_cast<uintptr_t>(logits) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(mask_stats_partial_kernel<true>, dim3(n * chunks), dim3(MS_THREADS), 0, s, logits, HW, W, t_hi, t_lo, threshold, chunks, partial);
    else
        hipLaunchKernelGGL(mask_stats_partial_kernel<false>, dim3(n * chunks), dim3(MS_THREADS), 0, s, logits, HW, W, t_hi, t_lo, threshold, chunks, partial);
    BC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mask_stats_combine_kernel, dim3(n), dim3(64), 0, s, partial, chunks, out);
    BC_CHECK_LAUNCH();
    return 0;
}
