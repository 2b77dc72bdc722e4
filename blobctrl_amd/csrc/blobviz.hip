// Blob visualisation, feature grid and score pyramid of blobctrl/utils/utils.py (splat_features beyond the pipeline's branch,
// splat_features_from_scores, pyramid_resize) and the app's uint8 image (scripts/blobctrl_app.py:647-648).  All kernels are
// elementwise fp64 / fp32 and memory-bound: one thread per output element, grid-stride, no local arrays.
#include "bc_common.h"
#include "bc_splat.h"

namespace {

inline int viz_blocks(long long total) { return (int)std::min<long long>((total + 255) / 256, 1 << 16); }

// ut:120-135 / 145-181 for one blob per image, channels-last as the reference holds them:
//   raw[n][y][x] = (1, s) (ut:175-176), composed[n][y][x] = ((1 - s), s) (ut:179-181).
__global__ void splat_maps_kernel(const SplatParams prm, int h, int w, double* __restrict__ raw, double* __restrict__ composed) {
    const int n = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= h * w) return;
    const int gy = idx / w, gx = idx - gy * w;
    const double s = bc_splat_score(prm.v + n * 8, gx, gy, h, w);
    const size_t o = ((size_t)n * h * w + idx) * 2;
    *reinterpret_cast<double2*>(raw + o) = make_double2(1.0, s);
    *reinterpret_cast<double2*>(composed + o) = make_double2(1.0 - s, s);
}

// ut:179-181 / 205-209: d_i = s_i * prod_{j>i}(1 - s_j), d_{K-1} = s_{K-1}.  The running product is built from the last
// channel down, in the order of the reference's reversed cumprod.
__global__ void alpha_composite_kernel(const double* __restrict__ raw, long long npix, int K, double* __restrict__ out) {
    for (long long pix = (long long)blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += (long long)gridDim.x * blockDim.x) {
        const double* s = raw + pix * K;
        double* d = out + pix * K;
        const double last = s[K - 1];
        d[K - 1] = last;
        double p = 1.0 - last;
        for (int i = K - 2; i >= 0; --i) {
            const double si = s[i];
            d[i] = p * si;
            p *= 1.0 - si;
        }
    }
}

// F.interpolate(mode="bilinear", align_corners=False), no antialias, along one axis: src = (dst + 0.5) * in / out - 0.5 clamped
// at 0, upper neighbour clamped to in - 1.  Positions and weights in fp64 for every element type.
struct Tap { int i0, i1; double w0, w1; };
__device__ __forceinline__ Tap bilinear_tap(int dst, int in, int out) {
    Tap t;
    if (in == out) { t.i0 = t.i1 = dst; t.w0 = 1.0; t.w1 = 0.0; return t; }
    double src = ((double)dst + 0.5) * ((double)in / (double)out) - 0.5;
    src = src < 0.0 ? 0.0 : src;
    t.i0 = min((int)src, in - 1);
    t.i1 = min(t.i0 + 1, in - 1);
    t.w1 = fmin(fmax(src - (double)t.i0, 0.0), 1.0);
    t.w0 = 1.0 - t.w1;
    return t;
}

template <typename T>
__device__ __forceinline__ double bilinear_read(const T* __restrict__ p, long long sy, long long sx, const Tap& ty, const Tap& tx) {
    const double r0 = tx.w0 * (double)p[ty.i0 * sy + tx.i0 * sx] + tx.w1 * (double)p[ty.i0 * sy + tx.i1 * sx];
    const double r1 = tx.w0 * (double)p[ty.i1 * sy + tx.i0 * sx] + tx.w1 * (double)p[ty.i1 * sy + tx.i1 * sx];
    return ty.w0 * r0 + ty.w1 * r1;
}

// ut:57-77 / pipeline_blobnet.py:706-721: out[n][c][y][x] = sum_m S[n][m][y][x] * F[n][m][c], S read through its strides
// (channels-first or channels-last) and resampled to Hout x Wout inside the read when the sizes differ.
template <typename T>
__global__ void splat_from_scores_kernel(const T* __restrict__ S, const T* __restrict__ F, int N, int M, int C, int Hin, int Win,
                                         long long sn, long long sm, long long sy, long long sx, int Hout, int Wout,
                                         T* __restrict__ out) {
    const long long total = (long long)N * C * Hout * Wout;
    const bool resample = Hin != Hout || Win != Wout;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wout);
        const int y = (int)((idx / Wout) % Hout);
        const int c = (int)((idx / ((long long)Wout * Hout)) % C);
        const int n = (int)(idx / ((long long)Wout * Hout * C));
        const T* s = S + n * sn;
        const T* f = F + (size_t)n * M * C + c;
        double acc = 0.0;
        if (resample) {
            const Tap ty = bilinear_tap(y, Hin, Hout), tx = bilinear_tap(x, Win, Wout);
            for (int m = 0; m < M; ++m) acc += (double)(T)bilinear_read(s + m * sm, sy, sx, ty, tx) * (double)f[(size_t)m * C];
        } else {
            for (int m = 0; m < M; ++m) acc += (double)s[m * sm + y * sy + x * sx] * (double)f[(size_t)m * C];
        }
        out[idx] = (T)acc;
    }
}

// ut:280-294 (one level of pyramid_resize): in [planes][Hin][Win] -> out [planes][Hout][Wout].
template <typename T>
__global__ void resize_bilinear_kernel(const T* __restrict__ in, long long planes, int Hin, int Win, int Hout, int Wout,
                                       T* __restrict__ out) {
    const long long total = planes * Hout * Wout;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(idx % Wout);
        const int y = (int)((idx / Wout) % Hout);
        const long long pl = idx / ((long long)Wout * Hout);
        const Tap ty = bilinear_tap(y, Hin, Hout), tx = bilinear_tap(x, Win, Wout);
        out[idx] = (T)bilinear_read(in + pl * Hin * Win, (long long)Win, 1LL, ty, tx);
    }
}

// app:647-648: img [3][H][W] fp64 -> out [H][W][3] uint8, truncating like astype(np.uint8) on values in [0, 1].
__global__ void pack_rgb8_kernel(const double* __restrict__ img, int H, int W, unsigned char* __restrict__ out) {
    const long long total = (long long)H * W * 3;
    const long long plane = (long long)H * W;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const long long pix = idx / 3;
        const int c = (int)(idx - pix * 3);
        const double v = img[c * plane + pix] * 255.0;
        out[idx] = (unsigned char)fmin(fmax(v, 0.0), 255.0);
    }
}

}  // namespace

extern "C" int bc_splat_maps(const double* params_host, int n, int h, int w, double* raw, double* composed, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(params_host && raw && composed && n > 0 && n <= 16 && h > 0 && w > 0 && (long long)h * w < (1LL << 31),
                 "bc_splat_maps: bad args (n<=16)");
    SplatParams prm;   // travels as a kernel argument: no allocation, no host->device copy, graph-capturable
    for (int i = 0; i < 8 * n; ++i) prm.v[i] = params_host[i];
    hipLaunchKernelGGL(splat_maps_kernel, dim3(bc_ceil_div((long long)h * w, 256), n), dim3(256), 0, stream, prm, h, w, raw, composed);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_alpha_composite(const double* raw, long long npix, int K, double* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(raw && out && raw != out && npix > 0 && K > 0, "bc_alpha_composite: bad args");
    hipLaunchKernelGGL(alpha_composite_kernel, dim3(viz_blocks(npix)), dim3(256), 0, stream, raw, npix, K, out);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_splat_from_scores(const void* S, const void* F, int N, int M, int C, int Hin, int Win, long long s_n,
                                    long long s_m, long long s_y, long long s_x, int Hout, int Wout, int is_f32, void* out,
                                    bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(S && F && out && N > 0 && M > 0 && C > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0,
                 "bc_splat_from_scores: bad args");
    BC_CHECK_ARG(s_n >= 0 && s_m >= 0 && s_y >= 0 && s_x >= 0, "bc_splat_from_scores: negative strides are not supported");
    const long long total = (long long)N * C * Hout * Wout;
    if (is_f32)
        hipLaunchKernelGGL(splat_from_scores_kernel<float>, dim3(viz_blocks(total)), dim3(256), 0, stream, (const float*)S,
                           (const float*)F, N, M, C, Hin, Win, s_n, s_m, s_y, s_x, Hout, Wout, (float*)out);
    else
        hipLaunchKernelGGL(splat_from_scores_kernel<double>, dim3(viz_blocks(total)), dim3(256), 0, stream, (const double*)S,
                           (const double*)F, N, M, C, Hin, Win, s_n, s_m, s_y, s_x, Hout, Wout, (double*)out);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_resize_bilinear(const void* in, long long planes, int Hin, int Win, int Hout, int Wout, int is_f32, void* out,
                                  bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(in && out && planes > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "bc_resize_bilinear: bad args");
    const long long total = planes * Hout * Wout;
    if (is_f32)
        hipLaunchKernelGGL(resize_bilinear_kernel<float>, dim3(viz_blocks(total)), dim3(256), 0, stream, (const float*)in, planes, Hin,
                           Win, Hout, Wout, (float*)out);
    else
        hipLaunchKernelGGL(resize_bilinear_kernel<double>, dim3(viz_blocks(total)), dim3(256), 0, stream, (const double*)in, planes,
                           Hin, Win, Hout, Wout, (double*)out);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_pack_rgb8(const double* img, int H, int W, unsigned char* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(img && out && H > 0 && W > 0, "bc_pack_rgb8: bad args");
    hipLaunchKernelGGL(pack_rgb8_kernel, dim3(viz_blocks((long long)H * W * 3)), dim3(256), 0, stream, img, H, W, out);
    BC_CHECK_LAUNCH();
    return 0;
}
