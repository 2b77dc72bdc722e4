// Blob maths and loop glue kernels (all HBM/latency-trivial): Gaussian-blob splat rasteriser, input assembly,
// timestep embedding, CFG + scheduler step, layout conversion at the nn.Module boundary, DINOv2 embedding glue.
#include "bc_common.h"
#include "bc_splat.h"
#include "bc_cfg_step.h"
#include "../../include/blobctrl_requests.h"

namespace {

// blobctrl/utils/utils.py:145-194 for one blob per image (the score itself: bc_splat.h).
//   out[0] = (1 - s) * 1 (background after alpha compositing), out[1] = s.
__global__ void splat_kernel(const SplatParams prm, int h, int w, double* __restrict__ out) {
    const int n = blockIdx.y;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= h * w) return;
    const int gy = idx / w, gx = idx - gy * w;
    const double s = bc_splat_score(prm.v + n * 8, gx, gy, h, w);
    double* o = out + (size_t)n * 2 * h * w;
    o[idx] = (1.0 - s);                                               // ut:179-181 alpha composite with bg score 1
    o[(size_t)h * w + idx] = s;
}

// The divisor of the noisy latents in a DIV_TABLE assembly (pipe:1032 `scheduler.scale_model_input`, the sigma-space schedulers):
// column 14 of coefficient row *step_idx, sqrt(sigma_t^2 + 1).  A step index outside [0, nsteps) (the capture warm-ups advance the
// counter) has no table row: the divisor is then 1 and x / 1 = x, the unscaled kernel's output bit for bit.
__device__ __forceinline__ float input_divisor(const float* __restrict__ coef, const int* __restrict__ step_idx, int nsteps) {
    const int step = *step_idx;
    return (step >= 0 && step < nsteps) ? coef[(size_t)step * 16 + 14] : 1.f;
}

// The divisor of image `b` in a DIV_IMAGE assembly (a batch of edit requests with their own step counts): column 14 of ITS row of the
// [Blat][nsteps][16] table.  A row whose column 14 is 0 ("do not divide": a table that does not scale its input) and a step index
// outside the table give 1, as above.
__device__ __forceinline__ float input_divisor_of(const float* __restrict__ coef, int step, int nsteps, int b) {
    if (step < 0 || step >= nsteps) return 1.f;
    const float d = coef[((size_t)b * nsteps + step) * 16 + 14];
    return d != 0.f ? d : 1.f;
}

// How an assembly divides the noisy latents: not at all, by the row of the one table every image shares (input_divisor), or image b
// by the row of its own table (input_divisor_of: a batch of edit requests).
enum DivMode { DIV_NONE, DIV_TABLE, DIV_IMAGE };

// pipeline_blobnet.py:724-739 + :706-721.  X[b][y][x][c], x in [0, 2w): left = clean image latents, right = noisy latents.
//   DIV: unless DIV_NONE the noisy latents (right half, channels 0-3) are divided in fp32 before the fp16 conversion, as the reference
//        divides `latent_model_input`; the clean latents, the score and the feature channels are what they are without it.  `coef`
//        ([nsteps][16], DIV_IMAGE: [Blat][nsteps][16]) / `step_idx` / `nsteps` are not read by the DIV_NONE instantiation.
template <DivMode DIV>
__global__ void assemble_kernel(const float* __restrict__ latents, int Blat, const float* __restrict__ img_lat,
                                const float* __restrict__ score, const float* __restrict__ feat, int Bimg, int F, int Bout,
                                int h, int w, int Cpad, int dup_score, const float* __restrict__ coef,
                                const int* __restrict__ step_idx, int nsteps, h16* __restrict__ X) {
    const long long total = (long long)Bout * h * 2 * w * (Cpad / 8);
    const float shared = DIV == DIV_TABLE ? input_divisor(coef, step_idx, nsteps) : 1.f;
    const int step = DIV == DIV_IMAGE ? *step_idx : 0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int nch = Cpad / 8;
        int ch = (int)(idx % nch);
        long long pix = idx / nch;
        int x = (int)(pix % (2 * w));
        int y = (int)((pix / (2 * w)) % h);
        int b = (int)(pix / ((long long)2 * w * h));
        const bool right = x >= w;
        const int xs = right ? x - w : x;
        const int bi = b % Bimg;
        const float sc = score[((size_t)bi * h + y) * w + xs];
        const float div = DIV == DIV_IMAGE ? input_divisor_of(coef, step, nsteps, b % Blat) : shared;
        uint4 raw;
        h16* o = reinterpret_cast<h16*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int c = ch * 8 + j;
            float v = 0.f;
            if (c < 4) {
                v = right ? latents[(((size_t)(b % Blat) * 4 + c) * h + y) * w + xs] : img_lat[(((size_t)bi * 4 + c) * h + y) * w + xs];
                if (DIV != DIV_NONE && right) v = v / div;
            } else if (c == 4) {
                v = sc;
            } else if (c < 5 + F) {
                v = sc * feat[(size_t)bi * F + c - 5];
            } else if (dup_score && c == 5) {
                v = sc;          // rank-1 collapsed feature channels: one extra copy of the score (see engine.py)
            }
            o[j] = (h16)v;
        }
        bc_st16(X + (size_t)pix * Cpad + ch * 8, raw);
    }
}

// The same input (8 channels: 4 latents, score, [score], 0, 0) written as the 3x3 im2col operand of conv_in: row = canvas pixel,
// k = tap * 8 + channel for the nine taps (zero outside the h x 2w canvas = the convolution's padding), zero-filled up to 128, so that
// conv_in (K = 72: outside the LDS-DMA GEMM's K % 64 == 0 fast path, 41 us per launch on the register-staged kernel) runs as a dense
// K = 128 GEMM.  One thread per (pixel, 16-byte chunk).  DIV as in assemble_kernel: the noisy latents of every tap are divided.
template <DivMode DIV>
__global__ void assemble_im2col_kernel(const float* __restrict__ latents, int Blat, const float* __restrict__ img_lat,
                                       const float* __restrict__ score, int Bimg, int Bout, int h, int w, int dup_score,
                                       const float* __restrict__ coef, const int* __restrict__ step_idx, int nsteps,
                                       h16* __restrict__ X) {
    const long long total = (long long)Bout * h * 2 * w * 16;
    const float shared = DIV == DIV_TABLE ? input_divisor(coef, step_idx, nsteps) : 1.f;
    const int step = DIV == DIV_IMAGE ? *step_idx : 0;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
        const int chunk = (int)(idx & 15);
        const long long pix = idx >> 4;
        const int x = (int)(pix % (2 * w));
        const int y = (int)((pix / (2 * w)) % h);
        const int b = (int)(pix / ((long long)2 * w * h));
        const float div = DIV == DIV_IMAGE ? input_divisor_of(coef, step, nsteps, b % Blat) : shared;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (chunk < 9) {
            const int yy = y + chunk / 3 - 1, xx = x + chunk % 3 - 1;
            if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)(2 * w)) {
                const bool right = xx >= w;
                const int xs = right ? xx - w : xx;
                const int bi = b % Bimg;
                const float sc = score[((size_t)bi * h + yy) * w + xs];
                h16* o = reinterpret_cast<h16*>(&raw);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float v = right ? latents[(((size_t)(b % Blat) * 4 + c) * h + yy) * w + xs]
                                    : img_lat[(((size_t)bi * 4 + c) * h + yy) * w + xs];
                    if (DIV != DIV_NONE && right) v = v / div;
                    o[c] = (h16)v;
                }
                o[4] = (h16)sc;
                o[5] = dup_score ? (h16)sc : (h16)0.f;
            }
        }
        bc_st16(X + (size_t)pix * 128 + chunk * 8, raw);
    }
}

// embeddings.py:27-78: [cos(t*f_k) | sin(t*f_k)], f_k = exp(-ln(10000) * k / half)
// rows_per_step > 0: row r belongs to step r / rows_per_step of the table (all steps of an edit at once)
//   COND: `cond` fp32 [cond_rows][dim] = cond_proj(timestep_cond) of a UNet with time_cond_proj_dim (embeddings.py:559, 578: added to the
//         sinusoid before linear_1); row r takes cond row r % cond_rows.  The sinusoid and the sum are formed in fp64 and rounded to
//         fp16 ONCE: the output is the fp16 nearest to the exact sum (an fp32 sinusoid at t ~ 1000 is off by up to 1e-4, a quarter of
//         an fp16 step; the launch is a few thousand elements once per edit).  `cond` / `cond_rows` are not read by the instantiation
//         without COND, which is the fp32 kernel it always was.
template <bool COND>
__device__ __forceinline__ void temb_body(const float* __restrict__ t_table, const int* __restrict__ t_idx, float t_value, int rows,
                                          int dim, int rows_per_step, const float* __restrict__ cond, int cond_rows,
                                          h16* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * dim) return;
    const int r = i / dim, c = i - r * dim;
    const int halfd = dim / 2;
    const float t = rows_per_step > 0 ? t_table[r / rows_per_step] : (t_table ? t_table[t_idx ? *t_idx : 0] : t_value);
    const int k = c < halfd ? c : c - halfd;
    if (COND) {
        const double a = (double)t * exp(-9.210340371976184 * (double)k / (double)halfd);
        out[i] = (h16)((c < halfd ? cos(a) : sin(a)) + (double)cond[(size_t)(r % cond_rows) * dim + c]);
        return;
    }
    const float freq = expf(-9.210340371976184f * (float)k / (float)halfd);
    const float a = t * freq;
    out[i] = (h16)(c < halfd ? cosf(a) : sinf(a));
}

__global__ void temb_kernel(const float* __restrict__ t_table, const int* __restrict__ t_idx, float t_value, int rows,
                            int dim, int rows_per_step, h16* __restrict__ out) {
    temb_body<false>(t_table, t_idx, t_value, rows, dim, rows_per_step, nullptr, 1, out);
}

__global__ void temb_cond_kernel(const float* __restrict__ t_table, const int* __restrict__ t_idx, float t_value, int rows,
                                 int dim, int rows_per_step, const float* __restrict__ cond, int cond_rows, h16* __restrict__ out) {
    temb_body<true>(t_table, t_idx, t_value, rows, dim, rows_per_step, cond, cond_rows, out);
}

__global__ void silu_kernel(const h16* __restrict__ x, h16* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = (h16)bc_silu_f((float)x[i]);
}

// Crop (right half) + classifier-free guidance + scheduler step: ONE body (cfg_step_body, bc_cfg_step.h) behind the bc_cfg_scheduler_step*
// entry points and their single-pass and request forms, specialised at compile time.
template <bool NOISE, bool THIRD, bool GUARD>
__global__ void cfg_step_kernel(const float* __restrict__ eps, float* __restrict__ latents, const float* __restrict__ coef,
                                const int* __restrict__ step_idx, float* __restrict__ hist, float guidance, int B, int h, int w,
                                const float* __restrict__ noise, int nsteps, float* __restrict__ eps_out) {
    cfg_step_body<false, NOISE, THIRD, GUARD>(eps, latents, coef, step_idx, hist, guidance, B, h, w, noise, nsteps, eps_out);
}

// The step of a single-pass plan: always guarded (its ABI has nsteps).
template <bool NOISE, bool THIRD>
__global__ void step_single_kernel(const float* __restrict__ eps, float* __restrict__ latents, const float* __restrict__ coef,
                                   const int* __restrict__ step_idx, float* __restrict__ hist, int B, int h, int w,
                                   const float* __restrict__ noise, int nsteps, float* __restrict__ eps_out) {
    cfg_step_body<true, NOISE, THIRD, true>(eps, latents, coef, step_idx, hist, 0.f, B, h, w, noise, nsteps, eps_out);
}

// The step of a requests plan: always guarded, guidance always from the row.
template <bool SINGLE, bool NOISE, bool THIRD>
__global__ void step_requests_kernel(const float* __restrict__ eps, float* __restrict__ latents, const float* __restrict__ coef,
                                     const int* __restrict__ step_idx, float* __restrict__ hist, int B, int h, int w,
                                     const float* __restrict__ noise, int nsteps, float* __restrict__ eps_out) {
    cfg_step_body<SINGLE, NOISE, THIRD, true, true>(eps, latents, coef, step_idx, hist, -1.f, B, h, w, noise, nsteps, eps_out);
}

__global__ void nchw_to_nhwc_kernel(const void* __restrict__ src, int src_f32, int B, int C, int HW, int Cpad,
                                    h16* __restrict__ dst) {
    const long long total = (long long)B * HW * Cpad;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c = (int)(i % Cpad);
        long long pix = i / Cpad;
        int p = (int)(pix % HW);
        int b = (int)(pix / HW);
        float v = 0.f;
        if (c < C) {
            size_t s = ((size_t)b * C + c) * HW + p;
            v = src_f32 ? reinterpret_cast<const float*>(src)[s] : (float)reinterpret_cast<const h16*>(src)[s];
        }
        dst[i] = (h16)v;
    }
}

__global__ void nhwc_to_nchw_kernel(const h16* __restrict__ src, int B, int C, int HW, int ldsrc, void* __restrict__ dst,
                                    int dst_f32) {
    const long long total = (long long)B * C * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int p = (int)(i % HW);
        int c = (int)((i / HW) % C);
        int b = (int)(i / ((long long)HW * C));
        float v = (float)src[((size_t)b * HW + p) * ldsrc + c];
        if (dst_f32) reinterpret_cast<float*>(dst)[i] = v;
        else reinterpret_cast<h16*>(dst)[i] = (h16)v;
    }
}

// out[b][0] = cls + pos[0]; out[b][1 + t] = patches[b][t] + pos[1 + t]
__global__ void add_cls_pos_kernel(const h16* __restrict__ patches, const float* __restrict__ cls,
                                   const float* __restrict__ pos, int B, int T, int D, h16* __restrict__ out) {
    const long long total = (long long)B * (T + 1) * D;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int d = (int)(i % D);
        int t = (int)((i / D) % (T + 1));
        int b = (int)(i / ((long long)D * (T + 1)));
        float v = (t == 0) ? cls[d] : (float)patches[((size_t)b * T + (t - 1)) * D + d];
        out[i] = (h16)(v + pos[(size_t)t * D + d]);
    }
}

// im2col for kernel = stride = patch: row (b, gy, gx), column (c, ky, kx) matching Conv2d weight.flatten(1)
__global__ void patchify_kernel(const float* __restrict__ px, int B, int H, int W, int patch, int Kpad, h16* __restrict__ out) {
    const int gh = H / patch, gw = W / patch;
    const long long total = (long long)B * gh * gw * Kpad;
    const int K = 3 * patch * patch;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int k = (int)(i % Kpad);
        long long row = i / Kpad;
        int gx = (int)(row % gw);
        int gy = (int)((row / gw) % gh);
        int b = (int)(row / ((long long)gw * gh));
        float v = 0.f;
        if (k < K) {
            int c = k / (patch * patch);
            int r = k - c * patch * patch;
            int ky = r / patch, kx = r - ky * patch;
            v = px[(((size_t)b * 3 + c) * H + gy * patch + ky) * W + gx * patch + kx];
        }
        out[i] = (h16)v;
    }
}

// vae.py:767-789: mean + exp(0.5 * clamp(logvar, -30, 20)) * noise, times the latent scaling factor
__global__ void gaussian_sample_kernel(const h16* __restrict__ mom, const float* __restrict__ noise, int B, int Cz, int HW,
                                       float scale, float* __restrict__ out) {
    const long long total = (long long)B * Cz * HW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int p = (int)(i % HW);
        int c = (int)((i / HW) % Cz);
        int b = (int)(i / ((long long)HW * Cz));
        const h16* m = mom + ((size_t)b * HW + p) * (2 * Cz);
        float mean = (float)m[c];
        float logvar = fminf(fmaxf((float)m[Cz + c], -30.f), 20.f);
        out[i] = (mean + expf(0.5f * logvar) * noise[i]) * scale;
    }
}

// CLIPTextEmbeddings (transformers models/clip/modeling_clip.py): token_embedding(ids) + position_embedding(arange(T))
__global__ void embed_tokens_kernel(const long long* __restrict__ ids, const h16* __restrict__ tok, const float* __restrict__ pos,
                                    int B, int T, int D, int vocab, h16* __restrict__ out) {
    const long long total = (long long)B * T * (D / 8);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ch = (int)(i % (D / 8));
        const long long row = i / (D / 8);
        const int t = (int)(row % T);
        long long id = ids[row];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        const uint4 raw = bc_ld16(tok + (size_t)id * D + ch * 8);
        const h16* e = reinterpret_cast<const h16*>(&raw);
        uint4 o;
        h16* oh = reinterpret_cast<h16*>(&o);
#pragma unroll
        for (int j = 0; j < 8; ++j) oh[j] = (h16)((float)e[j] + pos[(size_t)t * D + ch * 8 + j]);
        bc_st16(out + (size_t)row * D + ch * 8, o);
    }
}

inline int ew_blocks(long long total) { return (int)std::min<long long>((total + 255) / 256, 256 * 8); }

}  // namespace

extern "C" int bc_splat_scores(const double* params_host, int n, int h, int w, double* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(params_host && out && n > 0 && n <= 16 && h > 0 && w > 0, "bc_splat_scores: bad args (n<=16)");
    SplatParams prm;   // travels as a kernel argument: no allocation, no host->device copy, graph-capturable
    for (int i = 0; i < 8 * n; ++i) prm.v[i] = params_host[i];
    hipLaunchKernelGGL(splat_kernel, dim3(bc_ceil_div(h * w, 256), n), dim3(256), 0, stream, prm, h, w, out);
    BC_CHECK_LAUNCH();
    return 0;
}

// The launchers behind the six assembly entry points (`name` = the entry point's own name for the error text); an undivided entry
// point passes coef = step_idx = nullptr / nsteps = 0, which its instantiation never reads.
template <DivMode DIV>
static int assemble_launch(const char* name, const float* latents, int Blat, const float* img_lat, const float* score, const float* feat,
                           int Bimg, int F, int Bout, int h, int w, int Cpad, int dup_score, const float* coef, const int* step_idx,
                           int nsteps, bc_half* X, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (!feat) F = 0;
    BC_CHECK_ARG(latents && img_lat && score && X && Blat > 0 && Bout > 0 && Bimg > 0 &&
                 (DIV == DIV_NONE || (coef && step_idx && nsteps > 0 && h > 0 && w > 0)), "%s: bad args", name);
    BC_CHECK_ARG(Cpad % 8 == 0 && Cpad >= 5 + F, "%s: Cpad=%d must be a multiple of 8 and >= %d", name, Cpad, 5 + F);
    long long total = (long long)Bout * h * 2 * w * (Cpad / 8);
    hipLaunchKernelGGL(assemble_kernel<DIV>, dim3(ew_blocks(total)), dim3(256), 0, stream, latents, Blat, img_lat, score, feat,
                       Bimg, F, Bout, h, w, Cpad, dup_score, coef, step_idx, nsteps, reinterpret_cast<h16*>(X));
    BC_CHECK_LAUNCH();
    return 0;
}

template <DivMode DIV>
static int assemble_im2col_launch(const char* name, const float* latents, int Blat, const float* img_lat, const float* score, int Bimg,
                                  int Bout, int h, int w, int dup_score, const float* coef, const int* step_idx, int nsteps, bc_half* X,
                                  bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(latents && img_lat && score && X && Blat > 0 && Bout > 0 && Bimg > 0 &&
                 (DIV == DIV_NONE || (coef && step_idx && nsteps > 0 && h > 0 && w > 0)), "%s: bad args", name);
    long long total = (long long)Bout * h * 2 * w * 16;
    hipLaunchKernelGGL(assemble_im2col_kernel<DIV>, dim3(ew_blocks(total)), dim3(256), 0, stream, latents, Blat, img_lat, score, Bimg,
                       Bout, h, w, dup_score, coef, step_idx, nsteps, reinterpret_cast<h16*>(X));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_assemble_input(const float* latents, int Blat, const float* img_lat, const float* score,
                                 const float* feat, int Bimg, int F, int Bout, int h, int w, int Cpad, int dup_score,
                                 bc_half* X, bc_stream stream) {
    return assemble_launch<DIV_NONE>("bc_assemble_input", latents, Blat, img_lat, score, feat, Bimg, F, Bout, h, w, Cpad, dup_score,
                                     nullptr, nullptr, 0, X, stream);
}

extern "C" int bc_assemble_input_scaled(const float* latents, int Blat, const float* img_lat, const float* score,
                                        const float* feat, int Bimg, int F, int Bout, int h, int w, int Cpad, int dup_score,
                                        const float* coef, const int* step_idx, int nsteps, bc_half* X, bc_stream stream) {
    return assemble_launch<DIV_TABLE>("bc_assemble_input_scaled", latents, Blat, img_lat, score, feat, Bimg, F, Bout, h, w, Cpad,
                                      dup_score, coef, step_idx, nsteps, X, stream);
}

extern "C" int bc_assemble_input_requests(const float* latents, int Blat, const float* img_lat, const float* score, const float* feat,
                                          int Bimg, int F, int Bout, int h, int w, int Cpad, int dup_score, const float* coef,
                                          const int* step_idx, int nsteps, bc_half* X, bc_stream stream) {
    return assemble_launch<DIV_IMAGE>("bc_assemble_input_requests", latents, Blat, img_lat, score, feat, Bimg, F, Bout, h, w, Cpad,
                                      dup_score, coef, step_idx, nsteps, X, stream);
}

extern "C" int bc_assemble_input_im2col(const float* latents, int Blat, const float* img_lat, const float* score, int Bimg, int Bout,
                                        int h, int w, int dup_score, bc_half* X, bc_stream stream) {
    return assemble_im2col_launch<DIV_NONE>("bc_assemble_input_im2col", latents, Blat, img_lat, score, Bimg, Bout, h, w, dup_score,
                                            nullptr, nullptr, 0, X, stream);
}

extern "C" int bc_assemble_input_im2col_scaled(const float* latents, int Blat, const float* img_lat, const float* score, int Bimg,
                                               int Bout, int h, int w, int dup_score, const float* coef, const int* step_idx, int nsteps,
                                               bc_half* X, bc_stream stream) {
    return assemble_im2col_launch<DIV_TABLE>("bc_assemble_input_im2col_scaled", latents, Blat, img_lat, score, Bimg, Bout, h, w,
                                             dup_score, coef, step_idx, nsteps, X, stream);
}

extern "C" int bc_assemble_input_im2col_requests(const float* latents, int Blat, const float* img_lat, const float* score, int Bimg,
                                                 int Bout, int h, int w, int dup_score, const float* coef, const int* step_idx,
                                                 int nsteps, bc_half* X, bc_stream stream) {
    return assemble_im2col_launch<DIV_IMAGE>("bc_assemble_input_im2col_requests", latents, Blat, img_lat, score, Bimg, Bout, h, w,
                                             dup_score, coef, step_idx, nsteps, X, stream);
}

extern "C" int bc_timestep_embedding(const float* t_table, const int* t_idx, float t_value, int rows, int dim,
                                     bc_half* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(out && rows > 0 && dim > 0 && dim % 2 == 0, "bc_timestep_embedding: bad args");
    hipLaunchKernelGGL(temb_kernel, dim3(bc_ceil_div(rows * dim, 256)), dim3(256), 0, stream, t_table, t_idx, t_value, rows,
                       dim, 0, reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_timestep_embedding_table(const float* t_table, int nsteps, int rows_per_step, int dim, bc_half* out,
                                           bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(t_table && out && nsteps > 0 && rows_per_step > 0 && dim > 0 && dim % 2 == 0, "bc_timestep_embedding_table: bad args");
    const int rows = nsteps * rows_per_step;
    hipLaunchKernelGGL(temb_kernel, dim3(bc_ceil_div(rows * dim, 256)), dim3(256), 0, stream, t_table, nullptr, 0.f, rows, dim,
                       rows_per_step, reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

// The `_cond` forms of the two entry points above: cond fp32 [cond_rows][dim] is added to the sinusoid in fp32 (temb_cond_kernel).
extern "C" int bc_timestep_embedding_cond(const float* t_table, const int* t_idx, float t_value, int rows, int dim, const float* cond,
                                          bc_half* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(out && cond && rows > 0 && dim > 0 && dim % 2 == 0, "bc_timestep_embedding_cond: bad args");
    hipLaunchKernelGGL(temb_cond_kernel, dim3(bc_ceil_div(rows * dim, 256)), dim3(256), 0, stream, t_table, t_idx, t_value, rows,
                       dim, 0, cond, rows, reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_timestep_embedding_table_cond(const float* t_table, int nsteps, int rows_per_step, int dim, const float* cond,
                                                bc_half* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(t_table && cond && out && nsteps > 0 && rows_per_step > 0 && dim > 0 && dim % 2 == 0,
                 "bc_timestep_embedding_table_cond: bad args");
    const int rows = nsteps * rows_per_step;
    hipLaunchKernelGGL(temb_cond_kernel, dim3(bc_ceil_div(rows * dim, 256)), dim3(256), 0, stream, t_table, nullptr, 0.f, rows, dim,
                       rows_per_step, cond, rows_per_step, reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

// One timestep per ROW (a batch of edit requests with their own schedules): the table kernels with one row per "step", so the
// arithmetic - and with it every bit of the output - is theirs for the same t.
extern "C" int bc_timestep_embedding_rows(const float* t_rows, int rows, int dim, const float* cond, int cond_rows, bc_half* out,
                                          bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(t_rows && out && rows > 0 && dim > 0 && dim % 2 == 0 && (!cond || cond_rows > 0) && (long long)rows * dim < (1ll << 31),
                 "bc_timestep_embedding_rows: bad args");
    if (cond)
        hipLaunchKernelGGL(temb_cond_kernel, dim3(bc_ceil_div(rows * dim, 256)), dim3(256), 0, stream, t_rows, nullptr, 0.f, rows, dim, 1,
                           cond, cond_rows, reinterpret_cast<h16*>(out));
    else
        hipLaunchKernelGGL(temb_kernel, dim3(bc_ceil_div(rows * dim, 256)), dim3(256), 0, stream, t_rows, nullptr, 0.f, rows, dim, 1,
                           reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_silu(const bc_half* x, bc_half* y, long long n, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(x && y && n > 0, "bc_silu: bad args");
    hipLaunchKernelGGL(silu_kernel, dim3(ew_blocks(n)), dim3(256), 0, stream, reinterpret_cast<const h16*>(x),
                       reinterpret_cast<h16*>(y), n);
    BC_CHECK_LAUNCH();
    return 0;
}

// The three CFG entry points are one instance each; one without NOISE / GUARD passes noise = nullptr / nsteps = 0, which its
// instantiation never reads.
template <bool NOISE, bool THIRD, bool GUARD>
static int cfg_step_launch(const char* name, const float* eps, float* latents, const float* coef, int* step_idx, float* hist,
                           float guidance_scale, int B, int h, int w, const float* noise, int nsteps, float* eps_out, int advance,
                           bc_stream stream) {
    return step_launch(name, eps && latents && coef && step_idx && hist && B > 0 && (!NOISE || noise) &&
                       (!GUARD || (h > 0 && w > 0 && nsteps > 0)), cfg_step_kernel<NOISE, THIRD, GUARD>, B, h, w, step_idx, advance, stream,
                       eps, latents, coef, step_idx, hist, guidance_scale, B, h, w, noise, nsteps, eps_out);
}

extern "C" int bc_cfg_scheduler_step(const float* eps, float* latents, const float* coef, int* step_idx, float* hist,
                                     float guidance_scale, int B, int h, int w, float* eps_out, int advance,
                                     bc_stream stream) {
    return cfg_step_launch<false, false, false>("bc_cfg_scheduler_step", eps, latents, coef, step_idx, hist, guidance_scale, B, h, w,
                                                nullptr, 0, eps_out, advance, stream);
}

extern "C" int bc_cfg_scheduler_step_noise(const float* eps, float* latents, const float* coef, int* step_idx, float* hist,
                                           float guidance_scale, int B, int h, int w, const float* noise, int nsteps, float* eps_out,
                                           int advance, bc_stream stream) {
    return cfg_step_launch<true, false, true>("bc_cfg_scheduler_step_noise", eps, latents, coef, step_idx, hist, guidance_scale, B, h,
                                              w, noise, nsteps, eps_out, advance, stream);
}

extern "C" int bc_cfg_scheduler_step3(const float* eps, float* latents, const float* coef, int* step_idx, float* hist,
                                      float guidance_scale, int B, int h, int w, int nsteps, float* eps_out, int advance,
                                      bc_stream stream) {
    return cfg_step_launch<false, true, true>("bc_cfg_scheduler_step3", eps, latents, coef, step_idx, hist, guidance_scale, B, h, w,
                                              nullptr, nsteps, eps_out, advance, stream);
}

// The entry points that take their step form at run time pick the instance from these tables, index noise * 2 + third (requests:
// single * 4 + noise * 2 + third).
using GuardedStep = void (*)(const float*, float*, const float*, const int*, float*, int, int, int, const float*, int, float*);
static const GuardedStep single_steps[4] = {step_single_kernel<false, false>, step_single_kernel<false, true>,
                                            step_single_kernel<true, false>, step_single_kernel<true, true>};
static const GuardedStep request_steps[8] = {
    step_requests_kernel<false, false, false>, step_requests_kernel<false, false, true>, step_requests_kernel<false, true, false>,
    step_requests_kernel<false, true, true>,   step_requests_kernel<true, false, false>, step_requests_kernel<true, false, true>,
    step_requests_kernel<true, true, false>,   step_requests_kernel<true, true, true>};

// The step of a guidance-free (single-pass) plan: eps [B][h][2w][4], e = its right half.  noise != NULL adds cf[12] * noise[step],
// third != 0 adds cf[13] * x0_{i-2}; a step index outside [0, nsteps) leaves every buffer as it is.
extern "C" int bc_scheduler_step_single(const float* eps, float* latents, const float* coef, int* step_idx, float* hist, int B, int h,
                                        int w, const float* noise, int nsteps, int third, float* eps_out, int advance,
                                        bc_stream stream) {
    return step_launch("bc_scheduler_step_single", eps && latents && coef && step_idx && hist && B > 0 && h > 0 && w > 0 && nsteps > 0,
                       single_steps[step_form(false, noise, third)], B, h, w, step_idx, advance, stream,
                       eps, latents, coef, step_idx, hist, B, h, w, noise, nsteps, eps_out);
}

// The step of a batch of edit requests: coef [B][nsteps][16], image b applies its own row (guidance from column 11) and is left alone
// when the row's column 15 is set.  single != 0: eps holds B images (a single-pass plan), else the 2B of the CFG pairs.
extern "C" int bc_scheduler_step_requests(const float* eps, float* latents, const float* coef, int* step_idx, float* hist, int B, int h,
                                          int w, const float* noise, int nsteps, int third, int single, float* eps_out, int advance,
                                          bc_stream stream) {
    return step_launch("bc_scheduler_step_requests", eps && latents && coef && step_idx && hist && B > 0 && h > 0 && w > 0 && nsteps > 0 &&
                       (long long)B * 4 * h * w < (1ll << 31), request_steps[step_form(single, noise, third)], B, h, w, step_idx, advance,
                       stream, eps, latents, coef, step_idx, hist, B, h, w, noise, nsteps, eps_out);
}

extern "C" int bc_nchw_to_nhwc_f16(const void* src, int src_is_f32, int B, int C, int HW, int Cpad, bc_half* dst,
                                   bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(src && dst && Cpad >= C, "bc_nchw_to_nhwc_f16: bad args");
    long long total = (long long)B * HW * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_blocks(total)), dim3(256), 0, stream, src, src_is_f32, B, C, HW, Cpad,
                       reinterpret_cast<h16*>(dst));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_nhwc_to_nchw(const bc_half* src, int B, int C, int HW, int ldsrc, void* dst, int dst_is_f32,
                               bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(src && dst && ldsrc >= C, "bc_nhwc_to_nchw: bad args");
    long long total = (long long)B * C * HW;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ew_blocks(total)), dim3(256), 0, stream, reinterpret_cast<const h16*>(src), B,
                       C, HW, ldsrc, dst, dst_is_f32);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_add_cls_pos(const bc_half* patches, const float* cls, const float* pos, int B, int T, int D,
                              bc_half* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(patches && cls && pos && out, "bc_add_cls_pos: bad args");
    long long total = (long long)B * (T + 1) * D;
    hipLaunchKernelGGL(add_cls_pos_kernel, dim3(ew_blocks(total)), dim3(256), 0, stream, reinterpret_cast<const h16*>(patches),
                       cls, pos, B, T, D, reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_patchify(const float* pixels, int B, int H, int W, int patch, int Kpad, bc_half* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(pixels && out && H % patch == 0 && W % patch == 0 && Kpad >= 3 * patch * patch && Kpad % 8 == 0,
                 "bc_patchify: bad args");
    long long total = (long long)B * (H / patch) * (W / patch) * Kpad;
    hipLaunchKernelGGL(patchify_kernel, dim3(ew_blocks(total)), dim3(256), 0, stream, pixels, B, H, W, patch, Kpad,
                       reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_gaussian_sample(const bc_half* moments, const float* noise, int B, int Cz, int HW, float scale, float* out,
                                  bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(moments && noise && out && B > 0 && Cz > 0 && HW > 0, "bc_gaussian_sample: bad args");
    long long total = (long long)B * Cz * HW;
    hipLaunchKernelGGL(gaussian_sample_kernel, dim3(ew_blocks(total)), dim3(256), 0, stream,
                       reinterpret_cast<const h16*>(moments), noise, B, Cz, HW, scale, out);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_embed_tokens(const long long* ids, const bc_half* tok_emb, const float* pos_emb, int B, int T, int D, int vocab,
                               bc_half* out, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(ids && tok_emb && pos_emb && out && B > 0 && T > 0 && D > 0 && D % 8 == 0 && vocab > 0, "bc_embed_tokens: bad args");
    long long total = (long long)B * T * (D / 8);
    hipLaunchKernelGGL(embed_tokens_kernel, dim3(ew_blocks(total)), dim3(256), 0, stream, ids, reinterpret_cast<const h16*>(tok_emb),
                       pos_emb, B, T, D, vocab, reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}
