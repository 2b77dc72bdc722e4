// AutoencoderTiny (TAESD) decoder kernels for gfx950 (include/blobctrl_tiny_vae.h): the 3x3 convolution of the decoder's five layer forms on
// v_mfma_f32_32x32x16_f16, and the latent prologue.
//
// tiny_conv3x3_kernel<CI, MT>: a workgroup of four waves owns an 8 x 32 pixel tile with all its output channels.
//   * The weights [Co][3][3][CI] are copied into LDS once per workgroup (72 KB at 64 -> 64) and stay there over a persistent loop over tiles.
//   * The (8 + 2) x (32 + 2) x CI input halo of a tile is staged in LDS once; the nearest-2x upsample of the `up` form and the zero padding
//     (in the upsampled domain) are applied on that load.  The halo of the NEXT tile is fetched into registers before the MFMA loop of the
//     current one and written to LDS behind it, so the global loads fly under the matrix work.
//   * GEMM orientation: A = weights (rows = output channels), B = halo pixels (columns = 32 consecutive pixels of one tile row), so the
//     accumulator has the pixel on the lane and the channels in the registers.  The A rows are dealt to the channels so that a lane ends up
//     with 32 CONSECUTIVE channels of its pixel (MT = 2: accumulator register i of M tile t on half-wave h is channel 32 h + 16 t + i): the
//     epilogue is four 16-byte stores per pixel and lane, and the skip tensor is read the same way.
//   * A wave computes two tile rows (2 x 32 pixels) x 64 channels: per 16-wide K step two A and two B fragments (ds_read_b128) feed four MFMAs.
//   * CI = 8 (the `in` form): one K step per tap, the upper half-wave (k = 8 .. 15) feeds zeros.
//   * MT = 1 (the `out` form, 3 channels in weight rows padded to 8): weight rows 8 .. 31 are zero in LDS; channels 0 .. 2 sit in
//     accumulator registers 0 .. 2 of the lower half-wave, which alone stores - fp32 NCHW or the quantised bytes.
// LDS: CI 64 / MT 2: 74752 (weights, row pitch 584 halfs) + 48960 (halo, pixel pitch 72 halfs) + 256 (bias) = 123968 bytes, one workgroup per CU.
#include "bc_common.h"
#include "../../include/blobctrl_tiny_vae.h"

namespace {

constexpr int TV_TH = 8, TV_TW = 32, TV_THREADS = 256;
constexpr int TV_HH = TV_TH + 2, TV_HW = TV_TW + 2, TV_HPIX = TV_HH * TV_HW;

template <int CI>
struct TvGeom {
    static constexpr int PP = CI + 8;                 // halo pixel pitch in halfs: +16 bytes keeps the 32 pixel reads of a fragment off each other's banks
    static constexpr int WP = 9 * CI + 8;             // weight row pitch in halfs
    static constexpr int CPP = CI / 8;                // 16-byte chunks per pixel
    static constexpr int CHUNKS = TV_HPIX * CPP;
    static constexpr int ITERS = (CHUNKS + TV_THREADS - 1) / TV_THREADS;
    static constexpr int KS = CI >= 16 ? CI / 16 : 1; // K steps per tap
};

template <int CI, int MT>
constexpr int tv_lds_bytes() {
    return (MT * 32 * TvGeom<CI>::WP + TV_HPIX * TvGeom<CI>::PP) * 2 + 64 * 4;
}

struct TvArgs {
    const h16* x;
    const h16* w;
    const float* bias;
    const h16* skip;
    void* out;
    int B, H, W, Hin, Win;
    int co_rows, co;
    int up, relu, out_mode;
    int tiles_x, tiles_y;
    long long ntiles;
};

struct TvTile { int b, y0, x0; };

__device__ __forceinline__ TvTile tv_tile(const TvArgs& a, long long t) {
    const int per_image = a.tiles_x * a.tiles_y;
    TvTile r;
    r.b = (int)(t / per_image);
    const int rem = (int)(t - (long long)r.b * per_image);
    r.y0 = (rem / a.tiles_x) * TV_TH;
    r.x0 = (rem % a.tiles_x) * TV_TW;
    return r;
}

// The halo of tile `t` from global memory into registers: zero outside the H x W domain, source pixel (y >> 1, x >> 1) with `up`.
template <int CI>
__device__ __forceinline__ void tv_fetch(const TvArgs& a, long long t, int tid, uint4 (&pre)[TvGeom<CI>::ITERS]) {
    using G = TvGeom<CI>;
    const TvTile tl = tv_tile(a, t);
#pragma unroll
    for (int it = 0; it < G::ITERS; ++it) {
        const int c = tid + it * TV_THREADS;
        uint4 v = {0u, 0u, 0u, 0u};
        if (c < G::CHUNKS) {
            const int pix = c / G::CPP, k = c % G::CPP;
            const int cy = tl.y0 - 1 + pix / TV_HW, cx = tl.x0 - 1 + pix % TV_HW;
            if (cy >= 0 && cy < a.H && cx >= 0 && cx < a.W) {
                const int sy = a.up ? cy >> 1 : cy, sx = a.up ? cx >> 1 : cx;
                v = bc_ld16(a.x + (((size_t)tl.b * a.Hin + sy) * a.Win + sx) * CI + k * 8);
            }
        }
        pre[it] = v;
    }
}

template <int CI>
__device__ __forceinline__ void tv_stage(h16* sX, int tid, const uint4 (&pre)[TvGeom<CI>::ITERS]) {
    using G = TvGeom<CI>;
#pragma unroll
    for (int it = 0; it < G::ITERS; ++it) {
        const int c = tid + it * TV_THREADS;
        if (c < G::CHUNKS) bc_st16(sX + (c / G::CPP) * G::PP + (c % G::CPP) * 8, pre[it]);
    }
}

__device__ __forceinline__ uint4 tv_pack8(const float (&v)[8]) {
    h16x8 h;
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = (h16)v[j];
    return *reinterpret_cast<uint4*>(&h);
}

template <int CI, int MT>
__global__ __launch_bounds__(TV_THREADS) void tiny_conv3x3_kernel(const TvArgs a) {
    using G = TvGeom<CI>;
    extern __shared__ __align__(16) unsigned char tv_smem[];
    h16* sW = reinterpret_cast<h16*>(tv_smem);
    h16* sX = sW + MT * 32 * G::WP;
    float* sB = reinterpret_cast<float*>(sX + TV_HPIX * G::PP);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

    uint4 pre[G::ITERS];
    long long t = blockIdx.x;
    if (t < a.ntiles) tv_fetch<CI>(a, t, tid, pre);

    // weights -> LDS, once per workgroup; rows the weight buffer does not have are zero
    // (unrolled: the 16-byte loads of a thread - 18 at 64 -> 64 - are in flight together instead of one latency after the other)
    constexpr int WCH = 9 * CI / 8, WTOT = MT * 32 * WCH;
#pragma unroll
    for (int it = 0; it < (WTOT + TV_THREADS - 1) / TV_THREADS; ++it) {
        const int c = tid + it * TV_THREADS;
        if (c < WTOT) {
            const int row = c / WCH, k = c % WCH;
            uint4 v = {0u, 0u, 0u, 0u};
            if (row < a.co_rows) v = bc_ld16(a.w + (size_t)row * (9 * CI) + k * 8);
            bc_st16(sW + row * G::WP + k * 8, v);
        }
    }
    if (tid < 64) sB[tid] = (a.bias != nullptr && tid < a.co) ? a.bias[tid] : 0.0f;

    // MFMA row rr of M tile t holds the channel whose accumulator register lands where the epilogue wants it (see the head of the file)
    const int hh = (r >> 2) & 1, ri = (r & 3) + 4 * (r >> 3);
    int wrow[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) wrow[m] = (MT == 2 ? 32 * hh + 16 * m + ri : 16 * hh + ri) * G::WP + 8 * h;

    for (; t < a.ntiles; t += gridDim.x) {
        const TvTile tl = tv_tile(a, t);
        tv_stage<CI>(sX, tid, pre);
        __syncthreads();                                   // halo (and, the first time, weights and bias) visible
        if (t + gridDim.x < a.ntiles) tv_fetch<CI>(a, t + gridDim.x, tid, pre);

        f32x16 acc[2][MT];
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[n][m][i] = 0.0f;

#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int ky = tap / 3, kx = tap % 3;
#pragma unroll
            for (int s = 0; s < G::KS; ++s) {
                h16x8 fa[MT], fb[2];
                const bool live = CI >= 16 || h == 0;      // CI = 8: k = 8 .. 15 of the step does not exist
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    fa[m] = (h16x8)(h16)0;
                    if (live) fa[m] = *reinterpret_cast<const h16x8*>(sW + wrow[m] + tap * CI + s * 16);
                }
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    fb[n] = (h16x8)(h16)0;
                    if (live) fb[n] = *reinterpret_cast<const h16x8*>(sX + ((2 * wave + n + ky) * TV_HW + r + kx) * G::PP + s * 16 + 8 * h);
                }
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int m = 0; m < MT; ++m) acc[n][m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[m], fb[n], acc[n][m], 0, 0, 0);
            }
        }

        // ---- epilogue: lane (r, h) holds pixel (y0 + 2 wave + n, x0 + r)
        const int ox = tl.x0 + r;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int oy = tl.y0 + 2 * wave + n;
            if (oy >= a.H || ox >= a.W) continue;
            const size_t pix = ((size_t)tl.b * a.H + oy) * a.W + ox;
            if constexpr (MT == 2) {
                // channels 32 h .. 32 h + 31: bias, skip, ReLU in fp32, one rounding, four 16-byte stores
                h16* dst = reinterpret_cast<h16*>(a.out) + pix * 64 + 32 * h;
                const h16* sk = a.skip ? a.skip + pix * 64 + 32 * h : nullptr;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float v[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = acc[n][q >> 1][(q & 1) * 8 + j] + sB[32 * h + 8 * q + j];
                    if (sk) {
                        const uint4 raw = bc_ld16(sk + 8 * q);
                        const h16x8 s8 = *reinterpret_cast<const h16x8*>(&raw);
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] += (float)s8[j];
                    }
                    if (a.relu) {
#pragma unroll
                        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.0f);
                    }
                    bc_st16(dst + 8 * q, tv_pack8(v));
                }
            } else {
                if (h != 0) continue;                      // channels 0 .. 2 are registers 0 .. 2 of the lower half-wave
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float v = 2.0f * (acc[n][0][c] + sB[c]) - 1.0f;
                    if (a.out_mode == BC_TINY_OUT_IMAGE) {
                        reinterpret_cast<float*>(a.out)[(((size_t)tl.b * 3 + c) * a.H + oy) * a.W + ox] = v;
                    } else {
                        const float q = fminf(fmaxf(v / 2.0f + 0.5f, 0.0f), 1.0f) * 255.0f;
                        reinterpret_cast<unsigned char*>(a.out)[pix * 3 + c] = (unsigned char)(int)rintf(q);
                    }
                }
            }
        }
        __syncthreads();                                   // every wave is done with the halo before the next one is staged
    }
}

__global__ __launch_bounds__(256) void tiny_latents_in_kernel(const float* __restrict__ z, long long pixels, long long hw, h16* __restrict__ out) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const long long b = p / hw, i = p - b * hw;
    float v[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) v[c] = tanhf(z[(b * 4 + c) * hw + i] / 3.0f) * 3.0f;
#pragma unroll
    for (int c = 4; c < 8; ++c) v[c] = 0.0f;
    bc_st16(out + p * 8, tv_pack8(v));
}

int tv_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        cus = 256;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    }
    return cus;
}

template <int CI, int MT>
int tv_launch(const TvArgs& a, hipStream_t stream) {
    static std::atomic<unsigned long long> lds_set{0};
    constexpr int lds = tv_lds_bytes<CI, MT>();
    BC_CHECK_HIP(bc_set_max_lds(lds_set, reinterpret_cast<const void*>(&tiny_conv3x3_kernel<CI, MT>), lds));
    const int grid = (int)std::min<long long>(a.ntiles, tv_cus());
    hipLaunchKernelGGL((tiny_conv3x3_kernel<CI, MT>), dim3(grid), dim3(TV_THREADS), lds, stream, a);
    BC_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int bc_tiny_conv3x3(const bc_tiny_conv_args* p, bc_stream stream) {
    BC_CHECK_ARG(p != nullptr, "bc_tiny_conv3x3: null arguments");
    BC_CHECK_ARG(p->x && p->w && p->out, "bc_tiny_conv3x3: null pointer");
    BC_CHECK_ARG(p->B >= 1 && p->H >= 1 && p->W >= 1 && p->H <= (1 << 20) && p->W <= (1 << 20), "bc_tiny_conv3x3: bad shape B=%d H=%d W=%d", p->B,
                 p->H, p->W);
    BC_CHECK_ARG(p->Ci == 8 || p->Ci == 64, "bc_tiny_conv3x3: Ci=%d (8 or 64)", p->Ci);
    BC_CHECK_ARG(p->Co == 64 || p->Co == 3, "bc_tiny_conv3x3: Co=%d (64 or 3)", p->Co);
    BC_CHECK_ARG(p->out_mode >= BC_TINY_OUT_F16 && p->out_mode <= BC_TINY_OUT_U8, "bc_tiny_conv3x3: out_mode=%d", p->out_mode);
    if (p->Co == 64) {
        BC_CHECK_ARG(p->out_mode == BC_TINY_OUT_F16, "bc_tiny_conv3x3: Co=64 stores fp16 NHWC, not out_mode=%d", p->out_mode);
    } else {
        BC_CHECK_ARG(p->out_mode != BC_TINY_OUT_F16, "bc_tiny_conv3x3: Co=3 stores the image (out_mode 1 or 2), not out_mode=%d", p->out_mode);
        BC_CHECK_ARG(p->Ci == 64 && !p->up && !p->skip && !p->relu, "bc_tiny_conv3x3: the Co=3 form takes Ci=64 and no up, skip or relu");
    }
    BC_CHECK_ARG(p->Ci == 64 || (!p->up && !p->skip), "bc_tiny_conv3x3: the Ci=8 form takes no up and no skip");
    BC_CHECK_ARG(!p->up || (p->H % 2 == 0 && p->W % 2 == 0), "bc_tiny_conv3x3: up needs an even output size, not H=%d W=%d", p->H, p->W);
    const uintptr_t al = (uintptr_t)p->x | (uintptr_t)p->w | (uintptr_t)p->skip | (p->out_mode == BC_TINY_OUT_F16 ? (uintptr_t)p->out : 0);
    BC_CHECK_ARG(al % 16 == 0, "bc_tiny_conv3x3: x, w, skip and an fp16 out need 16-byte alignment");
    BC_CHECK_ARG((uintptr_t)p->bias % 4 == 0 && (p->out_mode != BC_TINY_OUT_IMAGE || (uintptr_t)p->out % 4 == 0),
                 "bc_tiny_conv3x3: bias and an fp32 out are aligned fp32");
    TvArgs a;
    a.x = reinterpret_cast<const h16*>(p->x);
    a.w = reinterpret_cast<const h16*>(p->w);
    a.bias = p->bias;
    a.skip = reinterpret_cast<const h16*>(p->skip);
    a.out = p->out;
    a.B = p->B; a.H = p->H; a.W = p->W;
    a.Hin = p->up ? p->H / 2 : p->H;
    a.Win = p->up ? p->W / 2 : p->W;
    a.co = p->Co;
    a.co_rows = p->Co == 64 ? 64 : 8;
    a.up = p->up ? 1 : 0; a.relu = p->relu ? 1 : 0; a.out_mode = p->out_mode;
    a.tiles_x = bc_ceil_div(p->W, TV_TW);
    a.tiles_y = bc_ceil_div(p->H, TV_TH);
    a.ntiles = (long long)p->B * a.tiles_x * a.tiles_y;
    BC_CHECK_ARG((long long)a.tiles_x * a.tiles_y < (1ll << 31), "bc_tiny_conv3x3: H=%d W=%d too large", p->H, p->W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (p->Co == 3) return tv_launch<64, 1>(a, s);
    if (p->Ci == 8) return tv_launch<8, 2>(a, s);
    return tv_launch<64, 2>(a, s);
}

extern "C" int bc_tiny_conv3x3_flat(const bc_half* x, const bc_half* w, const float* bias, const bc_half* skip, void* out, int B, int H, int W, int Ci,
                                    int Co, int up, int relu, int out_mode, bc_stream stream) {
    bc_tiny_conv_args a;
    a.x = x; a.w = w; a.bias = bias; a.skip = skip; a.out = out;
    a.B = B; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.up = up; a.relu = relu; a.out_mode = out_mode;
    return bc_tiny_conv3x3(&a, stream);
}

extern "C" int bc_tiny_latents_in(const float* z, int B, int h, int w, bc_half* out, bc_stream stream) {
    BC_CHECK_ARG(z && out, "bc_tiny_latents_in: null pointer");
    BC_CHECK_ARG(B >= 1 && h >= 1 && w >= 1, "bc_tiny_latents_in: bad shape B=%d h=%d w=%d", B, h, w);
    BC_CHECK_ARG((uintptr_t)z % 4 == 0 && (uintptr_t)out % 16 == 0, "bc_tiny_latents_in: z is aligned fp32 and out needs 16-byte alignment");
    const long long hw = (long long)h * w, pixels = hw * B;
    BC_CHECK_ARG(pixels < (1ll << 38), "bc_tiny_latents_in: B=%d h=%d w=%d too large", B, h, w);
    hipLaunchKernelGGL(tiny_latents_in_kernel, dim3(bc_ceil_div(pixels, 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), z, pixels, hw,
                       reinterpret_cast<h16*>(out));
    BC_CHECK_LAUNCH();
    return 0;
}
