// FreeU (https://arxiv.org/abs/2309.11497) in front of the channel concat of an up block, gfx950: one launch per site does both halves.
//
// Reference call sites replaced: apply_freeu (D/utils/torch_utils.py:123-148) in front of torch.cat([hidden_states, res_hidden_states])
// of up_blocks.0 / up_blocks.1 (D/models/unets/unet_2d_blocks.py:2535-2557, 2695-2717):
//   hidden[:, :C_h // 2] *= b_stage
//   skip = fourier_filter(skip, threshold=1, scale=s_stage)                      (torch_utils.py:93-120)
// With threshold 1 the fft-shifted mask box covers the frequency indices ky in {0, H - 1}, kx in {0, W - 1} (sets: H = 1 leaves one row
// index) and the reference keeps the real part of the inverse transform, so for a real map x[y][x] of one (image, channel), with
// theta_k = 2 pi (ky y / H + kx x / W):
//   A_k = sum x cos theta_k, S_k = sum x sin theta_k
//   out = x + (s - 1) / (H W) * sum_k (A_k cos theta_k + S_k sin theta_k)
// - at most four frequency pairs, eight real sums per map (the DC sine is zero), and a rank <= 4 update: no FFT.  The host tabulates
// (cos theta_k, sin theta_k) per token in fp64 for the DEDUPLICATED frequency list (engine.freeu_basis: [HW][4][2] fp32, unused pairs
// zero), so the kernel runs no device sincos and does not depend on H or W beyond their product.
//
// Work shape: lanes run along channels, 16 bytes (8 x fp16) per lane.  A workgroup owns one image and a slab of 64 channels of ONE of
// the two tensors (grid.x = slabs of hidden, then slabs of skip): 8 channel lanes x 32 token groups.  A skip workgroup accumulates the
// eight sums of its channels over all tokens in fp32, combines them across its token groups (wave shuffles, then LDS in wave order:
// a fixed order, so the result is bit-reproducible), and walks its tokens a second time - an L2-resident re-read - to write.  A hidden
// workgroup scales (channels below C_h / 2) or copies in one pass.  Both emit the GroupNorm statistics of what they STORED (the fp16
// values) as per-channel totals, the format of a bc_gn_stats pass: each (image, channel) has exactly one adding workgroup.
// The parameters (s1, s2, b1, b2) are read from device memory: one plan and one captured graph serve every setting.
#include "bc_common.h"

namespace {

constexpr int FU_CH_LANES = 8;                       // lanes along channels: 8 x 8 = 64 channels = 128 bytes of a token row
constexpr int FU_SLAB = FU_CH_LANES * 8;
constexpr int FU_TOK_GROUPS = 256 / FU_CH_LANES;     // 32 token groups: 8 per wave
constexpr int FU_PAIRS = 4;                          // frequency pairs of the basis table (unused ones are zero rows)

// Sum of v over the 8 token groups of a wave (lanes l, l ^ 8, l ^ 16, l ^ 32 hold the same channels).
__device__ __forceinline__ float fu_wave_groups_sum(float v) {
    v += __shfl_xor(v, 8);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

// acc[N] per thread -> the sum over all 32 token groups, in every thread of the channel lane (wave order through LDS).
template <int N>
__device__ __forceinline__ void fu_block_sum(float (&acc)[N], float* red /* [4][FU_CH_LANES][N] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cl = lane & (FU_CH_LANES - 1);
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = fu_wave_groups_sum(acc[i]);
    __syncthreads();                                 // (the previous use of `red` is over)
    if (lane < FU_CH_LANES) {
#pragma unroll
        for (int i = 0; i < N; ++i) red[(wave * FU_CH_LANES + cl) * N + i] = acc[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[(w * FU_CH_LANES + cl) * N + i];
        acc[i] = s;
    }
}

__global__ __launch_bounds__(256) void freeu_kernel(const h16* __restrict__ hidden, int C_h, const h16* __restrict__ skip, int C_s, int HW,
                                                    const float* __restrict__ params, int stage, const float* __restrict__ basis,
                                                    h16* __restrict__ hidden_out, h16* __restrict__ skip_out,
                                                    unsigned long long* __restrict__ tot_h, unsigned long long* __restrict__ tot_s) {
    __shared__ float red[4 * FU_CH_LANES * 64];      // 8 KiB: the cross-wave reduction (64 = 8 channels x 8 sums per lane)
    const int b = blockIdx.y;
    const int slabs_h = (C_h + FU_SLAB - 1) / FU_SLAB;
    const bool is_skip = (int)blockIdx.x >= slabs_h;
    const int slab = is_skip ? blockIdx.x - slabs_h : blockIdx.x;
    const int C = is_skip ? C_s : C_h;
    const int cl = threadIdx.x & (FU_CH_LANES - 1), tg = threadIdx.x / FU_CH_LANES;
    const int c0 = slab * FU_SLAB + cl * 8;          // first of this lane's 8 channels
    const bool live = c0 < C;                        // slab tail (C % 8 == 0: a live lane has all 8 channels)
    const h16* src = (is_skip ? skip : hidden) + (size_t)b * HW * C + c0;
    h16* dst = (is_skip ? skip_out : hidden_out) + (size_t)b * HW * C + c0;
    float st[16];                                    // (sum, sum of squares) of the stored values, per channel
#pragma unroll
    for (int j = 0; j < 16; ++j) st[j] = 0.f;

    if (!is_skip) {
        const float bscale = params[2 + stage];
        const int half = C_h / 2;
        if (live) {
            for (int p = tg; p < HW; p += FU_TOK_GROUPS) {
                uint4 raw = bc_ld16(src + (size_t)p * C);
                h16* v = reinterpret_cast<h16*>(&raw);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (c0 + j < half) v[j] = (h16)((float)v[j] * bscale);
                    const float f = (float)v[j];
                    st[2 * j] += f;
                    st[2 * j + 1] += f * f;
                }
                bc_st16(dst + (size_t)p * C, raw);
            }
        }
    } else {
        const float g = (params[stage] - 1.0f) / (float)HW;
        float acc[64];                               // [channel j][pair k]: A_k at 8 j + 2 k, S_k at 8 j + 2 k + 1
#pragma unroll
        for (int i = 0; i < 64; ++i) acc[i] = 0.f;
        if (live) {
            for (int p = tg; p < HW; p += FU_TOK_GROUPS) {
                const uint4 raw = bc_ld16(src + (size_t)p * C);
                const h16* v = reinterpret_cast<const h16*>(&raw);
                const float4 t0 = *reinterpret_cast<const float4*>(basis + (size_t)p * 2 * FU_PAIRS);
                const float4 t1 = *reinterpret_cast<const float4*>(basis + (size_t)p * 2 * FU_PAIRS + 4);
                const float cs[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float f = (float)v[j];
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[8 * j + k] = fmaf(f, cs[k], acc[8 * j + k]);
                }
            }
        }
        fu_block_sum<64>(acc, red);
#pragma unroll
        for (int i = 0; i < 64; ++i) acc[i] *= g;    // out = x + sum_k (g A_k) cos_k + (g S_k) sin_k
        if (live) {
            for (int p = tg; p < HW; p += FU_TOK_GROUPS) {
                const uint4 raw = bc_ld16(src + (size_t)p * C);
                const h16* v = reinterpret_cast<const h16*>(&raw);
                const float4 t0 = *reinterpret_cast<const float4*>(basis + (size_t)p * 2 * FU_PAIRS);
                const float4 t1 = *reinterpret_cast<const float4*>(basis + (size_t)p * 2 * FU_PAIRS + 4);
                const float cs[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
                uint4 outraw;
                h16* o = reinterpret_cast<h16*>(&outraw);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float d = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) d = fmaf(acc[8 * j + k], cs[k], d);
                    o[j] = (h16)((float)v[j] + d);
                    const float f = (float)o[j];
                    st[2 * j] += f;
                    st[2 * j + 1] += f * f;
                }
                bc_st16(dst + (size_t)p * C, outraw);
            }
        }
    }
    fu_block_sum<16>(st, red);
    if (live && tg == 0) {
        unsigned long long* t = (is_skip ? tot_s : tot_h) + ((size_t)b * C + c0) * BC_GN_TOT_WORDS;
#pragma unroll
        for (int j = 0; j < 8; ++j) bc_gn_tot_add(t + (size_t)j * BC_GN_TOT_WORDS, st[2 * j], st[2 * j + 1]);
    }
}

}  // namespace

extern "C" int bc_freeu(const bc_half* hidden, int C_h, const bc_half* skip, int C_s, int B, int HW, const float* params, int stage,
                        const float* basis, bc_half* hidden_out, bc_half* skip_out, unsigned long long* tot_h, unsigned long long* tot_s,
                        bc_stream stream_) {
    BC_CHECK_ARG(hidden && skip && params && basis && hidden_out && skip_out && tot_h && tot_s, "bc_freeu: null pointer");
    BC_CHECK_ARG(B > 0 && B <= 65535 && HW > 0 && C_h > 0 && C_s > 0 && C_h % 8 == 0 && C_s % 8 == 0,
                 "bc_freeu: bad shape B=%d HW=%d C_h=%d C_s=%d (widths %% 8 == 0)", B, HW, C_h, C_s);
    BC_CHECK_ARG(stage == 0 || stage == 1, "bc_freeu: stage %d (FreeU runs in up_blocks.0 and up_blocks.1 only)", stage);
    BC_CHECK_ARG((const void*)hidden_out != (const void*)hidden && (const void*)skip_out != (const void*)skip &&
                     (const void*)hidden_out != (const void*)skip_out,
                 "bc_freeu: the outputs are buffers of their own (the second pass re-reads the inputs)");
    const uintptr_t al = (uintptr_t)hidden | (uintptr_t)skip | (uintptr_t)hidden_out | (uintptr_t)skip_out | (uintptr_t)basis;
    BC_CHECK_ARG(al % 16 == 0, "bc_freeu: tensors and the basis table need 16-byte alignment");
    const int slabs = bc_ceil_div(C_h, FU_SLAB) + bc_ceil_div(C_s, FU_SLAB);
    hipLaunchKernelGGL(freeu_kernel, dim3(slabs, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream_),
                       reinterpret_cast<const h16*>(hidden), C_h, reinterpret_cast<const h16*>(skip), C_s, HW, params, stage, basis,
                       reinterpret_cast<h16*>(hidden_out), reinterpret_cast<h16*>(skip_out), tot_h, tot_s);
    BC_CHECK_LAUNCH();
    return 0;
}
