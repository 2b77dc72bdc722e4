// Perturbed-attention guidance (include/blobctrl_pag.h): the identity attention of the perturbed images - a transpose copy of V^T into
// the attention output rows - and the guidance + scheduler step of a PAG plan, an instance of the one step body (bc_cfg_step.h).
#include "bc_cfg_step.h"
#include "../../include/blobctrl_pag.h"

namespace {

constexpr int kTile = 64;            // channels x tokens of one workgroup
constexpr int kPad = 8;              // halves behind every LDS row: rows stay 16-byte aligned for the staging stores

// out[(b * HW + p) * ldo + c] = vt[(b * C + c) * ldvt + p] for one 64-channel x 64-token tile of image b0 + blockIdx.z.  16-byte loads
// along the tokens (8 lanes cover 128 contiguous bytes of a V^T row), 16-byte stores along the channels (8 lanes cover 128 contiguous
// bytes of an output row); the transpose happens in the LDS reads.  A token chunk is loaded whenever it lies inside ldvt - the pad
// columns of vt among them - and stored only for tokens < HW; channel rows >= C are neither loaded nor stored.
__global__ __launch_bounds__(256) void attention_identity_kernel(const h16* __restrict__ vt, h16* __restrict__ out, int b0, int HW, int C,
                                                                 int ldvt, int ldo) {
    __shared__ __attribute__((aligned(16))) h16 tile[kTile][kTile + kPad];
    const int p0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile, b = b0 + blockIdx.z;
    const h16* src = vt + ((size_t)b * C + c0) * ldvt + p0;
    for (int k = threadIdx.x; k < kTile * kTile / 8; k += 256) {
        const int r = k >> 3, q = (k & 7) * 8;                    // channel row, first token of the chunk
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (c0 + r < C && p0 + q + 8 <= ldvt) v = bc_ld16(src + (size_t)r * ldvt + q);
        *reinterpret_cast<uint4*>(&tile[r][q]) = v;
    }
    __syncthreads();
    h16* dst = out + ((size_t)b * HW + p0) * ldo + c0;
    for (int k = threadIdx.x; k < kTile * kTile / 8; k += 256) {
        const int r = k >> 3, q = (k & 7) * 8;                    // token row, first channel of the chunk
        if (p0 + r >= HW || c0 + q >= C) continue;                // (C % 8 == 0: a chunk is inside [0, C) or outside)
        uint4 raw;
        h16* o = reinterpret_cast<h16*>(&raw);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = tile[q + j][r];
        bc_st16(dst + (size_t)r * ldo + q, raw);
    }
}

template <bool SINGLE, bool NOISE, bool THIRD>
__global__ void pag_step_kernel(const float* __restrict__ eps, float* __restrict__ latents, const float* __restrict__ coef,
                                const int* __restrict__ step_idx, float* __restrict__ hist, const float* __restrict__ pag_table, int B,
                                int h, int w, const float* __restrict__ noise, int nsteps, float* __restrict__ eps_out) {
    cfg_step_body<SINGLE, NOISE, THIRD, true, false, true>(eps, latents, coef, step_idx, hist, -1.f, B, h, w, noise, nsteps, eps_out,
                                                           pag_table);
}

using PagStep = void (*)(const float*, float*, const float*, const int*, float*, const float*, int, int, int, const float*, int, float*);
const PagStep pag_steps[8] = {pag_step_kernel<false, false, false>, pag_step_kernel<false, false, true>, pag_step_kernel<false, true, false>,
                              pag_step_kernel<false, true, true>,   pag_step_kernel<true, false, false>, pag_step_kernel<true, false, true>,
                              pag_step_kernel<true, true, false>,   pag_step_kernel<true, true, true>};

}  // namespace

extern "C" int bc_attention_identity(const bc_half* vt, bc_half* out, int B, int b0, int HW, int C, int ldvt, int ldo, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(vt && out && B > 0 && b0 >= 0 && b0 <= B && HW > 0 && C > 0, "bc_attention_identity: bad args");
    BC_CHECK_ARG(C % 8 == 0 && ldvt >= HW && ldvt % 8 == 0 && ldo >= C && ldo % 8 == 0,
                 "bc_attention_identity: C (%d), ldvt (%d) and ldo (%d) must be multiples of 8 with ldvt >= HW (%d) and ldo >= C", C, ldvt, ldo, HW);
    BC_CHECK_ARG(((uintptr_t)vt | (uintptr_t)out) % 16 == 0, "bc_attention_identity: vt and out must be 16-byte aligned");
    BC_CHECK_ARG(B - b0 <= 65535 && bc_ceil_div(C, kTile) <= 65535, "bc_attention_identity: too many images or channels for one grid");
    if (b0 == B) return 0;
    hipLaunchKernelGGL(attention_identity_kernel, dim3(bc_ceil_div(HW, kTile), bc_ceil_div(C, kTile), B - b0), dim3(256), 0, stream,
                       reinterpret_cast<const h16*>(vt), reinterpret_cast<h16*>(out), b0, HW, C, ldvt, ldo);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_pag_scheduler_step(const float* eps, float* latents, const float* coef, int* step_idx, float* hist, const float* pag_table,
                                     int B, int h, int w, const float* noise, int nsteps, int third, int single, float* eps_out,
                                     int advance, bc_stream stream) {
    return step_launch("bc_pag_scheduler_step", eps && latents && coef && step_idx && hist && pag_table && B > 0 && h > 0 && w > 0 &&
                       nsteps > 0 && (long long)B * 4 * h * w < (1ll << 31), pag_steps[step_form(single, noise, third)], B, h, w, step_idx,
                       advance, stream, eps, latents, coef, step_idx, hist, pag_table, B, h, w, noise, nsteps, eps_out);
}
