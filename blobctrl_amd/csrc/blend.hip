// Masked edits (include/blobctrl_blend.h): the step of a blend plan - an instance of the one step body (bc_cfg_step.h) with the BLEND
// term, with or without the perturbed-attention term - and the uint8 mask of an edit at latent resolution.
#include "bc_cfg_step.h"
#include "../../include/blobctrl_blend.h"

namespace {

template <bool PAG, bool SINGLE, bool NOISE, bool THIRD>
__global__ void blend_step_kernel(const float* __restrict__ eps, float* __restrict__ latents, const float* __restrict__ coef,
                                  const int* __restrict__ step_idx, float* __restrict__ hist, const float* __restrict__ pag_table,
                                  const float* __restrict__ image, const float* __restrict__ bnoise, const float* __restrict__ mask,
                                  const float* __restrict__ blend_table, int B, int h, int w, const float* __restrict__ noise, int nsteps,
                                  float* __restrict__ eps_out) {
    cfg_step_body<SINGLE, NOISE, THIRD, true, false, PAG, true>(eps, latents, coef, step_idx, hist, -1.f, B, h, w, noise, nsteps, eps_out,
                                                                 pag_table, image, bnoise, mask, blend_table);
}

using BlendStep = void (*)(const float*, float*, const float*, const int*, float*, const float*, const float*, const float*, const float*,
                           const float*, int, int, int, const float*, int, float*);
#define BLEND_FORMS(PAG)                                                                                                               \
    blend_step_kernel<PAG, false, false, false>, blend_step_kernel<PAG, false, false, true>, blend_step_kernel<PAG, false, true, false>, \
        blend_step_kernel<PAG, false, true, true>, blend_step_kernel<PAG, true, false, false>, blend_step_kernel<PAG, true, false, true>, \
        blend_step_kernel<PAG, true, true, false>, blend_step_kernel<PAG, true, true, true>
const BlendStep blend_steps[16] = {BLEND_FORMS(false), BLEND_FORMS(true)};      // index pag * 8 + step_form(single, noise, third)

// out[i][y][x] = mask[i][8y][8x] >= 128: one thread per latent pixel, total = n * (H / 8) * (W / 8)
__global__ void blend_mask_kernel(const unsigned char* __restrict__ mask, float* __restrict__ out, int total, int H, int W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int w = W / 8, h = H / 8;
    const int x = i % w, y = (i / w) % h, img = i / (w * h);
    out[i] = mask[((size_t)img * H + 8 * y) * W + 8 * x] >= 128 ? 1.f : 0.f;
}

}  // namespace

extern "C" int bc_blend_scheduler_step(const float* eps, float* latents, const float* coef, int* step_idx, float* hist,
                                       const float* pag_table, const float* image, const float* bnoise, const float* mask,
                                       const float* blend_table, int B, int h, int w, const float* noise, int nsteps, int third, int single,
                                       float* eps_out, int advance, bc_stream stream) {
    return step_launch("bc_blend_scheduler_step", eps && latents && coef && step_idx && hist && image && bnoise && mask && blend_table &&
                       B > 0 && h > 0 && w > 0 && nsteps > 0 && (long long)B * 4 * h * w < (1ll << 31),
                       blend_steps[(pag_table ? 8 : 0) + step_form(single, noise, third)], B, h, w, step_idx, advance, stream, eps, latents,
                       coef, step_idx, hist, pag_table, image, bnoise, mask, blend_table, B, h, w, noise, nsteps, eps_out);
}

extern "C" int bc_blend_mask(const unsigned char* mask, float* out, int n, int H, int W, bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(mask && out && n > 0 && H > 0 && W > 0, "bc_blend_mask: bad args");
    BC_CHECK_ARG(H % 8 == 0 && W % 8 == 0, "bc_blend_mask: H (%d) and W (%d) must be multiples of 8", H, W);
    BC_CHECK_ARG((long long)n * H * W < (1ll << 31), "bc_blend_mask: n * H * W must be below 2^31");
    const int total = n * (H / 8) * (W / 8);
    hipLaunchKernelGGL(blend_mask_kernel, dim3(bc_ceil_div(total, 256)), dim3(256), 0, stream, mask, out, total, H, W);
    BC_CHECK_LAUNCH();
    return 0;
}
