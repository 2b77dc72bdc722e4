// Crop + guidance + scheduler step: the ONE body behind every step entry point (elementwise.hip: bc_cfg_scheduler_step*,
// bc_scheduler_step_single, bc_scheduler_step_requests; pag.hip: bc_pag_scheduler_step; blend.hip: bc_blend_scheduler_step) and the host side they share.
#pragma once
#include "bc_common.h"

namespace {

// The BLEND term of cfg_step_body and the store of latents[i]: *dst = (1 - m) * (a * image + s * bnoise) + m * xn, compiled without
// contraction - one rounding per written operation - and never inlined (see the call).
__device__ __noinline__ void blend_store(float* dst, float xn, float a, float s, float image, float bnoise, float m) {
#pragma clang fp contract(off)
    const float pa = a * image, ps = s * bnoise;
    const float p = pa + ps;
    const float keep = (1.f - m) * p, repaint = m * xn;
    *dst = keep + repaint;
}

// Crop (right half) + classifier-free guidance + scheduler step, specialised at compile time.  cf = coef row *step_idx (16 floats; the
// full column table is at the top of blobctrl_amd/schedulers.py).
//   NOISE: x_next += cf[12] * noise[step][i], the variance noise of stochastic DDIM (scheduling_ddim.py:438-466) and SDE-DPM-Solver++;
//          noise fp32 [nsteps][B][4][h][w]
//   THIRD: x_next += cf[13] * x0_{i-2}, third-order DPM-Solver++ (scheduling_dpmsolver_multistep.py:804-887), read from the hist slot
//          m1 that every instantiation already loads
//   GUARD: a step index outside [0, nsteps) (the capture warm-ups advance the counter) has no table row and no noise slice: the
//          launch then leaves every buffer as it is.  The plain entry point has no nsteps in its ABI, hence no guard.
//   SINGLE: a guidance-free (single-pass) plan: eps holds B images, not 2B, and e is the right half of image b as it is - no second
//          read, no guidance arithmetic, `guidance` and column 11 are not read (pipe:1031, 1095: do_classifier_free_guidance False).
//   REQ:   a batch of edit requests with their own tables: coef is [B][nsteps][16] and image b applies ITS row, guidance (column 11)
//          included.  Column 15 != 0 marks a request that has finished: its elements are left alone - nothing of image b is loaded from
//          eps and nothing is stored, eps_out included - whatever the networks put out for it (a non-finite value included).
//   PAG:   perturbed-attention guidance (pag_utils.py:_apply_perturbed_attention_guidance): eps holds B more images behind the others,
//          the perturbed ones, and e += s * (e_cond - e_perturbed) with s = pag_table[step] (fp32 [nsteps]) - with SINGLE on
//          [cond | perturbed], e = e_c + s * (e_c - e_p); else on [uncond | cond | perturbed], e = e_u + g * (e_c - e_u) + s * (e_c - e_p).
//   BLEND: a masked edit (the reference stack's pipeline_stable_diffusion_inpaint.py:1272-1285): after the step, noise and third-order
//          terms included, x_next = (1 - m) * (a * image[i] + s * bnoise[i]) + m * x_next with (a, s) = blend_table[step] (fp32
//          [nsteps][2]: add_noise to the NEXT timestep) and m = mask[b][yy][xx], one value for the 4 channels.  Rounded operation by
//          operation as written (no contraction), so m == 0 stores exactly a * image + s * bnoise and m == 1 exactly the step's result.
// `noise` / `nsteps` are not read by an instantiation without NOISE / GUARD, `pag_table` by none without PAG, the four blend operands by
// none without BLEND.
template <bool SINGLE, bool NOISE, bool THIRD, bool GUARD, bool REQ = false, bool PAG = false, bool BLEND = false>
__device__ __forceinline__ void cfg_step_body(const float* __restrict__ eps, float* __restrict__ latents, const float* __restrict__ coef,
                                              const int* __restrict__ step_idx, float* __restrict__ hist, float guidance, int B, int h,
                                              int w, const float* __restrict__ noise, int nsteps, float* __restrict__ eps_out,
                                              const float* __restrict__ pag_table = nullptr, const float* __restrict__ bl_image = nullptr,
                                              const float* __restrict__ bl_noise = nullptr, const float* __restrict__ bl_mask = nullptr,
                                              const float* __restrict__ bl_table = nullptr) {
    const int n = B * 4 * h * w;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int step = *step_idx;
    if (i >= n) return;
    if (GUARD && (step < 0 || step >= nsteps)) return;
    const float* cf = coef + (size_t)step * 16;
    const int xx = i % w;
    const int yy = (i / w) % h;
    const int c = (i / (w * h)) % 4;
    const int b = i / (4 * w * h);
    if (REQ) {
        cf = coef + ((size_t)b * nsteps + step) * 16;
        if (cf[15] != 0.f) return;
    }
    // eps token-major [2B][h][2w][4]; right half, uncond = batch b, cond = batch B + b   (pipe:1092-1098)
    const size_t pu = (((size_t)b * h + yy) * (2 * w) + (w + xx)) * 4 + c;
    const size_t image = (size_t)B * h * (2 * w) * 4;                 // elements of B images of eps
    float e;
    if (SINGLE) {
        e = eps[pu];                                              // eps token-major [B][h][2w][4]
        if (PAG) e = e + pag_table[step] * (e - eps[pu + image]);     // [cond | perturbed]
    } else {
        const size_t pc = (((size_t)(B + b) * h + yy) * (2 * w) + (w + xx)) * 4 + c;
        const float eu = eps[pu], ec = eps[pc];
        const float gscale = guidance >= 0.f ? guidance : cf[11];     // < 0: read from the coefficient table (graph-replay safe)
        e = eu + gscale * (ec - eu);
        if (PAG) e = e + pag_table[step] * (ec - eps[pc + image]);    // [uncond | cond | perturbed]
    }
    if (eps_out) eps_out[i] = e;
    const float x = latents[i];
    float* m0 = hist, *m1 = hist + n, *last = hist + 2 * (size_t)n;
    const float x0 = x * cf[0] - e * cf[1];
    float xc = x;
    const float pm0 = m0[i], pm1 = m1[i];
    if (cf[2] != 0.f) xc = cf[3] * last[i] + cf[4] * pm0 + cf[5] * pm1 + cf[6] * x0;
    float xn = cf[7] * xc + cf[8] * x0 + cf[9] * pm0 + cf[10] * e;
    m1[i] = pm0;
    m0[i] = x0;
    last[i] = xc;
    // the optional terms come last, after the history stores: every instantiation is the plain step up to here
    if (NOISE) xn = xn + cf[12] * noise[(size_t)step * n + i];
    if (THIRD) xn = xn + cf[13] * pm1;
    if (BLEND) {
        // xn is a finished value here, where the other instantiations store it.  The blend and the store are a call of their own: to
        // the compiler the step's arithmetic ends in one use of xn, as it does in their store, so it compiles to the same operations
        // and the m == 1 bits are theirs (inlined, the blend's products regroup the step's and its roundings change)
        blend_store(latents + i, xn, bl_table[2 * step], bl_table[2 * step + 1], bl_image[i], bl_noise[i],
                    bl_mask[((size_t)b * h + yy) * w + xx]);
        return;
    }
    latents[i] = xn;
}

__global__ void advance_kernel(int* step_idx) { *step_idx += 1; }

// The host side of every step entry point: `ok` is the entry point's argument check (`name` = its own name for the error text), then
// the launch of its kernel instance over the B * 4 * h * w latent elements and, with `advance`, of the step counter's increment.
template <typename... Params, typename... Args>
int step_launch(const char* name, bool ok, void (*kernel)(Params...), int B, int h, int w, int* step_idx, int advance,
                bc_stream stream_, Args... args) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(ok, "%s: bad args", name);
    hipLaunchKernelGGL(kernel, dim3(bc_ceil_div(B * 4 * h * w, 256)), dim3(256), 0, stream, args...);
    BC_CHECK_LAUNCH();
    if (advance) {
        hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, stream, step_idx);
        BC_CHECK_LAUNCH();
    }
    return 0;
}

// The entry points that take their step form at run time pick the instance from a table, index single * 4 + noise * 2 + third.
inline int step_form(bool single, bool noise, bool third) { return (single ? 4 : 0) | (noise ? 2 : 0) | (third ? 1 : 0); }

}  // namespace
