// Tiled VAE encode / decode, gfx950: the blend / crop / scatter step between a tile's plan replay and the stitched result.
//
// Reference call sites replaced: blend_v / blend_h (D/models/autoencoders/autoencoder_kl.py:328-338) and the `[:limit, :limit]` crop +
// torch.cat of tiled_encode / tiled_decode (autoencoder_kl.py:374-387, 425-438).  The reference blends IN PLACE and in row-major order,
// so the `above` and `left` operands of a tile are the neighbours' BLENDED values: the host driver (vae.py) launches this kernel once
// per tile in that order and hands it the neighbours' keep-buffers.  Per element of the tile, in fp32 with every product and the sum
// rounded separately (torch's mul, mul, add; the weights are Python doubles rounded to fp32 once):
//   v = src;  y < ev: v = above[ha - ev + y][x] * (1 - y / ev) + v * (y / ev);  x < eh: v = left[y][wl - eh + x] * (1 - x / eh) + v * (x / eh)
//   keep = v;  y < ch and x < cw: result[oy + y][ox + x] = v
//
// Work shape.  The kernel is a pure stream (no reuse): it reads the tile, writes the keep-buffer (both NHWC, the two streams that
// dominate the traffic) and writes at most as much again into the result.  A thread owns a run of pixels along x that makes its NHWC
// accesses 16-byte vectors - decode: 4 pixels x 3 channels of fp32 = three 16-byte loads and stores; encode: 1 pixel x 8 channels of
// fp16 = one 16-byte load, two 16-byte keep stores, one 16-byte result store - and consecutive lanes own consecutive runs, so a wave
// walks a tile row linearly.  The decode result is NCHW: the same thread's 4 pixels are 4 consecutive floats of each channel plane, one
// 16-byte store per plane when the origin, crop and row pitch allow it (they do whenever the tile sizes are multiples of 4 pixels),
// scalar stores otherwise.  The blend bands are thin (an eighth to a quarter of a tile each): their extra reads and the two fp64
// divisions per weight stay far below the stream.
#include "bc_common.h"
#include "../../include/blobctrl_vae.h"

namespace {

struct VtGeom {
    int B, th, tw, ha, wl, ev, eh, oy, ox, ch, cw, H, W;
};

__device__ __forceinline__ void vt_weights(int i, int e, float& w_nb, float& w_own) {
    const double r = (double)i / (double)e;
    w_nb = (float)(1.0 - r);
    w_own = (float)r;
}

__device__ __forceinline__ float vt_mix(float nb, float own, float w_nb, float w_own) {
#pragma clang fp contract(off)                                         // the reference rounds three times: no fused multiply-add
    const float p = nb * w_nb, q = own * w_own;
    return p + q;
}

// N consecutive fp32 values; 16-byte vectors when N is a multiple of 4 (the caller guarantees the alignment then)
template <int N>
__device__ __forceinline__ void vt_ld_f32(const float* p, float (&v)[N]) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) {
            const float4 t = reinterpret_cast<const float4*>(p)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = p[i];
    }
}

template <int N>
__device__ __forceinline__ void vt_st_f32(float* p, const float (&v)[N]) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N / 4; ++i) reinterpret_cast<float4*>(p)[i] = make_float4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = v[i];
    }
}

template <int MODE, int PX>
__global__ __launch_bounds__(256) void vae_tile_kernel(const void* __restrict__ src_, const float* __restrict__ above,
                                                       const float* __restrict__ left, float* __restrict__ keep, void* __restrict__ out_,
                                                       VtGeom g, int vec_out) {
    constexpr int C = MODE == BC_VAE_TILE_DECODE ? 3 : 8;
    constexpr int N = PX * C;
    const int runs = g.tw / PX;                                      // runs of PX pixels per tile row (PX divides tw)
    const unsigned items = (unsigned)g.B * g.th * runs;              // (the host refuses tiles of 2^28 pixels and more: 32-bit indices)
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const int x0 = (int)(it % runs) * PX;
        const unsigned row = it / runs;
        const int y = (int)(row % g.th), b = (int)(row / g.th);
        const size_t e0 = (((size_t)b * g.th + y) * g.tw + x0) * C;
        float v[N];
        if constexpr (MODE == BC_VAE_TILE_DECODE) {
            vt_ld_f32<N>(reinterpret_cast<const float*>(src_) + e0, v);
        } else {
            static_assert(PX == 1, "encode: one pixel (8 x fp16 = 16 bytes) per thread");
            const uint4 raw = bc_ld16(reinterpret_cast<const h16*>(src_) + e0);
            const h16* hv = reinterpret_cast<const h16*>(&raw);
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (float)hv[i];
        }
        if (above != nullptr && y < g.ev) {
            float a[N], w_nb, w_own;
            vt_ld_f32<N>(above + (((size_t)b * g.ha + (g.ha - g.ev + y)) * g.tw + x0) * C, a);
            vt_weights(y, g.ev, w_nb, w_own);
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = vt_mix(a[i], v[i], w_nb, w_own);
        }
        if (left != nullptr && x0 < g.eh) {
#pragma unroll
            for (int p = 0; p < PX; ++p) {
                const int x = x0 + p;
                if (x < g.eh) {
                    float l[C], w_nb, w_own;
                    vt_ld_f32<C>(left + (((size_t)b * g.th + y) * g.wl + (g.wl - g.eh + x)) * C, l);
                    vt_weights(x, g.eh, w_nb, w_own);
#pragma unroll
                    for (int c = 0; c < C; ++c) v[p * C + c] = vt_mix(l[c], v[p * C + c], w_nb, w_own);
                }
            }
        }
        vt_st_f32<N>(keep + e0, v);
        if (y >= g.ch || x0 >= g.cw) continue;
        if constexpr (MODE == BC_VAE_TILE_DECODE) {
            float* out = reinterpret_cast<float*>(out_);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float* o = out + (((size_t)b * C + c) * g.H + (g.oy + y)) * g.W + (g.ox + x0);
                if (PX == 4 && vec_out && x0 + PX <= g.cw) {
                    *reinterpret_cast<float4*>(o) = make_float4(v[c], v[C + c], v[2 * C + c], v[3 * C + c]);
                } else {
#pragma unroll
                    for (int p = 0; p < PX; ++p)
                        if (x0 + p < g.cw) o[p] = v[p * C + c];
                }
            }
        } else {
            uint4 raw;
            h16* hv = reinterpret_cast<h16*>(&raw);
#pragma unroll
            for (int i = 0; i < 8; ++i) hv[i] = (h16)v[i];
            bc_st16(reinterpret_cast<h16*>(out_) + (((size_t)b * g.H + (g.oy + y)) * g.W + (g.ox + x0)) * C, raw);
        }
    }
}

bool vt_overlap(const void* a, size_t na, const void* b, size_t nb) {
    if (a == nullptr || b == nullptr) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace

extern "C" int bc_vae_tile_blend(const void* src, const float* above, const float* left, float* keep, void* out, int mode, int B, int th,
                                 int tw, int ha, int wl, int ev, int eh, int oy, int ox, int ch, int cw, int H, int W, bc_stream stream_) {
    BC_CHECK_ARG(src && keep && out, "bc_vae_tile_blend: null pointer (src, keep and out are required)");
    BC_CHECK_ARG(mode == BC_VAE_TILE_DECODE || mode == BC_VAE_TILE_ENCODE, "bc_vae_tile_blend: mode %d (0 decode, 1 encode)", mode);
    BC_CHECK_ARG(B > 0 && th > 0 && tw > 0 && H > 0 && W > 0 && (long long)B * th * tw <= 0x7fffffffll / 8 &&
                     (long long)B * H * W <= 0x7fffffffll / 8,
                 "bc_vae_tile_blend: bad shape B=%d tile %dx%d result %dx%d", B, th, tw, H, W);
    BC_CHECK_ARG(above == nullptr || (ha > 0 && ev >= 0 && ev <= ha && ev <= th),
                 "bc_vae_tile_blend: vertical extent %d larger than a tile (above %d rows, own %d rows)", ev, ha, th);
    BC_CHECK_ARG(left == nullptr || (wl > 0 && eh >= 0 && eh <= wl && eh <= tw),
                 "bc_vae_tile_blend: horizontal extent %d larger than a tile (left %d columns, own %d columns)", eh, wl, tw);
    BC_CHECK_ARG(ch >= 0 && cw >= 0 && ch <= th && cw <= tw && oy >= 0 && ox >= 0 && oy <= H - ch && ox <= W - cw,
                 "bc_vae_tile_blend: crop %dx%d at (%d, %d) leaves the tile %dx%d or the result %dx%d", ch, cw, oy, ox, th, tw, H, W);
    const uintptr_t al = (uintptr_t)src | (uintptr_t)above | (uintptr_t)left | (uintptr_t)keep | (uintptr_t)out;
    BC_CHECK_ARG(al % 16 == 0, "bc_vae_tile_blend: every buffer needs 16-byte alignment");
    const int C = mode == BC_VAE_TILE_DECODE ? 3 : 8;
    const size_t esz = mode == BC_VAE_TILE_DECODE ? 4 : 2;
    const size_t n_src = (size_t)B * th * tw * C * esz, n_keep = (size_t)B * th * tw * C * 4, n_out = (size_t)B * H * W * C * esz;
    const size_t n_above = above ? (size_t)B * ha * tw * C * 4 : 0, n_left = left ? (size_t)B * th * wl * C * 4 : 0;
    BC_CHECK_ARG(!vt_overlap(keep, n_keep, src, n_src) && !vt_overlap(keep, n_keep, above, n_above) && !vt_overlap(keep, n_keep, left, n_left) &&
                     !vt_overlap(keep, n_keep, out, n_out) && !vt_overlap(out, n_out, src, n_src) && !vt_overlap(out, n_out, above, n_above) &&
                     !vt_overlap(out, n_out, left, n_left),
                 "bc_vae_tile_blend: keep and out are buffers of their own (they overlap an input or each other)");
    const VtGeom g = {B, th, tw, ha, wl, above ? ev : 0, left ? eh : 0, oy, ox, ch, cw, H, W};
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (mode == BC_VAE_TILE_ENCODE) {
        const int blocks = std::min(bc_ceil_div((long long)B * th * tw, 256), 2048);
        hipLaunchKernelGGL((vae_tile_kernel<BC_VAE_TILE_ENCODE, 1>), dim3(blocks), dim3(256), 0, stream, src, above, left, keep, out, g, 0);
    } else if (tw % 4 == 0) {
        const int vec_out = (W % 4 == 0 && ox % 4 == 0) ? 1 : 0;     // (a run then starts on a 16-byte boundary of its plane row)
        const int blocks = std::min(bc_ceil_div((long long)B * th * (tw / 4), 256), 2048);
        hipLaunchKernelGGL((vae_tile_kernel<BC_VAE_TILE_DECODE, 4>), dim3(blocks), dim3(256), 0, stream, src, above, left, keep, out, g, vec_out);
    } else {
        const int blocks = std::min(bc_ceil_div((long long)B * th * tw, 256), 2048);
        hipLaunchKernelGGL((vae_tile_kernel<BC_VAE_TILE_DECODE, 1>), dim3(blocks), dim3(256), 0, stream, src, above, left, keep, out, g, 0);
    }
    BC_CHECK_LAUNCH();
    return 0;
}
