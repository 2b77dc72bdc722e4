// IP-Adapter masks: the image cross-attention of an attn2 with one softmax PER IMAGE, each image's result weighted row by row with that
// image's mask, accumulated onto the text-attention output in place; and the bicubic downsampling that makes those masks.  gfx950.
//
// Reference call site replaced: IPAdapterAttnProcessor2_0 with ip_adapter_masks (D/models/attention_processor.py:3818-3849), per adapter
//   for i in images:  hidden_states += scale * (F.scaled_dot_product_attention(query, ip_key[i], ip_value[i]) * mask_downsample[i])
// and IPAdapterMaskProcessor.downsample (D/image_processor.py:969-1029) for mask_downsample.
//
// The scalar kernel is the MASKED form of the body in bc_attention_ip.h, which attention_ip.hip instantiates without a mask; the MFMA
// tiles, for images whose token count is a multiple of 16 (IP-Adapter Plus), are attention_ip_tiles_kernel of attention_ip.hip with the
// mask block in front and one softmax per image between the two products.  The mask block in LDS with its three skips, the softmax per
// image and the weight m[i, r] / l_i are described in the header.
#include "bc_attention_ip.h"
#include "../../include/blobctrl_ip_mask.h"

namespace {

template <int D>
__global__ __launch_bounds__(IP_THREADS) void attention_ip_masked_kernel(const h16* __restrict__ Q, const h16* __restrict__ K,
                                                                         const h16* __restrict__ V, h16* __restrict__ O, int rows_per_batch,
                                                                         int heads, int images, int Tp, int ldq, int ldkv, int ldo,
                                                                         float scale_log2, const float* __restrict__ w,
                                                                         const h16* __restrict__ mask, int ldm, int slab_heads, int block_rows) {
    attention_ip_body<D, true>(Q, K, V, O, rows_per_batch, heads, images, Tp, ldq, ldkv, ldo, scale_log2, w, mask, ldm, slab_heads, block_rows);
}

template <int D, int NT>
__global__ __launch_bounds__(IP_THREADS) void attention_ip_masked_tiles_kernel(const h16* __restrict__ Q, const h16* __restrict__ K,
                                                                                const h16* __restrict__ V, h16* __restrict__ O,
                                                                                int rows_per_batch, int heads, int ldq, int ldkv, int ldo,
                                                                                float scale_log2, const float* __restrict__ w,
                                                                                const h16* __restrict__ mask, int ldm, int images, int tpi,
                                                                                int slab_heads, int block_rows) {
    constexpr int T = NT * 16;
    constexpr int KS = (D + 31) / 32;                // k-steps of the score product
    constexpr int CT = (D + 15) / 16;                // 16-channel tiles of the output
    constexpr int VS = T + 4;                        // halves per row of the transposed V image (rows stay 8-byte aligned)
    extern __shared__ uint4 ip_lds[];
    const float wv = *w;
    if (wv == 0.0f) return;                          // uniform: the same word for every workgroup
    const int r0 = blockIdx.x * block_rows;
    const int nrows = min(block_rows, rows_per_batch - r0);
    h16* Ms = reinterpret_cast<h16*>(ip_lds);        // [images][block_rows]
    if (!ipm_load_block(Ms, mask, ldm, images, r0, nrows, block_rows, blockDim.x)) return;     // nothing of Q, K, V or O is read

    const int b = blockIdx.y;
    const int h0 = blockIdx.z * slab_heads;
    const int hs = min(slab_heads, heads - h0);
    const int W = hs * D, W8 = W / 8, KR = W + 8;    // slab width; halves per row of the K image (one 16-byte slot of padding)
    h16* Ks = reinterpret_cast<h16*>(ip_lds) + IP_MASK_BYTES / 2;
    h16* Vt = Ks + (size_t)T * KR;
    for (int idx = threadIdx.x; idx < T * W8; idx += blockDim.x) {
        const int t = idx / W8, cc = idx - t * W8;
        bc_st16(Ks + (size_t)t * KR + cc * 8, bc_ld16(K + ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8));
    }
    for (int idx = threadIdx.x; idx < T * W8; idx += blockDim.x) {
        const int cc = idx / T, t = idx - cc * T;
        const uint4 vraw = bc_ld16(V + ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8);
        const h16* vh = reinterpret_cast<const h16*>(&vraw);
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(size_t)(cc * 8 + j) * VS + t] = vh[j];
    }
    __syncthreads();

    const int nitems = ((nrows + 15) >> 4) * hs;
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int qi = lane & 15, gq = lane >> 4;
    for (int item = wave; item < nitems; item += nwaves) {           // wave-uniform: every MFMA runs with all lanes
        const int tile = item / hs, hl = item - tile * hs;
        const int row = tile * 16 + qi;
        const bool ractive = row < nrows && ipm_row_nonzero(Ms, images, block_rows, row);   // inside the block, with a non-zero mask
        if (!__any(ractive)) continue;               // wave-uniform
        const size_t grow = (size_t)b * rows_per_batch + r0 + row;
        const h16* qrow = Q + grow * ldq + (size_t)(h0 + hl) * D;
        h16* orow = O + grow * ldo + (size_t)(h0 + hl) * D;
        h16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int ch = ks * 32 + gq * 8;
            uint4 raw = make_uint4(0, 0, 0, 0);
            if (ractive && ch < D) raw = bc_ld16(qrow + ch);
            qf[ks] = __builtin_bit_cast(h16x8, raw);
        }
        uint2 oraw[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int ch = ct * 16 + gq * 4;
            oraw[ct] = make_uint2(0, 0);
            if (ractive && ch < D) oraw[ct] = *reinterpret_cast<const uint2*>(orow + ch);
        }

        f32x4 s[NT];
        float mt[NT];                                // per tile: the maximum of the lane's row, then of its image
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int ch = ks * 32 + gq * 8;
                uint4 raw = make_uint4(0, 0, 0, 0);
                if (ch < D) raw = *reinterpret_cast<const uint4*>(Ks + (size_t)(kt * 16 + qi) * KR + hl * D + ch);
                s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h16x8, raw), qf[ks], s[kt], 0, 0, 0);
            }
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] *= scale_log2;
                m = fmaxf(m, s[kt][r]);
            }
            m = fmaxf(m, __shfl_xor(m, 16));
            mt[kt] = fmaxf(m, __shfl_xor(m, 32));
        }
        float mg[NT], lt[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            mg[kt] = mt[kt];
#pragma unroll
            for (int k2 = 0; k2 < NT; ++k2)
                if (k2 != kt && k2 / tpi == kt / tpi) mg[kt] = fmaxf(mg[kt], mt[k2]);       // (uniform: tpi is a launch argument)
        }
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            float l = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] = __builtin_amdgcn_exp2f(s[kt][r] - mg[kt]);
                l += s[kt][r];
            }
            l += __shfl_xor(l, 16);
            lt[kt] = l + __shfl_xor(l, 32);
        }
        h16x4 pf[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            float l = lt[kt];                        // >= 1 once the image's tiles are summed: its maximum contributes exp2(0)
#pragma unroll
            for (int k2 = 0; k2 < NT; ++k2)
                if (k2 != kt && k2 / tpi == kt / tpi) l += lt[k2];
            const float f = ractive ? (float)Ms[(kt / tpi) * block_rows + row] / l : 0.f;    // the image's weight on this row, fp32
#pragma unroll
            for (int r = 0; r < 4; ++r) pf[kt][r] = (h16)(s[kt][r] * f);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const h16* vrow = Vt + (size_t)(hl * D + ct * 16 + qi) * VS + gq * 4;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                const uint2 raw = *reinterpret_cast<const uint2*>(vrow + kt * 16);
                acc = __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(h16x4, raw), pf[kt], acc, 0, 0, 0);
            }
            const int ch = ct * 16 + gq * 4;
            if (ractive && ch < D) {
                h16x4 o = __builtin_bit_cast(h16x4, oraw[ct]);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (h16)fmaf(acc[r], wv, (float)o[r]);
                *reinterpret_cast<uint2*>(orow + ch) = __builtin_bit_cast(uint2, o);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ the downsampling
// One thread per output element.  upsample_bicubic2d of the reference's F.interpolate: source coordinate scale * (dst + 0.5) - 0.5 with
// scale = in / out (not clamped at 0 for the cubic filter), taps floor - 1 .. floor + 2 clamped to the image, the cubic convolution
// coefficients with A = -0.75.
__device__ __forceinline__ void ipm_cubic(double t, double* c) {
    const double A = -0.75;
    auto c1 = [&](double x) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; };
    auto c2 = [&](double x) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; };
    c[0] = c2(t + 1.0);
    c[1] = c1(t);
    c[2] = c1(1.0 - t);
    c[3] = c2(2.0 - t);
}

template <typename TIn>
__global__ __launch_bounds__(256) void ip_mask_downsample_kernel(const TIn* __restrict__ mask, int images, int H, int W, int mask_h, int mask_w,
                                                                 int rows, h16* __restrict__ out, int ldo) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)images * rows) return;
    const int i = (int)(idx / rows), r = (int)(idx - (long long)i * rows);
    float v = 0.f;
    if (r < mask_h * mask_w) {
        const int oy = r / mask_w, ox = r - oy * mask_w;
        const double sy = (double)H / mask_h * (oy + 0.5) - 0.5, sx = (double)W / mask_w * (ox + 0.5) - 0.5;
        const double fy = floor(sy), fx = floor(sx);
        double cy[4], cx[4];
        ipm_cubic(sy - fy, cy);
        ipm_cubic(sx - fx, cx);
        const TIn* img = mask + (size_t)i * H * W;
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int y = min(max((int)fy - 1 + a, 0), H - 1);
            double rowsum = 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int x = min(max((int)fx - 1 + e, 0), W - 1);
                rowsum += cx[e] * (double)img[(size_t)y * W + x];
            }
            acc += cy[a] * rowsum;
        }
        v = (float)acc;
    }
    out[(size_t)i * ldo + r] = (h16)v;
}

}  // namespace

// Which kernel bc_attention_ip_masked runs: the measured classes of bc_attention_ip_path at images x Tp keys, where Tp is a multiple of
// 16 - the same tiles, the same staging, the same work per key; tools/ip_adapter_probe.py --masks-markdown times both masked kernels by
// name on those classes (profiles/ip_adapter_masks.md).  Everything else - an unmeasured (heads, d) pair, any other Tp - is the scalar
// kernel's.
extern "C" int bc_attention_ip_masked_path(int d, int images, int tokens_per_image, int rows_per_batch, int heads) {
    if (images < 1 || tokens_per_image < 16 || tokens_per_image % 16 != 0 || images * tokens_per_image > BC_ATTENTION_IP_MAX_T) return 0;
    return bc_attention_ip_path(d, images * tokens_per_image, rows_per_batch, heads);
}

extern "C" int bc_attention_ip_masked_with(int path, const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch,
                                           int heads, int d, int images, int tokens_per_image, int ldq, int ldkv, int ldo, float qk_scale,
                                           const float* w, const bc_half* mask, int ldm, bc_stream stream_) {
    const char* name = "bc_attention_ip_masked";
    const int Tp = tokens_per_image, T = images * Tp;
    const IpMaskArgs margs = {mask, ldm, images, Tp};
    if (ip_check_args(name, path, Q, K, V, O, B, rows_per_batch, heads, d, T, ldq, ldkv, ldo, w, &margs)) return 1;
    const h16* q = reinterpret_cast<const h16*>(Q);
    const h16* k = reinterpret_cast<const h16*>(K);
    const h16* v = reinterpret_cast<const h16*>(V);
    const h16* m = reinterpret_cast<const h16*>(mask);
    h16* o = reinterpret_cast<h16*>(O);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const float scale_log2 = qk_scale * 1.4426950408889634f;
    return ip_dispatch_d(d, [&](auto D) {
        if (path == 0)
            return ip_launch(name, attention_ip_masked_kernel<D()>, ip_scalar_geometry(D(), heads, T, IP_MASK_BYTES), B, rows_per_batch, heads, stream,
                             q, k, v, o, rows_per_batch, heads, images, Tp, ldq, ldkv, ldo, scale_log2, w, m, ldm);
        return ip_dispatch_nt(T, [&](auto NT) {
            return ip_launch(name, attention_ip_masked_tiles_kernel<D(), NT()>, ip_tiles_geometry(D(), heads, T, B, rows_per_batch, IP_MASK_BYTES), B,
                             rows_per_batch, heads, stream, q, k, v, o, rows_per_batch, heads, ldq, ldkv, ldo, scale_log2, w, m, ldm, images,
                             NT() / images);
        });
    });
}

extern "C" int bc_attention_ip_masked(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads,
                                      int d, int images, int tokens_per_image, int ldq, int ldkv, int ldo, float qk_scale, const float* w,
                                      const bc_half* mask, int ldm, bc_stream stream) {
    return bc_attention_ip_masked_with(bc_attention_ip_masked_path(d, images, tokens_per_image, rows_per_batch, heads), Q, K, V, O, B,
                                       rows_per_batch, heads, d, images, tokens_per_image, ldq, ldkv, ldo, qk_scale, w, mask, ldm, stream);
}

extern "C" int bc_ip_mask_downsample(const void* mask, int is_u8, int images, int H, int W, int mask_h, int mask_w, int rows, bc_half* out,
                                     int ldo, bc_stream stream_) {
    BC_CHECK_ARG(mask && out, "bc_ip_mask_downsample: null pointer");
    BC_CHECK_ARG(images >= 1 && H >= 1 && W >= 1 && (long long)images * H * W < (1ll << 31), "bc_ip_mask_downsample: bad mask images=%d H=%d W=%d",
                 images, H, W);
    BC_CHECK_ARG(mask_h >= 1 && mask_w >= 1 && rows >= 1 && (long long)mask_h * mask_w <= rows,
                 "bc_ip_mask_downsample: the grid mask_h=%d x mask_w=%d must be non-empty and fit rows=%d", mask_h, mask_w, rows);
    BC_CHECK_ARG(ldo >= rows, "bc_ip_mask_downsample: ldo=%d must cover rows=%d", ldo, rows);
    BC_CHECK_ARG((long long)images * rows < (1ll << 31), "bc_ip_mask_downsample: images=%d x rows=%d too large", images, rows);
    BC_CHECK_ARG((uintptr_t)out % 2 == 0 && (is_u8 || (uintptr_t)mask % 4 == 0), "bc_ip_mask_downsample: misaligned pointer");
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const int blocks = bc_ceil_div((long long)images * rows, 256);
    h16* o = reinterpret_cast<h16*>(out);
    if (is_u8)
        hipLaunchKernelGGL(ip_mask_downsample_kernel<unsigned char>, dim3(blocks), dim3(256), 0, stream,
                           reinterpret_cast<const unsigned char*>(mask), images, H, W, mask_h, mask_w, rows, o, ldo);
    else
        hipLaunchKernelGGL(ip_mask_downsample_kernel<float>, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const float*>(mask), images, H,
                           W, mask_h, mask_w, rows, o, ldo);
    BC_CHECK_LAUNCH();
    return 0;
}
