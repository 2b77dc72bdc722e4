// IP-Adapter masks: the image cross-attention of an attn2 with one softmax PER IMAGE, each image's result weighted row by row with that
// image's mask, accumulated onto the text-attention output in place; and the bicubic downsampling that makes those masks.  gfx950.
//
// Reference call site replaced: IPAdapterAttnProcessor2_0 with ip_adapter_masks (D/models/attention_processor.py:3818-3849), per adapter
//   for i in images:  hidden_states += scale * (F.scaled_dot_product_attention(query, ip_key[i], ip_value[i]) * mask_downsample[i])
// and IPAdapterMaskProcessor.downsample (D/image_processor.py:969-1029) for mask_downsample.
//
// The attention kernel is attention_ip_kernel of attention_ip.hip (lanes along channels, d / 8 lanes per (row, head) item, segmented
// shuffle reductions, K and V of a head slab in LDS) with three differences:
//   - the online softmax over groups of four keys starts again for every image, and what an image leaves - its fp32 sum of
//     probability x V and its denominator l_i - goes into the item's fp32 total with the weight m[i, r] / l_i, formed in fp32;
//   - the mask values of the row block sit in LDS (4 KiB in front of K), loaded before anything else; a workgroup whose block holds no
//     non-zero value returns there, before K and V are staged - the launch of a blob-sized mask is mostly such workgroups;
//   - an item whose row has a zero mask for every image loads neither Q nor O and stores nothing, and a wave pass with no other item
//     is skipped (the trip count stays wave-uniform: every lane shuffles).
// The MFMA tiles of attention_ip.hip have a masked form too, for images whose token count is a multiple of 16 (IP-Adapter Plus): see the
// second kernel below.
#include "bc_common.h"
#include "../../include/blobctrl_ip_mask.h"

namespace {

constexpr int IPM_MAX_ROWS = 32;                     // rows of one image per workgroup, at most
constexpr int IPM_ITEMS_PER_LANE = 5;                // (row, head) items a lane group walks, about (attention_ip.hip)
constexpr int IPM_THREADS = 256;
constexpr int IPM_MASK_BYTES = 4096;                 // the block's mask: images * rows <= 64 * 32 halves
constexpr int IPM_LDS_BYTES = 65536 - IPM_MASK_BYTES;      // K + V of a head slab

__device__ __forceinline__ bool ipm_nonzero(h16 v) { return (__builtin_bit_cast(unsigned short, v) & 0x7fffu) != 0; }   // (a NaN counts)

template <int D>
__global__ __launch_bounds__(IPM_THREADS) void attention_ip_masked_kernel(const h16* __restrict__ Q, const h16* __restrict__ K,
                                                                          const h16* __restrict__ V, h16* __restrict__ O, int rows_per_batch,
                                                                          int heads, int images, int Tp, int ldq, int ldkv, int ldo,
                                                                          float scale_log2, const float* __restrict__ w,
                                                                          const h16* __restrict__ mask, int ldm, int slab_heads, int block_rows) {
    constexpr int L = D / 8;                         // lanes per item
    constexpr int G = 64 / L;                        // items per wave
    extern __shared__ uint4 ip_lds[];                // (16-byte aligned base: no static __shared__ in this kernel)
    const float wv = *w;
    if (wv == 0.0f) return;                          // uniform: the same word for every workgroup
    const int r0 = blockIdx.x * block_rows;
    const int nrows = min(block_rows, rows_per_batch - r0);
    h16* Ms = reinterpret_cast<h16*>(ip_lds);        // [images][block_rows]
    int any = 0;
    for (int idx = threadIdx.x; idx < images * nrows; idx += IPM_THREADS) {
        const int i = idx / nrows, r = idx - i * nrows;
        const h16 v = mask[(size_t)i * ldm + r0 + r];
        Ms[i * block_rows + r] = v;
        any |= ipm_nonzero(v);
    }
    if (!__syncthreads_or(any)) return;              // uniform over the workgroup: nothing of Q, K, V or O is read

    const int T = images * Tp;
    const int b = blockIdx.y;
    const int h0 = blockIdx.z * slab_heads;
    const int hs = min(slab_heads, heads - h0);      // heads of this slab
    const int W = hs * D, W8 = W / 8;                // slab width in channels / in 16-byte chunks
    h16* Ks = reinterpret_cast<h16*>(ip_lds) + IPM_MASK_BYTES / 2;
    h16* Vs = Ks + (size_t)T * W;
    for (int idx = threadIdx.x; idx < T * W8; idx += IPM_THREADS) {
        const int t = idx / W8, cc = idx - t * W8;
        const size_t src = ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8;
        bc_st16(Ks + (size_t)idx * 8, bc_ld16(K + src));
        bc_st16(Vs + (size_t)idx * 8, bc_ld16(V + src));
    }
    __syncthreads();

    const int nitems = nrows * hs;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane / L, c = lane - g * L;
    for (int base = wave * G; base < nitems; base += (IPM_THREADS / 64) * G) {     // wave-uniform trip count: every lane shuffles
        const int item = base + g;
        const bool inside = g < G && item < nitems;
        const int row = inside ? item / hs : 0, hl = inside ? item - row * hs : 0;
        bool active = false;
        if (inside)
            for (int i = 0; i < images; ++i) active |= ipm_nonzero(Ms[i * block_rows + row]);
        if (!__any(active)) continue;                // wave-uniform
        const int kcol = hl * D + c * 8;             // this lane's 8 channels inside the slab (lane c < L always: kcol + 8 <= W)
        const size_t grow = (size_t)b * rows_per_batch + r0 + row;
        const size_t col = (size_t)(h0 + hl) * D + c * 8;
        uint4 qraw = make_uint4(0, 0, 0, 0), oraw = make_uint4(0, 0, 0, 0);
        if (active) {
            qraw = bc_ld16(Q + grow * ldq + col);
            oraw = bc_ld16(O + grow * ldo + col);
        }
        const h16* qh = reinterpret_cast<const h16*>(&qraw);
        float q[8], tot[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            q[j] = (float)qh[j];
            tot[j] = 0.f;
        }
        for (int i = 0; i < images; ++i) {
            const h16* Ki = Ks + (size_t)i * Tp * W + kcol;
            const h16* Vi = Vs + (size_t)i * Tp * W + kcol;
            float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
            for (int t0 = 0; t0 < Tp; t0 += 4) {
                float s[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s[u] = 0.f;
                    if (t0 + u < Tp) {
                        const uint4 kraw = *reinterpret_cast<const uint4*>(Ki + (size_t)(t0 + u) * W);
                        const h16* kh = reinterpret_cast<const h16*>(&kraw);
#pragma unroll
                        for (int j = 0; j < 8; ++j) s[u] = fmaf(q[j], (float)kh[j], s[u]);
                    }
                }
                // segmented sum over the item's L lanes (lane c collects c .. L - 1), then the item's first lane tells everyone
#pragma unroll
                for (int off = 1; off < L; off *= 2) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float other = __shfl_down(s[u], off);
                        if (c + off < L) s[u] += other;
                    }
                }
                float mc = m;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s[u] = __shfl(s[u], lane - c);
                    s[u] = t0 + u < Tp ? s[u] * scale_log2 : -INFINITY;
                    mc = fmaxf(mc, s[u]);
                }
                const float corr = __builtin_amdgcn_exp2f(m - mc);      // first group: exp2(-inf) = 0
                m = mc;
                l *= corr;
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] *= corr;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (t0 + u < Tp) {
                        const float p = __builtin_amdgcn_exp2f(s[u] - mc);
                        l += p;
                        const uint4 vraw = *reinterpret_cast<const uint4*>(Vi + (size_t)(t0 + u) * W);
                        const h16* vh = reinterpret_cast<const h16*>(&vraw);
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, (float)vh[j], acc[j]);
                    }
                }
            }
            const float f = (float)Ms[i * block_rows + row] / l;        // the image's weight on this row, fp32 (l >= 1)
#pragma unroll
            for (int j = 0; j < 8; ++j) tot[j] = fmaf(acc[j], f, tot[j]);
        }
        if (active) {
            h16* oh = reinterpret_cast<h16*>(&oraw);
#pragma unroll
            for (int j = 0; j < 8; ++j) oh[j] = (h16)fmaf(tot[j], wv, (float)oh[j]);
            bc_st16(O + grow * ldo + col, oraw);
        }
    }
}

template <int D>
int attention_ip_masked_launch(const h16* Q, const h16* K, const h16* V, h16* O, int B, int rows_per_batch, int heads, int images, int Tp,
                               int ldq, int ldkv, int ldo, float qk_scale, const float* w, const h16* mask, int ldm, hipStream_t stream) {
    const int T = images * Tp;
    const int slab_heads = std::min(heads, IPM_LDS_BYTES / 4 / T / D);   // >= 1: T <= 64 and D <= 160 give 64 * 160 * 4 = 40 KiB
    const int slabs = bc_ceil_div(heads, slab_heads);
    BC_CHECK_ARG(slabs <= 65535, "bc_attention_ip_masked: %d head slabs exceed the grid", slabs);
    const size_t lds = IPM_MASK_BYTES + (size_t)2 * T * slab_heads * D * sizeof(h16);
    const int per_pass = (IPM_THREADS / 64) * (64 / (D / 8));            // items the workgroup takes per pass
    const int block_rows = std::max(1, std::min(IPM_MAX_ROWS, IPM_ITEMS_PER_LANE * per_pass / slab_heads));
    static_assert(BC_ATTENTION_IP_MAX_T * IPM_MAX_ROWS * sizeof(h16) <= IPM_MASK_BYTES, "the block's mask fits its LDS region");
    hipLaunchKernelGGL(attention_ip_masked_kernel<D>, dim3(bc_ceil_div(rows_per_batch, block_rows), B, slabs), dim3(IPM_THREADS), lds, stream,
                       Q, K, V, O, rows_per_batch, heads, images, Tp, ldq, ldkv, ldo, qk_scale * 1.4426950408889634f, w, mask, ldm, slab_heads,
                       block_rows);
    BC_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------- the MFMA path
// attention_ip_tiles_kernel of attention_ip.hip (a wave owns 16 query rows of one head; S^T = K . Q^T by v_mfma_f32_16x16x32_f16 per
// 16-key tile, O^T = V^T . P^T by v_mfma_f32_16x16x16f16 from a transposed V image in LDS; operand layouts as described there) for
// images of Tp = 16 `tpi` tokens: a 16-key tile belongs to exactly one image, tile kt to image kt / tpi.
//   softmax          the maximum and the sum of every TILE go through the two xor shuffles (16, 32); an image's maximum and its
//                    denominator l_i are those of its tiles.  Probabilities stay fp32 until the weight is known.
//   the weight       lane (query l & 15, group l >> 4) holds, in the accumulator registers of tile kt, the scores of ITS query row and
//                    keys 16 kt + 4 (l >> 4) + r - so the mask value of the lane's row, m[kt / tpi, row] / l_i in fp32, scales those four
//                    probabilities, which are then rounded to fp16 as the B operand of the P . V product.  The sum over images is the
//                    MFMA's own sum over key tiles; w meets the fp32 accumulator at the store.
// The mask block sits in LDS in front of K as in the scalar kernel; a workgroup without a non-zero mask value returns before staging, a
// wave skips an item (16 rows of a head) without one, and a lane whose row has none loads neither Q nor O and stores nothing.
constexpr int IPMT_ROWS = 64;                        // rows of one image per workgroup, at most (4 items per head)
constexpr int IPMT_WG_TARGET = 512;                  // workgroups to aim for when the launch is small (2 per CU)

static size_t ipmt_lds_bytes(int T, int W) { return IPM_MASK_BYTES + ((size_t)T * (W + 8) + (size_t)(W + 16) * (T + 4)) * sizeof(h16); }

template <int D, int NT>
__global__ __launch_bounds__(IPM_THREADS) void attention_ip_masked_tiles_kernel(const h16* __restrict__ Q, const h16* __restrict__ K,
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
    int any = 0;
    for (int idx = threadIdx.x; idx < images * nrows; idx += blockDim.x) {
        const int i = idx / nrows, r = idx - i * nrows;
        const h16 v = mask[(size_t)i * ldm + r0 + r];
        Ms[i * block_rows + r] = v;
        any |= ipm_nonzero(v);
    }
    if (!__syncthreads_or(any)) return;              // uniform over the workgroup: nothing of Q, K, V or O is read

    const int b = blockIdx.y;
    const int h0 = blockIdx.z * slab_heads;
    const int hs = min(slab_heads, heads - h0);
    const int W = hs * D, W8 = W / 8, KR = W + 8;    // slab width; halves per row of the K image (one 16-byte slot of padding)
    h16* Ks = reinterpret_cast<h16*>(ip_lds) + IPM_MASK_BYTES / 2;
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
        bool ractive = false;                        // the lane's row is inside the block and has a non-zero mask
        if (row < nrows)
            for (int i = 0; i < images; ++i) ractive |= ipm_nonzero(Ms[i * block_rows + row]);
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

template <int D, int NT>
int attention_ip_masked_tiles_launch(const h16* Q, const h16* K, const h16* V, h16* O, int B, int rows_per_batch, int heads, int images, int ldq,
                                     int ldkv, int ldo, float qk_scale, const float* w, const h16* mask, int ldm, hipStream_t stream) {
    constexpr int T = NT * 16;
    int slab_heads = 1;                                                  // T = 64, D = 160: 48.4 KiB for one head, the mask included
    while (slab_heads < heads && ipmt_lds_bytes(T, (slab_heads + 1) * D) <= (size_t)65536) ++slab_heads;
    int block_rows = IPMT_ROWS;
    // a small launch: narrower head slabs first (less staging per workgroup), then fewer rows
    auto wgs = [&] { return (long long)bc_ceil_div(rows_per_batch, block_rows) * B * bc_ceil_div(heads, slab_heads); };
    while (wgs() < IPMT_WG_TARGET && slab_heads > 1) slab_heads = (slab_heads + 1) / 2;
    while (wgs() < IPMT_WG_TARGET && block_rows > 16) block_rows /= 2;
    const int slabs = bc_ceil_div(heads, slab_heads);
    BC_CHECK_ARG(slabs <= 65535, "bc_attention_ip_masked: %d head slabs exceed the grid", slabs);
    static_assert(4 * IPMT_ROWS * sizeof(h16) <= IPM_MASK_BYTES, "the block's mask fits its LDS region (at most 4 images of 16 tokens)");
    const int items = bc_ceil_div(std::min(block_rows, rows_per_batch), 16) * slab_heads;
    const int threads = 64 * std::min(IPM_THREADS / 64, items);
    hipLaunchKernelGGL((attention_ip_masked_tiles_kernel<D, NT>), dim3(bc_ceil_div(rows_per_batch, block_rows), B, slabs), dim3(threads),
                       ipmt_lds_bytes(T, slab_heads * D), stream, Q, K, V, O, rows_per_batch, heads, ldq, ldkv, ldo,
                       qk_scale * 1.4426950408889634f, w, mask, ldm, images, NT / images, slab_heads, block_rows);
    BC_CHECK_LAUNCH();
    return 0;
}

template <int D>
int attention_ip_masked_tiles_dispatch(const h16* Q, const h16* K, const h16* V, h16* O, int B, int rows_per_batch, int heads, int images, int T,
                                       int ldq, int ldkv, int ldo, float qk_scale, const float* w, const h16* mask, int ldm, hipStream_t stream) {
#define BC_IPMT_NT(N) \
    case N: return attention_ip_masked_tiles_launch<D, N>(Q, K, V, O, B, rows_per_batch, heads, images, ldq, ldkv, ldo, qk_scale, w, mask, ldm, stream)
    switch (T / 16) {
        BC_IPMT_NT(1); BC_IPMT_NT(2); BC_IPMT_NT(3); BC_IPMT_NT(4);
    }
#undef BC_IPMT_NT
    return 1;
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
    const int Tp = tokens_per_image;
    BC_CHECK_ARG(path == 0 || path == 1, "bc_attention_ip_masked_with: path=%d (0 the scalar kernel, 1 the MFMA tiles)", path);
    BC_CHECK_ARG(Q && K && V && O && w && mask, "bc_attention_ip_masked: null pointer");
    BC_CHECK_ARG(B > 0 && B <= 65535 && rows_per_batch > 0 && heads > 0 && heads <= 65535,
                 "bc_attention_ip_masked: bad shape B=%d rows_per_batch=%d heads=%d", B, rows_per_batch, heads);
    BC_CHECK_ARG(images >= 1, "bc_attention_ip_masked: images=%d (at least 1)", images);
    BC_CHECK_ARG(Tp >= 1, "bc_attention_ip_masked: tokens_per_image=%d (at least 1)", Tp);
    BC_CHECK_ARG((long long)images * Tp <= BC_ATTENTION_IP_MAX_T, "bc_attention_ip_masked: images=%d x tokens_per_image=%d image tokens (1 .. %d)",
                 images, Tp, BC_ATTENTION_IP_MAX_T);
    BC_CHECK_ARG(d == 8 || d == 16 || d == 32 || d == 40 || d == 64 || d == 80 || d == 160,
                 "bc_attention_ip_masked: unsupported head size d=%d (8, 16, 32, 40, 64, 80, 160)", d);
    const long long Cc = (long long)heads * d;
    BC_CHECK_ARG(ldq >= Cc && ldo >= Cc && ldkv >= Cc && ldq % 8 == 0 && ldo % 8 == 0 && ldkv % 8 == 0,
                 "bc_attention_ip_masked: ldq=%d ldo=%d ldkv=%d must cover C=%lld and be multiples of 8", ldq, ldo, ldkv, Cc);
    BC_CHECK_ARG(rows_per_batch < (1 << 30), "bc_attention_ip_masked: rows_per_batch=%d too large", rows_per_batch);
    BC_CHECK_ARG(ldm >= rows_per_batch, "bc_attention_ip_masked: the mask's leading dimension ldm=%d must cover rows_per_batch=%d", ldm,
                 rows_per_batch);
    const uintptr_t al = (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O;
    BC_CHECK_ARG(al % 16 == 0, "bc_attention_ip_masked: Q, K, V and O need 16-byte alignment");
    BC_CHECK_ARG((uintptr_t)w % 4 == 0, "bc_attention_ip_masked: the weight is an aligned fp32 word");
    BC_CHECK_ARG((uintptr_t)mask % 2 == 0, "bc_attention_ip_masked: the mask is aligned fp16");
    if (path == 1) {
        BC_CHECK_ARG(Tp % 16 == 0, "bc_attention_ip_masked_with: the MFMA tiles take 16, 32, 48 or 64 tokens per image, not tokens_per_image=%d", Tp);
    }
    const h16* q = reinterpret_cast<const h16*>(Q);
    const h16* k = reinterpret_cast<const h16*>(K);
    const h16* v = reinterpret_cast<const h16*>(V);
    const h16* m = reinterpret_cast<const h16*>(mask);
    h16* o = reinterpret_cast<h16*>(O);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (path == 1) {
#define BC_IPMT_CASE(D) \
    case D: return attention_ip_masked_tiles_dispatch<D>(q, k, v, o, B, rows_per_batch, heads, images, images * Tp, ldq, ldkv, ldo, qk_scale, w, m, ldm, stream)
        switch (d) {
            BC_IPMT_CASE(8); BC_IPMT_CASE(16); BC_IPMT_CASE(32); BC_IPMT_CASE(40); BC_IPMT_CASE(64); BC_IPMT_CASE(80); BC_IPMT_CASE(160);
        }
#undef BC_IPMT_CASE
        return 1;
    }
#define BC_IPM_CASE(D) \
    case D: return attention_ip_masked_launch<D>(q, k, v, o, B, rows_per_batch, heads, images, Tp, ldq, ldkv, ldo, qk_scale, w, m, ldm, stream)
    switch (d) {
        BC_IPM_CASE(8); BC_IPM_CASE(16); BC_IPM_CASE(32); BC_IPM_CASE(40); BC_IPM_CASE(64); BC_IPM_CASE(80); BC_IPM_CASE(160);
    }
#undef BC_IPM_CASE
    return 1;
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
