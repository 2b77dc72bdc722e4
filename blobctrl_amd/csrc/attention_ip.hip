// IP-Adapter: the decoupled image cross-attention of an attn2, accumulated onto the text-attention output in place, gfx950.
//
// Reference call site replaced: IPAdapterAttnProcessor2_0 (D/models/attention_processor.py:3851-3868), per adapter
//   ip_hidden_states = F.scaled_dot_product_attention(query, ip_key, ip_value)
//   hidden_states = hidden_states + scale * ip_hidden_states                       (in front of to_out; skipped when scale == 0)
// with ip_key / ip_value the adapter's projections of its image tokens: T = 4 per image for the base adapter, a few images at most.
//
// Two kernels stand behind the entry point (work shapes, operand layouts and the host side are described in bc_attention_ip.h): the
// scalar one, made for T = 4 - the unmasked form of the body there - and MFMA tiles for T = 16, 32, 48, 64 (IP-Adapter Plus), written
// out below; bc_attention_ip_path picks by measured class, bc_attention_ip_with launches a named one.
#include "bc_attention_ip.h"

namespace {

template <int D>
__global__ __launch_bounds__(IP_THREADS) void attention_ip_kernel(const h16* __restrict__ Q, const h16* __restrict__ K, const h16* __restrict__ V,
                                                                  h16* __restrict__ O, int rows_per_batch, int heads, int T, int ldq, int ldkv,
                                                                  int ldo, float scale_log2, const float* __restrict__ w, int slab_heads, int block_rows) {
    attention_ip_body<D, false>(Q, K, V, O, rows_per_batch, heads, 1, T, ldq, ldkv, ldo, scale_log2, w, nullptr, 0, slab_heads, block_rows);
}

template <int D, int NT>
__global__ __launch_bounds__(IP_THREADS) void attention_ip_tiles_kernel(const h16* __restrict__ Q, const h16* __restrict__ K,
                                                                        const h16* __restrict__ V, h16* __restrict__ O, int rows_per_batch,
                                                                        int heads, int ldq, int ldkv, int ldo, float scale_log2,
                                                                        const float* __restrict__ w, int slab_heads, int block_rows) {
    constexpr int T = NT * 16;
    constexpr int KS = (D + 31) / 32;                // k-steps of the score product
    constexpr int CT = (D + 15) / 16;                // 16-channel tiles of the output
    constexpr int VS = T + 4;                        // halves per row of the transposed V image (rows stay 8-byte aligned)
    extern __shared__ uint4 ip_lds[];
    const float wv = *w;
    if (wv == 0.0f) return;                          // uniform: the same word for every workgroup
    const int b = blockIdx.y;
    const int h0 = blockIdx.z * slab_heads;
    const int hs = min(slab_heads, heads - h0);
    const int W = hs * D, W8 = W / 8, KR = W + 8;    // slab width; halves per row of the K image (one 16-byte slot of padding)
    h16* Ks = reinterpret_cast<h16*>(ip_lds);
    h16* Vt = Ks + (size_t)T * KR;
    // K: consecutive threads take consecutive 16-byte chunks of a row (coalesced loads, row-major image)
    for (int idx = threadIdx.x; idx < T * W8; idx += blockDim.x) {
        const int t = idx / W8, cc = idx - t * W8;
        bc_st16(Ks + (size_t)t * KR + cc * 8, bc_ld16(K + ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8));
    }
    // V: consecutive threads take consecutive keys of a chunk, so the eight 2-byte stores of a thread land beside its neighbours' in the
    // transposed image (the loads stride by ldkv; T * W elements per workgroup, L2 hits)
    for (int idx = threadIdx.x; idx < T * W8; idx += blockDim.x) {
        const int cc = idx / T, t = idx - cc * T;
        const uint4 vraw = bc_ld16(V + ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8);
        const h16* vh = reinterpret_cast<const h16*>(&vraw);
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(size_t)(cc * 8 + j) * VS + t] = vh[j];
    }
    __syncthreads();

    const int r0 = blockIdx.x * block_rows;
    const int nrows = min(block_rows, rows_per_batch - r0);
    const int nitems = ((nrows + 15) >> 4) * hs;
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int qi = lane & 15, gq = lane >> 4;
    for (int item = wave; item < nitems; item += nwaves) {           // wave-uniform: every MFMA runs with all lanes
        const int tile = item / hs, hl = item - tile * hs;
        const int row = tile * 16 + qi;
        const bool rvalid = row < nrows;
        const size_t grow = (size_t)b * rows_per_batch + r0 + row;
        const h16* qrow = Q + grow * ldq + (size_t)(h0 + hl) * D;
        h16* orow = O + grow * ldo + (size_t)(h0 + hl) * D;
        h16x8 qf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int ch = ks * 32 + gq * 8;
            uint4 raw = make_uint4(0, 0, 0, 0);
            if (rvalid && ch < D) raw = bc_ld16(qrow + ch);
            qf[ks] = __builtin_bit_cast(h16x8, raw);
        }
        uint2 oraw[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int ch = ct * 16 + gq * 4;
            oraw[ct] = make_uint2(0, 0);
            if (rvalid && ch < D) oraw[ct] = *reinterpret_cast<const uint2*>(orow + ch);
        }

        f32x4 s[NT];
        float m = -INFINITY;
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
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[kt][r] *= scale_log2;
                m = fmaxf(m, s[kt][r]);
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));
        h16x4 pf[NT];
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pf[kt][r] = (h16)__builtin_amdgcn_exp2f(s[kt][r] - m);
                l += (float)pf[kt][r];
            }
        }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);                      // >= 1: the row's maximum contributes exp2(0)
        const float f = wv / l;
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
            if (rvalid && ch < D) {
                h16x4 o = __builtin_bit_cast(h16x4, oraw[ct]);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (h16)fmaf(acc[r], f, (float)o[r]);
                *reinterpret_cast<uint2*>(orow + ch) = __builtin_bit_cast(uint2, o);
            }
        }
    }
}

}  // namespace

// Which kernel bc_attention_ip runs.  Decided by measurement (tools/ip_adapter_probe.py, profiles/ip_adapter_plus.md): a (channel width, T)
// class goes to the tiles only where they won on both batch rows of that class by more than the probe's run-to-run spread.
// Measured (profiles/ip_adapter_plus.md): 8 heads of 40, 80 and 160 channels at T = 16, 32, 48, 64, 128 to 8192 rows per image, UNet batch 2
// and 16 - the tiles took 0.12 to 0.47 of the scalar kernel's time on every row of the table, far outside the run-to-run spread.  Every
// other (heads, d) pair - another split of the same width included - is unmeasured, every T that is no multiple of 16 impossible: both
// stay on the scalar kernel.
extern "C" int bc_attention_ip_path(int d, int T, int rows_per_batch, int heads) {
    (void)rows_per_batch;                            // (no class split by rows: the tiles won from 128 to 8192 rows per image)
    const bool width = heads == 8 && (d == 40 || d == 80 || d == 160);
    const bool tokens = T == 16 || T == 32 || T == 48 || T == 64;
    return width && tokens ? 1 : 0;
}

extern "C" int bc_attention_ip_with(int path, const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads,
                                    int d, int T, int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream_) {
    const char* name = "bc_attention_ip";
    if (ip_check_args(name, path, Q, K, V, O, B, rows_per_batch, heads, d, T, ldq, ldkv, ldo, w, nullptr)) return 1;
    const h16* q = reinterpret_cast<const h16*>(Q);
    const h16* k = reinterpret_cast<const h16*>(K);
    const h16* v = reinterpret_cast<const h16*>(V);
    h16* o = reinterpret_cast<h16*>(O);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const float scale_log2 = qk_scale * 1.4426950408889634f;
    return ip_dispatch_d(d, [&](auto D) {
        if (path == 0)
            return ip_launch(name, attention_ip_kernel<D()>, ip_scalar_geometry(D(), heads, T, 0), B, rows_per_batch, heads, stream, q, k, v, o,
                             rows_per_batch, heads, T, ldq, ldkv, ldo, scale_log2, w);
        return ip_dispatch_nt(T, [&](auto NT) {
            return ip_launch(name, attention_ip_tiles_kernel<D(), NT()>, ip_tiles_geometry(D(), heads, T, B, rows_per_batch, 0), B, rows_per_batch,
                             heads, stream, q, k, v, o, rows_per_batch, heads, ldq, ldkv, ldo, scale_log2, w);
        });
    });
}

extern "C" int bc_attention_ip(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d, int T,
                               int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream) {
    return bc_attention_ip_with(bc_attention_ip_path(d, T, rows_per_batch, heads), Q, K, V, O, B, rows_per_batch, heads, d, T, ldq, ldkv, ldo,
                                qk_scale, w, stream);
}
