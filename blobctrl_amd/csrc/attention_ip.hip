// IP-Adapter: the decoupled image cross-attention of an attn2, accumulated onto the text-attention output in place, gfx950.
//
// Reference call site replaced: IPAdapterAttnProcessor2_0 (D/models/attention_processor.py:3851-3868), per adapter
//   ip_hidden_states = F.scaled_dot_product_attention(query, ip_key, ip_value)
//   hidden_states = hidden_states + scale * ip_hidden_states                       (in front of to_out; skipped when scale == 0)
// with ip_key / ip_value the adapter's projections of its image tokens: T = 4 per image for the base adapter, a few images at most.
//
// Two kernels stand behind the entry point: the scalar one described first, made for T = 4, and MFMA tiles for T = 16, 32, 48, 64 (IP-Adapter
// Plus) further down; bc_attention_ip_path picks by measured class, bc_attention_ip_with launches a named one.
//
// The launch is memory- and launch-bound: it reads Q, reads and writes O (3 * M * C * 2 bytes) and does ~4 T flops per byte of them.
// Work shape: lanes run along channels, 16 bytes (8 x fp16) per lane, so the d / 8 lanes of one (row, head) ITEM sit side by side in a
// wave - 64 / (d / 8) whole items per wave, no item straddles a wave (d = 40, 80, 160 leave 4 lanes idle).  A lane holds its 8 query
// channels and 8 output channels in registers for the whole item: Q and O are touched exactly once.  The partial dot products of an
// item's lanes are summed by a segmented shuffle reduction in a fixed order and broadcast from the item's first lane, so every lane of
// the item sees the same score; four keys go through the reduction at a time (independent shuffle chains), and the softmax runs online
// over those groups of four in fp32, in log2 units.
// A workgroup owns a block of consecutive rows of ONE image (row blocks are cut at image boundaries) and a slab of whole heads; it stages
// that image's K and V columns of the slab in LDS once (<= 64 KiB: T * slab width * 4 bytes) and every item reads them from there.
// An item is a chain of dependent latencies (global load, shuffles, exponentials), so a wave should walk only a few of them: the host
// sizes the row block for about IP_ITEMS_PER_LANE items per lane group - 7 rows at d = 160, 30 at d = 40 with 8 heads - and at most
// IP_MAX_ROWS rows (measured at 1280 channels, 2 x 512 rows: 34 us with 32-row blocks - 22 serial items per lane group on 32 workgroups -
// and 11.8 us with 7-row blocks; profiles/ip_adapter.md).  The price of small blocks: every row block stages the image's K / V slab again,
// at d = 160 and T = 4 about 20 KB of K / V (L2 hits) per 53 KB of Q / O traffic - the 1280-channel launches reach 0.7 (batch 2) to
// 2.9 TB/s (batch 16) of algorithmic bytes where the 320-channel level reaches 4.3.  Accepted: at those sizes the launch is latency-bound.
// The weight w is read from device memory: one plan and one captured graph serve every set_ip_adapter_scale.  w == 0 returns before
// anything else is read - the branch is uniform over the grid.
#include "bc_common.h"
#include "../../include/blobctrl_ip.h"

namespace {

constexpr int IP_MAX_ROWS = 32;                      // rows of one image per workgroup, at most
constexpr int IP_ITEMS_PER_LANE = 5;                 // (row, head) items a lane group walks, about
constexpr int IP_THREADS = 256;
constexpr int IP_LDS_BYTES = 65536;                  // K + V of a head slab

template <int D>
__global__ __launch_bounds__(IP_THREADS) void attention_ip_kernel(const h16* __restrict__ Q, const h16* __restrict__ K, const h16* __restrict__ V,
                                                                  h16* __restrict__ O, int rows_per_batch, int heads, int T, int ldq, int ldkv,
                                                                  int ldo, float scale_log2, const float* __restrict__ w, int slab_heads, int block_rows) {
    constexpr int L = D / 8;                         // lanes per item
    constexpr int G = 64 / L;                        // items per wave
    extern __shared__ uint4 ip_lds[];                // (16-byte aligned base: no static __shared__ in this kernel)
    const float wv = *w;
    if (wv == 0.0f) return;                          // uniform: the same word for every workgroup
    const int b = blockIdx.y;
    const int h0 = blockIdx.z * slab_heads;
    const int hs = min(slab_heads, heads - h0);      // heads of this slab
    const int W = hs * D, W8 = W / 8;                // slab width in channels / in 16-byte chunks
    h16* Ks = reinterpret_cast<h16*>(ip_lds);
    h16* Vs = Ks + (size_t)T * W;
    for (int idx = threadIdx.x; idx < T * W8; idx += IP_THREADS) {
        const int t = idx / W8, cc = idx - t * W8;
        const size_t src = ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8;
        bc_st16(Ks + (size_t)idx * 8, bc_ld16(K + src));
        bc_st16(Vs + (size_t)idx * 8, bc_ld16(V + src));
    }
    __syncthreads();

    const int r0 = blockIdx.x * block_rows;
    const int nitems = min(block_rows, rows_per_batch - r0) * hs;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane / L, c = lane - g * L;
    for (int base = wave * G; base < nitems; base += (IP_THREADS / 64) * G) {      // wave-uniform trip count: every lane shuffles
        const int item = base + g;
        const bool active = g < G && item < nitems;
        const int row = active ? item / hs : 0, hl = active ? item - row * hs : 0;
        const int kcol = hl * D + c * 8;             // this lane's 8 channels inside the slab (lane c < L always: kcol + 8 <= W)
        const size_t grow = (size_t)b * rows_per_batch + r0 + row;
        const size_t col = (size_t)(h0 + hl) * D + c * 8;
        uint4 qraw = make_uint4(0, 0, 0, 0), oraw = make_uint4(0, 0, 0, 0);
        if (active) {
            qraw = bc_ld16(Q + grow * ldq + col);
            oraw = bc_ld16(O + grow * ldo + col);
        }
        const h16* qh = reinterpret_cast<const h16*>(&qraw);
        float q[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (float)qh[j];

        float m = -INFINITY, l = 0.f, acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        for (int t0 = 0; t0 < T; t0 += 4) {
            float s[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s[u] = 0.f;
                if (t0 + u < T) {
                    const uint4 kraw = *reinterpret_cast<const uint4*>(Ks + (size_t)(t0 + u) * W + kcol);
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
                s[u] = t0 + u < T ? s[u] * scale_log2 : -INFINITY;
                mc = fmaxf(mc, s[u]);
            }
            const float corr = __builtin_amdgcn_exp2f(m - mc);          // first group: exp2(-inf) = 0
            m = mc;
            l *= corr;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] *= corr;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + u < T) {
                    const float p = __builtin_amdgcn_exp2f(s[u] - mc);
                    l += p;
                    const uint4 vraw = *reinterpret_cast<const uint4*>(Vs + (size_t)(t0 + u) * W + kcol);
                    const h16* vh = reinterpret_cast<const h16*>(&vraw);
#pragma unroll
                    for (int j = 0; j < 8; ++j) acc[j] = fmaf(p, (float)vh[j], acc[j]);
                }
            }
        }
        if (active) {
            const float f = wv / l;
            h16* oh = reinterpret_cast<h16*>(&oraw);
#pragma unroll
            for (int j = 0; j < 8; ++j) oh[j] = (h16)fmaf(acc[j], f, (float)oh[j]);
            bc_st16(O + grow * ldo + col, oraw);
        }
    }
}

template <int D>
int attention_ip_launch(const h16* Q, const h16* K, const h16* V, h16* O, int B, int rows_per_batch, int heads, int T, int ldq, int ldkv, int ldo,
                        float qk_scale, const float* w, hipStream_t stream) {
    const int slab_heads = std::min(heads, IP_LDS_BYTES / 4 / T / D);    // >= 1: T <= 64 and D <= 160 give 64 * 160 * 4 = 40 KiB
    const int slabs = bc_ceil_div(heads, slab_heads);
    BC_CHECK_ARG(slabs <= 65535, "bc_attention_ip: %d head slabs exceed the grid", slabs);
    const size_t lds = (size_t)2 * T * slab_heads * D * sizeof(h16);
    const int per_pass = (IP_THREADS / 64) * (64 / (D / 8));             // items the workgroup takes per pass
    const int block_rows = std::max(1, std::min(IP_MAX_ROWS, IP_ITEMS_PER_LANE * per_pass / slab_heads));
    hipLaunchKernelGGL(attention_ip_kernel<D>, dim3(bc_ceil_div(rows_per_batch, block_rows), B, slabs), dim3(IP_THREADS), lds, stream, Q, K, V, O,
                       rows_per_batch, heads, T, ldq, ldkv, ldo, qk_scale * 1.4426950408889634f, w, slab_heads, block_rows);
    BC_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------- the MFMA path
// For T = 16, 32, 48, 64 image tokens (IP-Adapter Plus: 16 per image).  Same contract, same staging idea, another work shape: a wave owns
// 16 consecutive query rows of one head (an ITEM), a workgroup a block of up to IPT_ROWS rows of one image and a slab of whole heads.
//   S^T = K . Q^T    v_mfma_f32_16x16x32_f16, A = 16 keys from the row-major K image in LDS (16 bytes per lane), B = the lane's 8 query
//                    channels straight from global memory; channels past d (d = 8, 16, 40, 80, 160 leave a k-step partly empty) are zero
//                    in BOTH operands' registers, so nothing in LDS or behind the head is multiplied.  The accumulator of key tile kt
//                    holds, on lane (query l & 15, group l >> 4), the scores of keys 16 kt + 4 (l >> 4) + r, r = 0 .. 3.
//   softmax          all T scores of a query live in the 4 NT registers of its 4 lanes: one maximum and one sum through two xor
//                    shuffles (16, 32), exp2 in fp32.  The sum runs over the fp16-rounded probabilities the next product consumes.
//   O^T = V^T . P^T  v_mfma_f32_16x16x16f16 per key tile: its B operand wants keys 4 (l >> 4) + j of query l & 15 in element j - exactly
//                    the accumulator's registers, converted to fp16, no lane movement.  A = 4 consecutive keys of one channel, 8 bytes
//                    from a TRANSPOSED V image [channel][T + 4] that the staging loop writes once per workgroup (2-byte LDS stores).
//                    The result has 4 consecutive channels of one query row on a lane: O is read and written 8 bytes per lane, once.
// Output channel tiles that stick out of the head (d % 16 != 0) read rows of the V image that belong to the next head or to the 16 pad
// rows behind the slab; those results are dropped.  Rows past the block are computed on zero queries and dropped.
constexpr int IPT_ROWS = 64;                         // rows of one image per workgroup, at most (4 items per head)
constexpr int IPT_WG_TARGET = 512;                   // workgroups to aim for when the launch is small (2 per CU)

static size_t ipt_lds_bytes(int T, int W) { return ((size_t)T * (W + 8) + (size_t)(W + 16) * (T + 4)) * sizeof(h16); }

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

template <int D, int NT>
int attention_ip_tiles_launch(const h16* Q, const h16* K, const h16* V, h16* O, int B, int rows_per_batch, int heads, int ldq, int ldkv, int ldo,
                              float qk_scale, const float* w, hipStream_t stream) {
    constexpr int T = NT * 16;
    int slab_heads = 1;                                                  // T = 64, D = 160: 44.4 KiB for one head
    while (slab_heads < heads && ipt_lds_bytes(T, (slab_heads + 1) * D) <= (size_t)IP_LDS_BYTES) ++slab_heads;
    int block_rows = IPT_ROWS;
    // a small launch: narrower head slabs first (less staging per workgroup), then fewer rows
    auto wgs = [&] { return (long long)bc_ceil_div(rows_per_batch, block_rows) * B * bc_ceil_div(heads, slab_heads); };
    while (wgs() < IPT_WG_TARGET && slab_heads > 1) slab_heads = (slab_heads + 1) / 2;
    while (wgs() < IPT_WG_TARGET && block_rows > 16) block_rows /= 2;
    const int slabs = bc_ceil_div(heads, slab_heads);
    BC_CHECK_ARG(slabs <= 65535, "bc_attention_ip: %d head slabs exceed the grid", slabs);
    const int items = bc_ceil_div(std::min(block_rows, rows_per_batch), 16) * slab_heads;
    const int threads = 64 * std::min(IP_THREADS / 64, items);
    hipLaunchKernelGGL((attention_ip_tiles_kernel<D, NT>), dim3(bc_ceil_div(rows_per_batch, block_rows), B, slabs), dim3(threads),
                       ipt_lds_bytes(T, slab_heads * D), stream, Q, K, V, O, rows_per_batch, heads, ldq, ldkv, ldo,
                       qk_scale * 1.4426950408889634f, w, slab_heads, block_rows);
    BC_CHECK_LAUNCH();
    return 0;
}

template <int D>
int attention_ip_tiles_dispatch(const h16* Q, const h16* K, const h16* V, h16* O, int B, int rows_per_batch, int heads, int T, int ldq, int ldkv,
                                int ldo, float qk_scale, const float* w, hipStream_t stream) {
    switch (T / 16) {
        case 1: return attention_ip_tiles_launch<D, 1>(Q, K, V, O, B, rows_per_batch, heads, ldq, ldkv, ldo, qk_scale, w, stream);
        case 2: return attention_ip_tiles_launch<D, 2>(Q, K, V, O, B, rows_per_batch, heads, ldq, ldkv, ldo, qk_scale, w, stream);
        case 3: return attention_ip_tiles_launch<D, 3>(Q, K, V, O, B, rows_per_batch, heads, ldq, ldkv, ldo, qk_scale, w, stream);
        case 4: return attention_ip_tiles_launch<D, 4>(Q, K, V, O, B, rows_per_batch, heads, ldq, ldkv, ldo, qk_scale, w, stream);
    }
    return 1;
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
    BC_CHECK_ARG(path == 0 || path == 1, "bc_attention_ip_with: path=%d (0 the scalar kernel, 1 the MFMA tiles)", path);
    BC_CHECK_ARG(Q && K && V && O && w, "bc_attention_ip: null pointer");
    BC_CHECK_ARG(B > 0 && B <= 65535 && rows_per_batch > 0 && heads > 0 && heads <= 65535,
                 "bc_attention_ip: bad shape B=%d rows_per_batch=%d heads=%d", B, rows_per_batch, heads);
    BC_CHECK_ARG(T >= 1 && T <= BC_ATTENTION_IP_MAX_T, "bc_attention_ip: T=%d image tokens (1 .. %d)", T, BC_ATTENTION_IP_MAX_T);
    BC_CHECK_ARG(d == 8 || d == 16 || d == 32 || d == 40 || d == 64 || d == 80 || d == 160,
                 "bc_attention_ip: unsupported head size d=%d (8, 16, 32, 40, 64, 80, 160)", d);
    const long long Cc = (long long)heads * d;
    BC_CHECK_ARG(ldq >= Cc && ldo >= Cc && ldkv >= Cc && ldq % 8 == 0 && ldo % 8 == 0 && ldkv % 8 == 0,
                 "bc_attention_ip: ldq=%d ldo=%d ldkv=%d must cover C=%lld and be multiples of 8", ldq, ldo, ldkv, Cc);
    BC_CHECK_ARG(rows_per_batch < (1 << 30), "bc_attention_ip: rows_per_batch=%d too large", rows_per_batch);
    const uintptr_t al = (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O;
    BC_CHECK_ARG(al % 16 == 0, "bc_attention_ip: Q, K, V and O need 16-byte alignment");
    BC_CHECK_ARG((uintptr_t)w % 4 == 0, "bc_attention_ip: the weight is an aligned fp32 word");
    const h16* q = reinterpret_cast<const h16*>(Q);
    const h16* k = reinterpret_cast<const h16*>(K);
    const h16* v = reinterpret_cast<const h16*>(V);
    h16* o = reinterpret_cast<h16*>(O);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if (path == 1) {
        BC_CHECK_ARG(T % 16 == 0, "bc_attention_ip_with: the MFMA tiles take T = 16, 32, 48 or 64 image tokens, not T=%d", T);
#define BC_IPT_CASE(D) \
    case D: return attention_ip_tiles_dispatch<D>(q, k, v, o, B, rows_per_batch, heads, T, ldq, ldkv, ldo, qk_scale, w, stream)
        switch (d) {
            BC_IPT_CASE(8); BC_IPT_CASE(16); BC_IPT_CASE(32); BC_IPT_CASE(40); BC_IPT_CASE(64); BC_IPT_CASE(80); BC_IPT_CASE(160);
        }
#undef BC_IPT_CASE
        return 1;
    }
#define BC_IP_CASE(D) \
    case D: return attention_ip_launch<D>(q, k, v, o, B, rows_per_batch, heads, T, ldq, ldkv, ldo, qk_scale, w, stream)
    switch (d) {
        BC_IP_CASE(8); BC_IP_CASE(16); BC_IP_CASE(32); BC_IP_CASE(40); BC_IP_CASE(64); BC_IP_CASE(80); BC_IP_CASE(160);
    }
#undef BC_IP_CASE
    return 1;
}

extern "C" int bc_attention_ip(const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch, int heads, int d, int T,
                               int ldq, int ldkv, int ldo, float qk_scale, const float* w, bc_stream stream) {
    return bc_attention_ip_with(bc_attention_ip_path(d, T, rows_per_batch, heads), Q, K, V, O, B, rows_per_batch, heads, d, T, ldq, ldkv, ldo,
                                qk_scale, w, stream);
}
