// IP-Adapter image cross-attention: what the four kernels of attention_ip.hip (attention_ip_kernel, attention_ip_tiles_kernel) and
// attention_ip_masked.hip (attention_ip_masked_kernel, attention_ip_masked_tiles_kernel) share - the ONE body of the scalar work shape,
// the mask block, the description of both work shapes, and the host side of their entry points.  MASKED is the compile-time switch
// between `O += w * softmax(scale Q K^T) V` over all T keys and `O += w * sum_i m[i, r] * softmax_i(scale Q K_i^T) V_i` with one softmax
// per image of Tp keys (T = images * Tp).
//
// Both shapes: a workgroup owns a block of consecutive rows of ONE image (row blocks are cut at image boundaries) and a slab of whole
// heads; it stages that image's K and V columns of the slab in LDS once (<= 64 KiB) and every item reads them from there.  The weight w
// is read from device memory: one plan and one captured graph serve every set_ip_adapter_scale.  w == 0 returns before anything else is
// read - the branch is uniform over the grid.
//
// The mask block (MASKED): the mask values of the row block, [images][block_rows] fp16, sit in the first IP_MASK_BYTES of LDS, in front
// of K, loaded before anything else.  A workgroup whose block holds no non-zero value returns there, before K and V are staged - the
// launch of a blob-sized mask is mostly such workgroups.  An item (a lane's row, in the tiles) whose row has a zero mask for every image
// loads neither Q nor O and stores nothing, and a wave pass with no other item is skipped (the trip count stays wave-uniform).
#pragma once
#include <type_traits>

#include "bc_common.h"
#include "../../include/blobctrl_ip.h"

namespace {

constexpr int IP_THREADS = 256;
constexpr int IP_LDS_BYTES = 65536;                  // the mask block, K and V of a head slab
constexpr int IP_MASK_BYTES = 4096;                  // the block's mask: images * rows <= 64 * 32 halves
constexpr int IP_MAX_ROWS = 32;                      // scalar: rows of one image per workgroup, at most
constexpr int IP_ITEMS_PER_LANE = 5;                 // scalar: (row, head) items a lane group walks, about
constexpr int IPT_ROWS = 64;                         // tiles: rows of one image per workgroup, at most (4 items per head)
constexpr int IPT_WG_TARGET = 512;                   // tiles: workgroups to aim for when the launch is small (2 per CU)
static_assert(BC_ATTENTION_IP_MAX_T * IP_MAX_ROWS * sizeof(h16) <= IP_MASK_BYTES, "the block's mask fits its LDS region");
static_assert(4 * IPT_ROWS * sizeof(h16) <= IP_MASK_BYTES, "the block's mask fits its LDS region (at most 4 images of 16 tokens)");

// ---------------------------------------------------------------------------------------------------------------------- the mask block
__device__ __forceinline__ bool ipm_nonzero(h16 v) { return (__builtin_bit_cast(unsigned short, v) & 0x7fffu) != 0; }   // (a NaN counts)

// Rows r0 .. r0 + nrows of every image's mask into Ms [images][block_rows]; false, uniform over the workgroup, when all of them are zero.
__device__ __forceinline__ bool ipm_load_block(h16* Ms, const h16* __restrict__ mask, int ldm, int images, int r0, int nrows, int block_rows,
                                               int nthreads) {
    int any = 0;
    // (one trip for most threads, a few at most, and most workgroups of a blob-sized mask do nothing else: no unrolled or interleaved copies)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
    for (int idx = threadIdx.x; idx < images * nrows; idx += nthreads) {
        const int i = idx / nrows, r = idx - i * nrows;
        const h16 v = mask[(size_t)i * ldm + r0 + r];
        Ms[i * block_rows + r] = v;
        any |= ipm_nonzero(v);
    }
    return __syncthreads_or(any);
}

__device__ __forceinline__ bool ipm_row_nonzero(const h16* Ms, int images, int block_rows, int row) {
    bool any = false;
    for (int i = 0; i < images; ++i) any |= ipm_nonzero(Ms[i * block_rows + row]);
    return any;
}

// ------------------------------------------------------------------------------------------------------------------ the scalar shape
// Made for T = 4.  The launch is memory- and launch-bound: it reads Q, reads and writes O (3 * M * C * 2 bytes) and does ~4 T flops per
// byte of them.  Lanes run along channels, 16 bytes (8 x fp16) per lane, so the L = d / 8 lanes of one (row, head) ITEM sit side by side
// in a wave - G = 64 / L whole items per wave, no item straddles a wave (d = 40, 80, 160 leave 4 lanes idle).  A lane holds its 8 query
// channels and 8 output channels in registers for the whole item: Q and O are touched exactly once.  The partial dot products of an
// item's lanes are summed by a segmented shuffle reduction in a fixed order and broadcast from the item's first lane, so every lane of
// the item sees the same score; four keys go through the reduction at a time (independent shuffle chains), and the softmax runs online
// over those groups of four in fp32, in log2 units.
// The slab is T * slab width * 4 bytes of LDS, K then V, both [T][W].  An item is a chain of dependent latencies (global load, shuffles,
// exponentials), so a wave should walk only a few of them: the host sizes the row block for about IP_ITEMS_PER_LANE items per lane
// group - 7 rows at d = 160, 30 at d = 40 with 8 heads - and at most IP_MAX_ROWS rows (measured at 1280 channels, 2 x 512 rows: 34 us
// with 32-row blocks - 22 serial items per lane group on 32 workgroups - and 11.8 us with 7-row blocks; profiles/ip_adapter.md).  The
// price of small blocks: every row block stages the image's K / V slab again, at d = 160 and T = 4 about 20 KB of K / V (L2 hits) per
// 53 KB of Q / O traffic - the 1280-channel launches reach 0.7 (batch 2) to 2.9 TB/s (batch 16) of algorithmic bytes where the
// 320-channel level reaches 4.3.  Accepted: at those sizes the launch is latency-bound.

// One image's online softmax over Tp keys for a lane's eight channels: Ki / Vi point at the lane's channels of the image's first key
// in the slab [.][W]; c is the lane's place among the L lanes of its item.  Leaves the denominator l (>= 1) and acc = sum_t p_t V_t.
template <int L>
__device__ __forceinline__ void ip_softmax_image(const h16* Ki, const h16* Vi, int W, int Tp, const float (&q)[8], float scale_log2, int lane,
                                                 int c, float& l, float (&acc)[8]) {
    float m = -INFINITY;
    l = 0.f;
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
        const float corr = __builtin_amdgcn_exp2f(m - mc);              // first group: exp2(-inf) = 0
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
}

// The plain kernel is the body at images = 1, Tp = T, without a mask.  MASKED: the online softmax starts again for every image, and
// what an image leaves - acc and its denominator l_i - goes into the item's fp32 total with the weight m[i, r] / l_i, formed in fp32.
template <int D, bool MASKED>
__device__ __forceinline__ void attention_ip_body(const h16* __restrict__ Q, const h16* __restrict__ K, const h16* __restrict__ V,
                                                  h16* __restrict__ O, int rows_per_batch, int heads, int images, int Tp, int ldq, int ldkv,
                                                  int ldo, float scale_log2, const float* __restrict__ w, const h16* __restrict__ mask, int ldm,
                                                  int slab_heads, int block_rows) {
    constexpr int L = D / 8;                         // lanes per item
    constexpr int G = 64 / L;                        // items per wave
    extern __shared__ uint4 ip_lds[];                // (16-byte aligned base: no static __shared__ in these kernels)
    const float wv = *w;
    if (wv == 0.0f) return;                          // uniform: the same word for every workgroup
    const int r0 = blockIdx.x * block_rows;
    const int nrows = min(block_rows, rows_per_batch - r0);
    h16* Ms = reinterpret_cast<h16*>(ip_lds);        // [images][block_rows]
    if (MASKED && !ipm_load_block(Ms, mask, ldm, images, r0, nrows, block_rows, IP_THREADS)) return;     // nothing of Q, K, V or O is read

    const int T = images * Tp;
    const int b = blockIdx.y;
    const int h0 = blockIdx.z * slab_heads;
    const int hs = min(slab_heads, heads - h0);      // heads of this slab
    const int W = hs * D, W8 = W / 8;                // slab width in channels / in 16-byte chunks
    h16* Ks = reinterpret_cast<h16*>(ip_lds) + (MASKED ? IP_MASK_BYTES / 2 : 0);
    h16* Vs = Ks + (size_t)T * W;
    for (int idx = threadIdx.x; idx < T * W8; idx += IP_THREADS) {
        const int t = idx / W8, cc = idx - t * W8;
        const size_t src = ((size_t)b * T + t) * ldkv + (size_t)h0 * D + cc * 8;
        bc_st16(Ks + (size_t)idx * 8, bc_ld16(K + src));
        bc_st16(Vs + (size_t)idx * 8, bc_ld16(V + src));
    }
    __syncthreads();

    const int nitems = nrows * hs;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane / L, c = lane - g * L;
    for (int base = wave * G; base < nitems; base += (IP_THREADS / 64) * G) {      // wave-uniform trip count: every lane shuffles
        const int item = base + g;
        const bool inside = g < G && item < nitems;
        const int row = inside ? item / hs : 0, hl = inside ? item - row * hs : 0;
        bool active = inside;
        if (MASKED) {
            active = inside && ipm_row_nonzero(Ms, images, block_rows, row);
            if (!__any(active)) continue;            // wave-uniform
        }
        const int kcol = hl * D + c * 8;             // this lane's 8 channels inside the slab (lane c < L always: kcol + 8 <= W)
        const size_t grow = (size_t)b * rows_per_batch + r0 + row;
        const size_t col = (size_t)(h0 + hl) * D + c * 8;
        uint4 qraw = make_uint4(0, 0, 0, 0), oraw = make_uint4(0, 0, 0, 0);
        if (active) {
            qraw = bc_ld16(Q + grow * ldq + col);
            oraw = bc_ld16(O + grow * ldo + col);
        }
        const h16* qh = reinterpret_cast<const h16*>(&qraw);
        float q[8], sum[8], f;                       // O += f * sum
#pragma unroll
        for (int j = 0; j < 8; ++j) q[j] = (float)qh[j];
        if (MASKED) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sum[j] = 0.f;
            for (int i = 0; i < images; ++i) {
                float l, acc[8];
                ip_softmax_image<L>(Ks + (size_t)i * Tp * W + kcol, Vs + (size_t)i * Tp * W + kcol, W, Tp, q, scale_log2, lane, c, l, acc);
                const float fi = (float)Ms[i * block_rows + row] / l;   // the image's weight on this row, fp32 (l >= 1)
#pragma unroll
                for (int j = 0; j < 8; ++j) sum[j] = fmaf(acc[j], fi, sum[j]);
            }
            f = wv;
        } else {
            float l;
            ip_softmax_image<L>(Ks + kcol, Vs + kcol, W, T, q, scale_log2, lane, c, l, sum);
            f = wv / l;
        }
        if (active) {
            h16* oh = reinterpret_cast<h16*>(&oraw);
#pragma unroll
            for (int j = 0; j < 8; ++j) oh[j] = (h16)fmaf(sum[j], f, (float)oh[j]);
            bc_st16(O + grow * ldo + col, oraw);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------- the tiles shape
// For T = 16, 32, 48, 64 image tokens (IP-Adapter Plus: 16 per image).  Same contract, same staging idea, another work shape: a wave owns
// 16 consecutive query rows of one head (an ITEM), a workgroup a block of up to IPT_ROWS rows of one image and a slab of whole heads.
//   S^T = K . Q^T    v_mfma_f32_16x16x32_f16, A = 16 keys from the row-major K image in LDS (16 bytes per lane), B = the lane's 8 query
//                    channels straight from global memory; channels past d (d = 8, 16, 40, 80, 160 leave a k-step partly empty) are zero
//                    in BOTH operands' registers, so nothing in LDS or behind the head is multiplied.  The accumulator of key tile kt
//                    holds, on lane (query l & 15, group l >> 4), the scores of keys 16 kt + 4 (l >> 4) + r, r = 0 .. 3.
//   softmax          plain: all T scores of a query live in the 4 NT registers of its 4 lanes: one maximum and one sum through two xor
//                    shuffles (16, 32), exp2 in fp32.  The sum runs over the fp16-rounded probabilities the next product consumes.
//                    MASKED, images of Tp = 16 `tpi` tokens: a 16-key tile belongs to exactly one image, tile kt to image kt / tpi.  The
//                    maximum and the sum of every TILE go through the two shuffles; an image's maximum and its denominator l_i are those
//                    of its tiles.  Probabilities stay fp32 until the weight is known: the lane's accumulator registers of tile kt hold
//                    scores of ITS query row, so the mask value of that row, m[kt / tpi, row] / l_i in fp32, scales those four
//                    probabilities, which are then rounded to fp16.  The sum over images is the next MFMA's own sum over key tiles; w
//                    meets the fp32 accumulator at the store.
//   O^T = V^T . P^T  v_mfma_f32_16x16x16f16 per key tile: its B operand wants keys 4 (l >> 4) + j of query l & 15 in element j - exactly
//                    the accumulator's registers, converted to fp16, no lane movement.  A = 4 consecutive keys of one channel, 8 bytes
//                    from a TRANSPOSED V image [channel][T + 4] that the staging loop writes once per workgroup (2-byte LDS stores).
//                    The result has 4 consecutive channels of one query row on a lane: O is read and written 8 bytes per lane, once.
// Output channel tiles that stick out of the head (d % 16 != 0) read rows of the V image that belong to the next head or to the 16 pad
// rows behind the slab; those results are dropped.  Rows past the block are computed on zero queries and dropped.
// The two tile kernels are written out in their own sources, not as one body here: as one inlined body (the score product, the staging
// and the store once, the two softmaxes as branches or as functions) the compiler assigned attention_ip_tiles_kernel<160, 4> 74 to 76
// VGPRs where it has 86 written out, and the launch at 1280 channels, 16 x 512 rows, T = 64 took 25.8 us where it takes 24.6
// (profiles/attention_ip_refactor.md).  They share the mask block, the LDS formula below and the host side.

// mask block + row-major K image [T][W + 8] + transposed V image [W + 16][T + 4]
inline size_t ipt_lds_bytes(int T, int W, int mask_bytes) { return mask_bytes + ((size_t)T * (W + 8) + (size_t)(W + 16) * (T + 4)) * sizeof(h16); }

// ----------------------------------------------------------------------------------------------------------------------- the host side
// mask_bytes: 0 for the plain kernels, IP_MASK_BYTES for the masked ones.
struct IpGeometry {
    int slab_heads, block_rows, threads;
    size_t lds;
};

inline IpGeometry ip_scalar_geometry(int D, int heads, int T, int mask_bytes) {
    IpGeometry g;
    g.slab_heads = std::min(heads, (IP_LDS_BYTES - mask_bytes) / 4 / T / D);       // >= 1: T <= 64 and D <= 160 give 64 * 160 * 4 = 40 KiB
    g.lds = mask_bytes + (size_t)2 * T * g.slab_heads * D * sizeof(h16);
    const int per_pass = (IP_THREADS / 64) * (64 / (D / 8));                        // items the workgroup takes per pass
    g.block_rows = std::max(1, std::min(IP_MAX_ROWS, IP_ITEMS_PER_LANE * per_pass / g.slab_heads));
    g.threads = IP_THREADS;
    return g;
}

inline IpGeometry ip_tiles_geometry(int D, int heads, int T, int B, int rows_per_batch, int mask_bytes) {
    IpGeometry g;
    g.slab_heads = 1;                                                    // T = 64, D = 160: 44.4 KiB for one head (48.4 with a mask block)
    while (g.slab_heads < heads && ipt_lds_bytes(T, (g.slab_heads + 1) * D, mask_bytes) <= (size_t)IP_LDS_BYTES) ++g.slab_heads;
    g.block_rows = IPT_ROWS;
    // a small launch: narrower head slabs first (less staging per workgroup), then fewer rows
    auto wgs = [&] { return (long long)bc_ceil_div(rows_per_batch, g.block_rows) * B * bc_ceil_div(heads, g.slab_heads); };
    while (wgs() < IPT_WG_TARGET && g.slab_heads > 1) g.slab_heads = (g.slab_heads + 1) / 2;
    while (wgs() < IPT_WG_TARGET && g.block_rows > 16) g.block_rows /= 2;
    const int items = bc_ceil_div(std::min(g.block_rows, rows_per_batch), 16) * g.slab_heads;
    g.threads = 64 * std::min(IP_THREADS / 64, items);
    g.lds = ipt_lds_bytes(T, g.slab_heads * D, mask_bytes);
    return g;
}

// One launch of `kernel` over (row blocks, B, head slabs); `args` are its arguments in front of (slab_heads, block_rows); `name` = the
// entry point's own name for the error text.
template <typename... Params, typename... Args>
int ip_launch(const char* name, void (*kernel)(Params...), const IpGeometry& g, int B, int rows_per_batch, int heads, hipStream_t stream,
              Args... args) {
    const int slabs = bc_ceil_div(heads, g.slab_heads);
    BC_CHECK_ARG(slabs <= 65535, "%s: %d head slabs exceed the grid", name, slabs);
    hipLaunchKernelGGL(kernel, dim3(bc_ceil_div(rows_per_batch, g.block_rows), B, slabs), dim3(g.threads), g.lds, stream, args..., g.slab_heads,
                       g.block_rows);
    BC_CHECK_LAUNCH();
    return 0;
}

// The argument check of bc_attention_ip_with (`m` null; T image tokens) and bc_attention_ip_masked_with (`m` = its mask arguments;
// T = images * tokens_per_image is not looked at): `name` = the entry point's name without _with.
struct IpMaskArgs {
    const bc_half* mask;
    int ldm, images, Tp;
};

inline int ip_check_args(const char* name, int path, const bc_half* Q, const bc_half* K, const bc_half* V, bc_half* O, int B, int rows_per_batch,
                         int heads, int d, int T, int ldq, int ldkv, int ldo, const float* w, const IpMaskArgs* m) {
    BC_CHECK_ARG(path == 0 || path == 1, "%s_with: path=%d (0 the scalar kernel, 1 the MFMA tiles)", name, path);
    BC_CHECK_ARG(Q && K && V && O && w && (!m || m->mask), "%s: null pointer", name);
    BC_CHECK_ARG(B > 0 && B <= 65535 && rows_per_batch > 0 && heads > 0 && heads <= 65535, "%s: bad shape B=%d rows_per_batch=%d heads=%d", name, B,
                 rows_per_batch, heads);
    if (m) {
        BC_CHECK_ARG(m->images >= 1, "%s: images=%d (at least 1)", name, m->images);
        BC_CHECK_ARG(m->Tp >= 1, "%s: tokens_per_image=%d (at least 1)", name, m->Tp);
        BC_CHECK_ARG((long long)m->images * m->Tp <= BC_ATTENTION_IP_MAX_T, "%s: images=%d x tokens_per_image=%d image tokens (1 .. %d)", name,
                     m->images, m->Tp, BC_ATTENTION_IP_MAX_T);
    } else {
        BC_CHECK_ARG(T >= 1 && T <= BC_ATTENTION_IP_MAX_T, "%s: T=%d image tokens (1 .. %d)", name, T, BC_ATTENTION_IP_MAX_T);
    }
    BC_CHECK_ARG(d == 8 || d == 16 || d == 32 || d == 40 || d == 64 || d == 80 || d == 160,
                 "%s: unsupported head size d=%d (8, 16, 32, 40, 64, 80, 160)", name, d);
    const long long Cc = (long long)heads * d;
    BC_CHECK_ARG(ldq >= Cc && ldo >= Cc && ldkv >= Cc && ldq % 8 == 0 && ldo % 8 == 0 && ldkv % 8 == 0,
                 "%s: ldq=%d ldo=%d ldkv=%d must cover C=%lld and be multiples of 8", name, ldq, ldo, ldkv, Cc);
    BC_CHECK_ARG(rows_per_batch < (1 << 30), "%s: rows_per_batch=%d too large", name, rows_per_batch);
    if (m)
        BC_CHECK_ARG(m->ldm >= rows_per_batch, "%s: the mask's leading dimension ldm=%d must cover rows_per_batch=%d", name, m->ldm, rows_per_batch);
    const uintptr_t al = (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)O;
    BC_CHECK_ARG(al % 16 == 0, "%s: Q, K, V and O need 16-byte alignment", name);
    BC_CHECK_ARG((uintptr_t)w % 4 == 0, "%s: the weight is an aligned fp32 word", name);
    if (m) {
        BC_CHECK_ARG((uintptr_t)m->mask % 2 == 0, "%s: the mask is aligned fp16", name);
        BC_CHECK_ARG(path == 0 || m->Tp % 16 == 0, "%s_with: the MFMA tiles take 16, 32, 48 or 64 tokens per image, not tokens_per_image=%d", name,
                     m->Tp);
    } else {
        BC_CHECK_ARG(path == 0 || T % 16 == 0, "%s_with: the MFMA tiles take T = 16, 32, 48 or 64 image tokens, not T=%d", name, T);
    }
    return 0;
}

// f(std::integral_constant<int, D>) for the head size d / f(std::integral_constant<int, NT>) for T = 16 NT keys; 1 when there is none.
template <typename F>
int ip_dispatch_d(int d, F&& f) {
#define BC_IP_D(D) \
    case D: return f(std::integral_constant<int, D>{})
    switch (d) {
        BC_IP_D(8); BC_IP_D(16); BC_IP_D(32); BC_IP_D(40); BC_IP_D(64); BC_IP_D(80); BC_IP_D(160);
    }
#undef BC_IP_D
    return 1;
}

template <typename F>
int ip_dispatch_nt(int T, F&& f) {
    switch (T / 16) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
    }
    return 1;
}

}  // namespace
