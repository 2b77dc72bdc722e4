// Flash attention forward with SAM's decomposed relative-position bias for gfx950 (wave64, v_mfma_f32_32x32x16_f16), head_dim 40 / 64 / 80.
//
// Replaces SamVisionAttention of transformers' modeling_sam.py (the ViT-H image encoder behind the reference app's click,
// scripts/blobctrl_app.py:1019-1043): softmax(scale Q K^T + rel_h[q][kh] + rel_w[q][kw]) V over a Kh x Kw key grid - 14 x 14 windows
// (196 keys, 25 windows per image) and four global layers (64 x 64 = 4096 keys).
//
// Two launches:
//   relpos_rows_kernel   rel[b][head][q][0 .. Kh) = Q[q] . Rh[qh - j + Kh - 1], [Kh .. Kh + Kw) = Q[q] . Rw[qw - j + Kw - 1], fp32, in log2
//                        units.  Q-tile x (Kh + Kw) x d: under 1 % of the attention's FLOPs, so plain FMAs.
//   attn_relpos_kernel   the product structure of attention.hip (S^T = K . Q^T with the query on the lane, the S^T accumulator
//                        registers as the B operand of O^T += V^T . P^T, keys fed in the bit-swapped order that makes the V^T
//                        fragment one ds_read_b128).  The workgroup's rel rows sit in LDS (row stride odd: a wave's 32 queries read
//                        32 different banks); a score becomes fma(acc, scale log2 e, rel_h + rel_w) in fp32 BEFORE the row maximum.
//                        When the key grid is as wide as the key tile (the 64 x 64 global layers) the kernel runs its key-row-per-tile
//                        form instead: rel_w in registers, one rel_h read per tile (template parameter ROWTILE, below).
//   The query stays unscaled in fp16 (the bias needs it unscaled, and the scale then costs nothing: it rides in the fma).
// K / V^T tiles of 64 keys are staged through registers into one LDS stage (the next tile's global loads are in flight under the
// MFMAs of the current one).  K rows past Nkv are NOT read (zeros are staged) and their scores are masked to -inf, so their P is
// exactly 0 and the V^T padding columns (zero by contract) never count.
#include <type_traits>
#include "bc_common.h"
#include "../../include/blobctrl_sam.h"

namespace {

constexpr int QW = 32;        // queries per wave (one MFMA column tile)
constexpr int KVT = 64;       // keys per tile
constexpr int NW = 4;         // waves per workgroup
constexpr int NT = 64 * NW;

template <int D>
struct RelCfg {
    static constexpr int D16 = (D + 15) / 16;          // QK^T k-steps
    static constexpr int DK = D16 * 16;                // padded head_dim for QK^T
    static constexpr int DT = (D + 31) / 32;           // O^T row tiles
    static constexpr int DC = D / 8;                   // 16-byte chunks per K row
    static constexpr int KS = DK + 8;                  // K row stride in halves: an odd number of 16-byte chunks
    static constexpr int VS = KVT + 8;                 // V^T row stride in halves (9 chunks)
    static constexpr int K_BYTES = KVT * KS * 2;
    static constexpr int V_BYTES = DT * 32 * VS * 2;
    static constexpr int KLD = (KVT * DC + NT - 1) / NT;   // staging registers (uint4) per thread for K and for V^T
    static constexpr int VLD = (D * (KVT / 8) + NT - 1) / NT;
};

__device__ __forceinline__ float rp_halves_max(float v) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float rp_halves_sum(float v) {
    auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// rel[b][head][q][j]: one thread per (q, j); threads of a row share the Q row, neighbouring j read neighbouring table rows.
__global__ __launch_bounds__(256) void relpos_rows_kernel(const h16* __restrict__ Q, const h16* __restrict__ Rh, const h16* __restrict__ Rw,
                                                          float* __restrict__ rel, int d, int Qw, int Kh, int Kw, int Nq, int ldq,
                                                          long long q_bs, int heads) {
    const int RW = Kh + Kw;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int head = blockIdx.y, b = blockIdx.z;
    if (idx >= (long long)Nq * RW) return;
    const int q = (int)(idx / RW), j = (int)(idx % RW);
    const int qh = q / Qw, qw = q % Qw;
    const h16* qrow = Q + (size_t)b * q_bs + (size_t)q * ldq + (size_t)head * d;
    const h16* trow = j < Kh ? Rh + (size_t)(qh - j + Kh - 1) * d : Rw + (size_t)(qw - (j - Kh) + Kw - 1) * d;
    float acc = 0.f;
    for (int c = 0; c < d; c += 8) {                       // (d is a multiple of 8; Q rows and table rows are 16-byte aligned)
        const uint4 a = bc_ld16(qrow + c), t = bc_ld16(trow + c);
        const h16* ah = reinterpret_cast<const h16*>(&a);
        const h16* th = reinterpret_cast<const h16*>(&t);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf((float)ah[e], (float)th[e], acc);
    }
    rel[(((size_t)b * heads + head) * Nq + q) * RW + j] = acc * 1.4426950408889634f;
}

// ROWTILE: the key grid is KVT keys wide, so key tile t IS key row t: kh is constant over a tile and a lane's 32 key columns are the same in
// every tile.  The lane then keeps its 32 rel_w values in registers for the whole launch and reads ONE rel_h value per tile; only the rel_h
// halves of the rows are staged in LDS (half the footprint: two workgroups per CU at the 64 x 64 grid), and no key is ever masked.
template <int D, bool ROWTILE>
__global__ __launch_bounds__(NT) void attn_relpos_kernel(const h16* __restrict__ Q, const h16* __restrict__ K, const h16* __restrict__ Vt,
                                                         h16* __restrict__ O, const float* __restrict__ rel, int Nq, int Nkv, int Kh, int Kw,
                                                         int ldq, int ldk, int ldvt, int ldo, long long q_bs, long long k_bs,
                                                         long long vt_bs, long long o_bs, float scale_log2e) {
#if defined(__HIP_DEVICE_COMPILE__)
    using C = RelCfg<D>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    h16* const ks = reinterpret_cast<h16*>(smem);                               // [KVT][KS]
    h16* const vs = reinterpret_cast<h16*>(smem + C::K_BYTES);                  // [DT * 32][VS]
    float* const rs = reinterpret_cast<float*>(smem + C::K_BYTES + C::V_BYTES); // [QW * NW][RS]
    const int RW = Kh + Kw, RSW = ROWTILE ? Kh : RW, RS = RSW | 1;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qcol = lane & 31, half = lane >> 5;
    const int krow = (qcol & ~12) | ((qcol & 4) << 1) | ((qcol & 8) >> 1);      // pi(qcol): bits 2 and 3 swapped
    const int head = blockIdx.y, b = blockIdx.z;
    const int qbase = blockIdx.x * (QW * NW);
    const int q = qbase + wave * QW + qcol;

    const h16* Qb = Q + (size_t)b * q_bs + (size_t)head * D;
    const h16* Kb = K + (size_t)b * k_bs + (size_t)head * D;
    const h16* Vb = Vt + (size_t)b * vt_bs + (size_t)head * D * ldvt;
    h16* Ob = O + (size_t)b * o_bs + (size_t)head * D;
    const float* relb = rel + ((size_t)b * gridDim.y + head) * (size_t)Nq * RW;

    // ---- Q fragments (B operand): lane holds Q[q][16 s + 8 half .. + 7], unscaled; rows past Nq and columns past D are zeros ----
    h16x8 qf[C::D16];
    {
        const int qc = q < Nq ? q : Nq - 1;
#pragma unroll
        for (int s = 0; s < C::D16; ++s) {
            const int dcol = 16 * s + 8 * half;
            const uint4 raw = bc_ld16(Qb + (size_t)qc * ldq + (dcol < D ? dcol : 0));
            const h16x8 v = *reinterpret_cast<const h16x8*>(&raw);
            const h16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            qf[s] = (q < Nq && dcol < D) ? v : z;
        }
    }
    // ---- LDS: zero the K / V^T images once (padded K columns D .. DK-1 and V^T rows D .. 32 DT - 1 are never written again), rel rows ----
    for (int i = tid; i < (C::K_BYTES + C::V_BYTES) / 16; i += NT) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
    for (int i = tid; i < QW * NW * RSW; i += NT) {
        const int r = i / RSW, j = i % RSW;
        rs[r * RS + j] = qbase + r < Nq ? relb[(size_t)(qbase + r) * RW + j] : 0.f;
    }
    const float* myrel = rs + (wave * QW + qcol) * RS;
    float relw[ROWTILE ? 32 : 1];
    if (ROWTILE) {              // register 16 kt + 8 g + j <-> key column 32 kt + 16 g + 8 half + j (the accumulator's key order, below)
        const float* wrow = relb + (size_t)(q < Nq ? q : Nq - 1) * RW + Kh;
#pragma unroll
        for (int i = 0; i < 32; ++i) relw[ROWTILE ? i : 0] = wrow[32 * (i >> 4) + 16 * ((i >> 3) & 1) + 8 * half + (i & 7)];
    }

    // ---- staging: tile -> registers -> LDS ----
    uint4 kreg[C::KLD], vreg[C::VLD];
    auto load_tile = [&](const int kbase) {
#pragma unroll
        for (int i = 0; i < C::KLD; ++i) {
            const int c = i * NT + tid, key = c / C::DC, ch = c % C::DC;
            kreg[i] = (c < KVT * C::DC && kbase + key < Nkv) ? bc_ld16(Kb + (size_t)(kbase + key) * ldk + ch * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < C::VLD; ++i) {
            const int c = i * NT + tid, row = c / (KVT / 8), ch = c % (KVT / 8);
            vreg[i] = c < D * (KVT / 8) ? bc_ld16(Vb + (size_t)row * ldvt + kbase + ch * 8) : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < C::KLD; ++i) {
            const int c = i * NT + tid, key = c / C::DC, ch = c % C::DC;
            if (c < KVT * C::DC) bc_st16(ks + key * C::KS + ch * 8, kreg[i]);
        }
#pragma unroll
        for (int i = 0; i < C::VLD; ++i) {
            const int c = i * NT + tid, row = c / (KVT / 8), ch = c % (KVT / 8);
            if (c < D * (KVT / 8)) bc_st16(vs + row * C::VS + ch * 8, vreg[i]);
        }
    };

    f32x16 oacc[C::DT];
#pragma unroll
    for (int t = 0; t < C::DT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    union PFrag { h16x8 v; h16x2 p[4]; };
    typedef float f32x2 __attribute__((ext_vector_type(2)));

    const int ntiles = (Nkv + KVT - 1) / KVT;
    load_tile(0);
    for (int tile = 0; tile < ntiles; ++tile) {
        const int kbase = tile * KVT;
        __syncthreads();                                   // everybody has finished reading the previous tile (first trip: the zero fill)
        store_tile();
        __syncthreads();
        if (tile + 1 < ntiles) load_tile(kbase + KVT);     // in flight under this tile's MFMAs

        // ---- S^T[kt] = K_tile[kt] . Q^T (two 32-key tiles) ----
        f32x16 sacc[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
            for (int s = 0; s < C::D16; ++s) {
                const h16x8 kf = *reinterpret_cast<const h16x8*>(ks + (kt * 32 + krow) * C::KS + 16 * s + 8 * half);
                if (s == 0) {
                    const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], z, 0, 0, 0);
                } else {
                    sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], sacc[kt], 0, 0, 0);
                }
            }
        }
        // ---- score = acc * scale + rel_h[kh] + rel_w[kw] (log2 units, fp32), tail keys -> -inf.  Register r of lane-half h holds key
        //      kbase + 32 kt + 16 (r >> 3) + 8 h + (r & 7): runs of 8 consecutive keys, walked with (kh, kw) counters ----
        float mx = -INFINITY;
        if (ROWTILE) {
            const float relh = myrel[tile];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    sacc[kt][r] = fmaf(sacc[kt][r], scale_log2e, relw[ROWTILE ? 16 * kt + r : 0] + relh);
                    mx = fmaxf(mx, sacc[kt][r]);
                }
        } else {
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int key0 = kbase + kt * 32 + 16 * g + 8 * half;
                    int kh = key0 / Kw, kw = key0 - kh * Kw;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int r = 8 * g + j;
                        const float bias = myrel[kh < Kh ? kh : Kh - 1] + myrel[Kh + kw];
                        const float sc = fmaf(sacc[kt][r], scale_log2e, bias);
                        sacc[kt][r] = key0 + j < Nkv ? sc : -INFINITY;
                        mx = fmaxf(mx, sacc[kt][r]);
                        if (++kw == Kw) { kw = 0; ++kh; }
                    }
                }
        }
        mx = rp_halves_max(mx);                            // the partner lane holds the tile's other 32 keys of this query
        const float m_new = fmaxf(m_run, mx);              // finite: every tile holds at least one valid key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        l_run *= alpha;
#pragma unroll
        for (int t = 0; t < C::DT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[t][r] *= alpha;
        PFrag pf[2][2];
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    f32x2 e;
                    e.x = __builtin_amdgcn_exp2f(sacc[kt][8 * s2 + 2 * jj] - m_new);
                    e.y = __builtin_amdgcn_exp2f(sacc[kt][8 * s2 + 2 * jj + 1] - m_new);
                    pf[kt][s2].p[jj] = __builtin_convertvector(e, h16x2);
                    psum += e.x + e.y;
                }
        l_run += rp_halves_sum(psum);

        // ---- O^T[t] += V^T_tile[t] . P^T ; A fragment = V^T[32 t + row][32 kt + 16 s2 + 8 half .. + 7] ----
#pragma unroll
        for (int t = 0; t < C::DT; ++t)
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const h16x8 vf = *reinterpret_cast<const h16x8*>(vs + (t * 32 + qcol) * C::VS + kt * 32 + 16 * s2 + 8 * half);
                    oacc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[kt][s2].v, oacc[t], 0, 0, 0);
                }
    }

    // ---- epilogue: O[q][dd] = O^T[dd][q] / l ; register r holds row (r & 3) + 8 (r >> 2) + 4 half ----
    if (q < Nq) {
        const float inv = 1.0f / l_run;
#pragma unroll
        for (int t = 0; t < C::DT; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int dd = t * 32 + 8 * g + 4 * half;
                if (dd < D) {
                    h16x4 o4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) o4[j] = (h16)(oacc[t][4 * g + j] * inv);
                    *reinterpret_cast<h16x4*>(Ob + (size_t)q * ldo + dd) = o4;
                }
            }
    }
#endif
}

template <int D, bool ROWTILE>
int launch_relpos_form(const h16* Q, const h16* K, const h16* Vt, h16* O, const float* rel, int B, int heads, int Nq, int Nkv, int Kh, int Kw,
                       int ldq, int ldk, int ldvt, int ldo, long long qbs, long long kbs, long long vbs, long long obs, float scale,
                       hipStream_t stream) {
    using C = RelCfg<D>;
    const int lds = C::K_BYTES + C::V_BYTES + QW * NW * ((ROWTILE ? Kh : Kh + Kw) | 1) * 4;
    BC_CHECK_ARG(lds <= 160 * 1024, "bc_attention_relpos: a %d x %d key grid needs %d bytes of LDS", Kh, Kw, lds);
    static std::atomic<unsigned long long> lds_set{0};       // one bit per device ordinal; the limit is the CU's whole LDS, whatever the grid
    BC_CHECK_HIP(bc_set_max_lds(lds_set, reinterpret_cast<const void*>(&attn_relpos_kernel<D, ROWTILE>), 160 * 1024));
    dim3 grid(bc_ceil_div(Nq, QW * NW), heads, B), block(NT);
    hipLaunchKernelGGL((attn_relpos_kernel<D, ROWTILE>), grid, block, lds, stream, Q, K, Vt, O, rel, Nq, Nkv, Kh, Kw, ldq, ldk, ldvt, ldo, qbs, kbs,
                       vbs, obs, scale * 1.4426950408889634f);
    BC_CHECK_LAUNCH();
    return 0;
}

template <int D>
int launch_relpos(const h16* Q, const h16* K, const h16* Vt, h16* O, const float* rel, int B, int heads, int Nq, int Nkv, int Kh, int Kw,
                  int ldq, int ldk, int ldvt, int ldo, long long qbs, long long kbs, long long vbs, long long obs, float scale,
                  hipStream_t stream) {
    if (Kw == KVT)
        return launch_relpos_form<D, true>(Q, K, Vt, O, rel, B, heads, Nq, Nkv, Kh, Kw, ldq, ldk, ldvt, ldo, qbs, kbs, vbs, obs, scale, stream);
    return launch_relpos_form<D, false>(Q, K, Vt, O, rel, B, heads, Nq, Nkv, Kh, Kw, ldq, ldk, ldvt, ldo, qbs, kbs, vbs, obs, scale, stream);
}

}  // namespace

extern "C" int bc_attention_relpos(const bc_half* Q, const bc_half* K, const bc_half* Vt, bc_half* O, int B, int heads, int d, int Qh, int Qw,
                                   int Kh, int Kw, int ldq, int ldk, int ldvt, int ldo, long long q_bstride, long long k_bstride,
                                   long long vt_bstride, long long o_bstride, float scale, const bc_half* Rh, const bc_half* Rw, float* rel,
                                   bc_stream stream_) {
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BC_CHECK_ARG(Q && K && Vt && O && Rh && Rw && rel && B > 0 && heads > 0 && Qh > 0 && Qw > 0 && Kh > 0 && Kw > 0, "bc_attention_relpos: bad args");
    BC_CHECK_ARG(Qh == Kh && Qw == Kw, "bc_attention_relpos: the query grid %d x %d must be the key grid %d x %d", Qh, Qw, Kh, Kw);
    BC_CHECK_ARG(d == 40 || d == 64 || d == 80, "bc_attention_relpos: head_dim %d not instantiated (supported: 40, 64, 80)", d);
    const long long nq = (long long)Qh * Qw, nkv = (long long)Kh * Kw;
    BC_CHECK_ARG(nq <= (1 << 20) && nkv <= (1 << 20), "bc_attention_relpos: grid too large");
    const int Nq = (int)nq, Nkv = (int)nkv;
    BC_CHECK_ARG(ldq % 8 == 0 && ldk % 8 == 0 && ldvt % 8 == 0 && ldo % 4 == 0, "bc_attention_relpos: strides must be multiples of 8 (ldo: 4)");
    BC_CHECK_ARG(ldvt >= bc_ceil_div(Nkv, KVT) * KVT, "bc_attention_relpos: ldvt=%d must cover Nkv=%d rounded up to %d (zero padded)", ldvt, Nkv, KVT);
    BC_CHECK_ARG(q_bstride % 8 == 0 && k_bstride % 8 == 0 && vt_bstride % 8 == 0 && o_bstride % 4 == 0,
                 "bc_attention_relpos: batch strides must be multiples of 8");
    BC_CHECK_ARG(heads <= 65535 && B <= 65535, "bc_attention_relpos: heads / batch above the grid limit");
    const h16* q = reinterpret_cast<const h16*>(Q);
    const h16* k = reinterpret_cast<const h16*>(K);
    const h16* v = reinterpret_cast<const h16*>(Vt);
    const h16* rh = reinterpret_cast<const h16*>(Rh);
    const h16* rw = reinterpret_cast<const h16*>(Rw);
    h16* o = reinterpret_cast<h16*>(O);
    {
        dim3 grid(bc_ceil_div((long long)Nq * (Kh + Kw), 256), heads, B), block(256);
        hipLaunchKernelGGL(relpos_rows_kernel, grid, block, 0, stream, q, rh, rw, rel, d, Qw, Kh, Kw, Nq, ldq, q_bstride, heads);
        BC_CHECK_LAUNCH();
    }
    switch (d) {
        case 40: return launch_relpos<40>(q, k, v, o, rel, B, heads, Nq, Nkv, Kh, Kw, ldq, ldk, ldvt, ldo, q_bstride, k_bstride, vt_bstride, o_bstride, scale, stream);
        case 64: return launch_relpos<64>(q, k, v, o, rel, B, heads, Nq, Nkv, Kh, Kw, ldq, ldk, ldvt, ldo, q_bstride, k_bstride, vt_bstride, o_bstride, scale, stream);
        default: return launch_relpos<80>(q, k, v, o, rel, B, heads, Nq, Nkv, Kh, Kw, ldq, ldk, ldvt, ldo, q_bstride, k_bstride, vt_bstride, o_bstride, scale, stream);
    }
}
