// Connected-component labelling of binary masks and remove_small_regions on top of it (include/blobctrl_masks.h).  gfx950.
//
// Labels are CANONICAL: the label of a pixel is the smallest raster index of its 8-connected component.  A union-find whose links only
// ever point to a SMALLER index gives that directly - the root of a tree is the minimum of its members - and makes every loop below
// terminate by the monotone decrease of a label: no workgroup ever waits for another, and any interleaving ends in the same array.
//
//   tile_label   one workgroup per MR_TH x MR_TW tile: union-find in LDS over the tile's pixels (ds atomic min), roots written as GLOBAL
//                raster indices (a tile's raster order is the image's, so the tile minimum is a member's global minimum).  Pixels start
//                linked to the first pixel of their horizontal run, and a vertical pair that a neighbour's pair implies is left out: on a
//                large component nearly every union would otherwise walk to, and contend for, the same root.  For the removal it also
//                counts the pixels of every tile-local root in LDS and stores that count at the root (0 elsewhere).
//   merge        one thread per pixel of a tile's first row / first column: unions it with its neighbours in the tile above / to the
//                left.  The label array is touched ONLY through agent-scope atomics here (relaxed loads for find, atomic min for
//                links): the XCDs' private L2s make a plain load of a word another workgroup links in the same launch unreliable.
//   flatten      every pixel -> its root.  Words change under the readers' feet here too, but only from one valid ancestor to the root
//                itself, and a root is never rewritten, so find ends at the same root whichever value it sees.  A tile root that is not
//                the component's root adds its count to the root's: one atomic per (tile, component), not one per pixel.
//   roots        per mask: the largest component (ties: smallest root) as one 64-bit atomic max, and whether any component is small.
//   apply        sets / clears the small components, and reduces area and box of the mask as it leaves.
#include "bc_common.h"
#include "../../include/blobctrl_masks.h"

namespace {

constexpr int MR_THREADS = 256, MR_TH = 32, MR_TW = 64, MR_TILE = MR_TH * MR_TW, MR_PER = MR_TILE / MR_THREADS;
constexpr int MR_CHUNK = 4096;                        // pixels of one mask per workgroup in the per-pixel passes
constexpr int MR_EMPTY_LO = 0x7fffffff, MR_EMPTY_HI = -1;
static_assert(MR_TW == 64, "a wave covers one tile row (the run counting below relies on it)");

// ---- union by minimum in LDS
__device__ __forceinline__ int lds_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_find(int* L, int x) {
    int n;
    while ((n = lds_load(L + x)) != x) x = n;        // links point down: ends at a root
    return x;
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }                                     // a > b: hang a under b
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;                        // a was still a root
        a = old;                                     // somebody linked a to `old` first: L[a] = min(old, b) now, (old, b) is left to join
    }
}

// ---- the same on the global label array: agent-scope atomics only
__device__ __forceinline__ int g_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(int* L, int x) {
    int n;
    while ((n = g_load(L + x)) != x) x = n;
    return x;
}
__device__ __forceinline__ void g_union(int* L, int a, int b) {
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// The per-mask words the roots pass hands to the apply pass live in the mask's row of `out` until apply overwrites it: a 64-bit key in the
// row's 8-byte aligned slot (ints 0-1 or 1-2 of the six) and the "a small component exists" flag in int 5.  tile_label zeroes the row.
__device__ __forceinline__ unsigned long long* mr_key_slot(int* row) {
    return reinterpret_cast<unsigned long long*>(row + ((reinterpret_cast<uintptr_t>(row) >> 2) & 1));     // (row is aligned to 4 bytes)
}

template <bool AREA>
__global__ __launch_bounds__(MR_THREADS) void mr_tile_label_kernel(const unsigned char* __restrict__ masks, int H, int W, int tilesX, int tilesY,
                                                                   int fg, int* __restrict__ labels, int* __restrict__ areas, int* __restrict__ out) {
    __shared__ int L[MR_TILE];
    __shared__ int cnt[AREA ? MR_TILE : 1];
    const int tiles = tilesX * tilesY, tid = threadIdx.x;
    const long long k = blockIdx.x / tiles;
    const int t = blockIdx.x % tiles, y0 = (t / tilesX) * MR_TH, x0 = (t % tilesX) * MR_TW;
    const long long base = k * ((long long)H * W);
    const unsigned char* m = masks + base;
    const int lane = tid & 63;                       // a wave holds one tile row: lane = column in the tile
    bool in[MR_PER];
    unsigned long long rowmask[MR_PER];
#pragma unroll
    for (int j = 0; j < MR_PER; ++j) {
        const int p = tid + j * MR_THREADS, gy = y0 + (p >> 6), gx = x0 + lane;
        in[j] = gy < H && gx < W && ((m[gy * W + gx] != 0) == (fg != 0));
        rowmask[j] = __ballot(in[j]);
        // every pixel starts linked to the first pixel of its horizontal run: rows need no unions of their own
        const unsigned long long gaps = ~rowmask[j] & ((1ull << lane) - 1);
        const int start = gaps ? 64 - __clzll((long long)gaps) : 0;
        L[p] = in[j] ? p - lane + start : -1;        // pixels past the image's edge are "other": never a neighbour
        if constexpr (AREA) cnt[p] = 0;
    }
    if constexpr (AREA) {
        if (t == 0 && tid < 6) out[k * 6 + tid] = 0;
    }
    __syncthreads();
    // Between rows a pixel joins N, or NW / NE when N is not set - but only where the pair is not implied by a neighbour's: with the left
    // neighbour and NW both set, (left, NW) carries (p, N); with N unset, the left neighbour's own N is NW, the right one's is NE.
#pragma unroll
    for (int j = 0; j < MR_PER; ++j) {
        const int p = tid + j * MR_THREADS;
        if (!in[j] || p < MR_TW) continue;
        const bool left = lane > 0 && ((rowmask[j] >> (lane - 1)) & 1), right = lane < MR_TW - 1 && ((rowmask[j] >> (lane + 1)) & 1);
        const bool nw = lane > 0 && lds_load(L + p - MR_TW - 1) >= 0, ne = lane < MR_TW - 1 && lds_load(L + p - MR_TW + 1) >= 0;
        if (lds_load(L + p - MR_TW) >= 0) {
            if (!(left && nw)) lds_union(L, p, p - MR_TW);
        } else {
            if (nw && !left) lds_union(L, p, p - MR_TW - 1);
            if (ne && !right) lds_union(L, p, p - MR_TW + 1);
        }
    }
    __syncthreads();
    int root[MR_PER];
#pragma unroll
    for (int j = 0; j < MR_PER; ++j) root[j] = in[j] ? lds_find(L, tid + j * MR_THREADS) : -1;
    if constexpr (AREA) {
        // lanes that share a root with their left neighbour form a run, and the run's head adds its length
#pragma unroll
        for (int j = 0; j < MR_PER; ++j) {
            const int r = root[j], prev = __shfl_up(r, 1, 64);
            const bool head = lane == 0 || prev != r;
            const unsigned long long heads = __ballot(head);
            if (head && r >= 0) {
                const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
                const int next = rest ? lane + __ffsll((long long)rest) : 64;
                __hip_atomic_fetch_add(cnt + r, next - lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        __syncthreads();
    }
    int* lab = labels + base;
#pragma unroll
    for (int j = 0; j < MR_PER; ++j) {
        const int p = tid + j * MR_THREADS, gy = y0 + (p >> 6), gx = x0 + (p & 63);
        if (gy >= H || gx >= W) continue;
        const int r = root[j], gidx = gy * W + gx;
        lab[gidx] = r < 0 ? -1 : (y0 + (r >> 6)) * W + x0 + (r & 63);
        if constexpr (AREA) areas[base + gidx] = r == p ? cnt[p] : 0;
    }
}

// nh = (tilesY - 1) * W pixels on first rows of tiles, then (tilesX - 1) * H on first columns, per mask
__global__ __launch_bounds__(MR_THREADS) void mr_merge_kernel(int* labels, int H, int W, int nh, int nb, long long total) {
    const long long id = (long long)blockIdx.x * MR_THREADS + threadIdx.x;
    if (id >= total) return;
    int* L = labels + (id / nb) * ((long long)H * W);
    int b = (int)(id % nb);
    // As inside a tile, a pair is left out where a neighbour's pair implies it.  What the column pass relies on lies inside one tile (vertical
    // neighbours, joined by tile_label) or is another pair of the column pass further up; the row pass relies on horizontal neighbours, which
    // tile_label or the column pass join - so nothing here relies on itself, the four pixels around a tile corner included.
    if (b < nh) {
        const int y = (b / W + 1) * MR_TH, x = b % W, p = y * W + x;
        if (g_load(L + p) < 0) return;
        const bool left = x > 0 && g_load(L + p - 1) >= 0, right = x < W - 1 && g_load(L + p + 1) >= 0;   // (column W - 1 and column 0 of
        const bool nw = x > 0 && g_load(L + p - W - 1) >= 0, ne = x < W - 1 && g_load(L + p - W + 1) >= 0;   //  the next row are no neighbours)
        if (g_load(L + p - W) >= 0) {
            if (!(left && nw)) g_union(L, p, p - W);
        } else {
            if (nw && !left) g_union(L, p, p - W - 1);
            if (ne && !right) g_union(L, p, p - W + 1);
        }
    } else {
        b -= nh;
        const int x = (b / H + 1) * MR_TW, y = b % H, p = y * W + x;
        if (g_load(L + p) < 0) return;
        const bool top = y % MR_TH == 0, bottom = (y + 1) % MR_TH == 0 || y == H - 1;      // p's first / last row in its tile
        const bool w = g_load(L + p - 1) >= 0;
        const bool nw = y > 0 && g_load(L + p - W - 1) >= 0, sw = y < H - 1 && g_load(L + p + W - 1) >= 0;   // (rows of no other mask)
        const bool up = !top && g_load(L + p - W) >= 0, down = !bottom && g_load(L + p + W) >= 0;          // ... in p's own tile
        if (w && !(up && nw)) g_union(L, p, p - 1);
        if (nw && !((w && !top) || up)) g_union(L, p, p - W - 1);
        if (sw && !((w && !bottom) || down)) g_union(L, p, p + W - 1);
    }
}

template <bool AREA>
__global__ __launch_bounds__(MR_THREADS) void mr_flatten_kernel(int* labels, int* areas, int HW, int chunks) {
    const long long k = blockIdx.x / chunks;
    const int lo = (blockIdx.x % chunks) * MR_CHUNK, len = min(MR_CHUNK, HW - lo);
    int* L = labels + k * HW;
    for (int i = threadIdx.x; i < len; i += MR_THREADS) {
        const int p = lo + i, l = g_load(L + p);
        if (l < 0) continue;
        const int r = g_find(L, l);
        if (r != l) __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (AREA) {
            // p is a tile's root (count > 0) under another tile's root: hand the count up.  Only roots of components are added to, and
            // a root never reads its own count here, so no word is both read plainly and added to in this launch.
            if (r != p) {
                const int a = areas[k * HW + p];
                if (a > 0) __hip_atomic_fetch_add(areas + k * HW + r, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

__global__ __launch_bounds__(MR_THREADS) void mr_roots_kernel(const int* __restrict__ labels, const int* __restrict__ areas, int HW, int chunks,
                                                              int area_thresh, int* out) {
    const long long k = blockIdx.x / chunks;
    const int lo = (blockIdx.x % chunks) * MR_CHUNK, len = min(MR_CHUNK, HW - lo);
    unsigned long long best = 0;                      // (area << 32) | (2^31 - 1 - root): the maximum is the largest area, then the first root
    int small = 0;
    for (int i = threadIdx.x; i < len; i += MR_THREADS) {
        const int p = lo + i, a = areas[k * HW + p];
        if (a > 0 && labels[k * HW + p] == p) {
            const unsigned long long key = ((unsigned long long)a << 32) | (unsigned)(0x7fffffff - p);
            best = key > best ? key : best;
            small |= a < area_thresh ? 1 : 0;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(best, d, 64);
        best = o > best ? o : best;
        small |= __shfl_xor(small, d, 64);
    }
    __shared__ unsigned long long wbest[MR_THREADS / 64];
    __shared__ int wsmall[MR_THREADS / 64];
    if ((threadIdx.x & 63) == 0) { wbest[threadIdx.x >> 6] = best; wsmall[threadIdx.x >> 6] = small; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MR_THREADS / 64; ++w) { best = wbest[w] > best ? wbest[w] : best; small |= wsmall[w]; }
        int* row = out + k * 6;
        if (best) __hip_atomic_fetch_max(mr_key_slot(row), best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (small) __hip_atomic_fetch_or(row + 5, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct RegionAcc {
    int area, x0, y0, x1, y1;
};
__device__ __forceinline__ void mr_wave_reduce(RegionAcc& a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.area += __shfl_xor(a.area, d, 64);
        a.x0 = min(a.x0, __shfl_xor(a.x0, d, 64)); a.y0 = min(a.y0, __shfl_xor(a.y0, d, 64));
        a.x1 = max(a.x1, __shfl_xor(a.x1, d, 64)); a.y1 = max(a.y1, __shfl_xor(a.y1, d, 64));
    }
}
__device__ __forceinline__ void mr_write_row(int* row, int changed, const RegionAcc& a) {
    const bool any = a.area > 0;
    row[0] = changed; row[1] = a.area;
    row[2] = any ? a.x0 : 0; row[3] = any ? a.y0 : 0; row[4] = any ? a.x1 : 0; row[5] = any ? a.y1 : 0;
}

// chunks = max(1, HW / MR_CHUNK) and the last chunk takes the remainder, so that with chunks > 1 every chunk owns at least five label words:
// a workgroup reads the labels of its own pixels only, and once it has read them all it parks its five partials in the first of them
// (mr_combine_kernel reads them).  With one chunk the workgroup writes the mask's row of `out` itself.
__global__ __launch_bounds__(MR_THREADS) void mr_apply_kernel(unsigned char* masks, int* labels, const int* __restrict__ areas, int W, int HW,
                                                              int chunks, int area_thresh, int mode, int* out) {
    const long long k = blockIdx.x / chunks;
    const int c = blockIdx.x % chunks, lo = c * MR_CHUNK, len = (c == chunks - 1 ? HW : lo + MR_CHUNK) - lo;
    int* row = out + k * 6;
    const unsigned long long key = *mr_key_slot(row);
    const int changed = row[5];
    const int best_area = (int)(key >> 32), best_root = 0x7fffffff - (int)(unsigned)(key & 0xffffffffull);
    const bool keep_largest = mode == 1 && best_area < area_thresh;                     // every component is small: the largest stays
    unsigned char* m = masks + k * HW;
    int* L = labels + k * HW;
    RegionAcc acc = {0, MR_EMPTY_LO, MR_EMPTY_LO, MR_EMPTY_HI, MR_EMPTY_HI};
    for (int i = threadIdx.x; i < len; i += MR_THREADS) {
        const int p = lo + i, l = L[p];
        bool v = (l >= 0) == (mode == 1);            // the pixel's value as it came: labelled pixels are the set ones in mode 1, the zeros in mode 0
        if (l >= 0 && areas[k * HW + l] < area_thresh && !(keep_largest && l == best_root)) {
            v = mode == 0;
            m[p] = v ? 1 : 0;
        }
        if (v) {
            const int y = p / W, x = p - y * W;
            acc.area += 1;
            acc.x0 = min(acc.x0, x); acc.x1 = max(acc.x1, x);
            acc.y0 = min(acc.y0, y); acc.y1 = max(acc.y1, y);
        }
    }
    mr_wave_reduce(acc);
    __shared__ int part[MR_THREADS / 64][5];
    if ((threadIdx.x & 63) == 0) {
        int* q = part[threadIdx.x >> 6];
        q[0] = acc.area; q[1] = acc.x0; q[2] = acc.y0; q[3] = acc.x1; q[4] = acc.y1;
    }
    __syncthreads();                                  // every label of this chunk, and the row's key and flag, have been read
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < MR_THREADS / 64; ++w) {
            acc.area += part[w][0];
            acc.x0 = min(acc.x0, part[w][1]); acc.y0 = min(acc.y0, part[w][2]);
            acc.x1 = max(acc.x1, part[w][3]); acc.y1 = max(acc.y1, part[w][4]);
        }
        if (chunks == 1) {
            mr_write_row(row, changed, acc);
        } else {
            L[lo] = acc.area; L[lo + 1] = acc.x0; L[lo + 2] = acc.y0; L[lo + 3] = acc.x1; L[lo + 4] = acc.y1;
        }
    }
}

__global__ __launch_bounds__(64) void mr_combine_kernel(const int* __restrict__ labels, int HW, int chunks, int* out) {
    const long long k = blockIdx.x;
    RegionAcc a = {0, MR_EMPTY_LO, MR_EMPTY_LO, MR_EMPTY_HI, MR_EMPTY_HI};
    for (int c = threadIdx.x; c < chunks; c += 64) {
        const int* p = labels + k * HW + (long long)c * MR_CHUNK;
        a.area += p[0];
        a.x0 = min(a.x0, p[1]); a.y0 = min(a.y0, p[2]); a.x1 = max(a.x1, p[3]); a.y1 = max(a.y1, p[4]);
    }
    mr_wave_reduce(a);
    if (threadIdx.x == 0) {
        int* row = out + k * 6;
        mr_write_row(row, row[5], a);                 // (the flag is read before the row is written)
    }
}

struct MaskGeom {
    int tilesX, tilesY, nh, nb, chunks, apply_chunks;
    long long HW;
};

// everything a launch below relies on; 1 with bc_last_error() set when the arguments are bad
int mr_geometry(const char* who, const void* masks, int n, int H, int W, const int* labels, MaskGeom& g) {
    BC_CHECK_ARG(masks && labels && n > 0 && H > 0 && W > 0, "%s: bad args (null pointer, or n, H, W <= 0)", who);
    g.HW = (long long)H * W;
    BC_CHECK_ARG(g.HW < (1ll << 31), "%s: a mask of %d x %d does not fit 2^31 elements", who, H, W);
    g.tilesX = bc_ceil_div(W, MR_TW);
    g.tilesY = bc_ceil_div(H, MR_TH);
    g.nh = (g.tilesY - 1) * W;
    g.nb = g.nh + (g.tilesX - 1) * H;
    g.chunks = bc_ceil_div(g.HW, MR_CHUNK);
    g.apply_chunks = (int)std::max(1ll, g.HW / MR_CHUNK);
    BC_CHECK_ARG((long long)n * g.tilesX * g.tilesY <= 0x7fffffffll && (long long)n * g.chunks <= 0x7fffffffll &&
                 ((long long)n * g.nb + MR_THREADS - 1) / MR_THREADS <= 0x7fffffffll, "%s: %d masks of %d x %d exceed the grid", who, n, H, W);
    return 0;
}

template <bool AREA>
int mr_label_phase(int phase, const unsigned char* masks, int n, int H, int W, int fg, int* labels, int* areas, int* out, const MaskGeom& g,
                   hipStream_t s) {
    if (phase == 0) {
        hipLaunchKernelGGL(mr_tile_label_kernel<AREA>, dim3(n * g.tilesX * g.tilesY), dim3(MR_THREADS), 0, s, masks, H, W, g.tilesX, g.tilesY, fg,
                           labels, areas, out);
    } else if (phase == 1) {
        if (g.nb == 0) return 0;                      // a single tile: nothing to merge
        const long long total = (long long)n * g.nb;
        hipLaunchKernelGGL(mr_merge_kernel, dim3((unsigned)((total + MR_THREADS - 1) / MR_THREADS)), dim3(MR_THREADS), 0, s, labels, H, W, g.nh,
                           g.nb, total);
    } else {
        hipLaunchKernelGGL(mr_flatten_kernel<AREA>, dim3(n * g.chunks), dim3(MR_THREADS), 0, s, labels, areas, (int)g.HW, g.chunks);
    }
    BC_CHECK_LAUNCH();
    return 0;
}

int mr_remove_phase(int phase, unsigned char* masks, int n, int H, int W, int area_thresh, int mode, int* labels, int* areas, int* out,
                    const MaskGeom& g, hipStream_t s) {
    if (phase <= 2) return mr_label_phase<true>(phase, masks, n, H, W, mode, labels, areas, out, g, s);   // mode 1 labels the set pixels
    if (phase == 3) {
        hipLaunchKernelGGL(mr_roots_kernel, dim3(n * g.chunks), dim3(MR_THREADS), 0, s, labels, areas, (int)g.HW, g.chunks, area_thresh, out);
        BC_CHECK_LAUNCH();
        return 0;
    }
    hipLaunchKernelGGL(mr_apply_kernel, dim3(n * g.apply_chunks), dim3(MR_THREADS), 0, s, masks, labels, areas, W, (int)g.HW, g.apply_chunks,
                       area_thresh, mode, out);
    BC_CHECK_LAUNCH();
    if (g.apply_chunks > 1) {
        hipLaunchKernelGGL(mr_combine_kernel, dim3(n), dim3(64), 0, s, labels, (int)g.HW, g.apply_chunks, out);
        BC_CHECK_LAUNCH();
    }
    return 0;
}

int mr_remove_args(const char* who, const void* masks, int n, int H, int W, int area_thresh, int mode, const int* labels, const int* areas,
                   const int* out, MaskGeom& g) {
    BC_CHECK_ARG(areas && out, "%s: bad args (null pointer)", who);
    BC_CHECK_ARG(area_thresh >= 0, "%s: area_thresh %d is negative", who, area_thresh);
    BC_CHECK_ARG(mode == 0 || mode == 1, "%s: mode %d is neither 0 (holes) nor 1 (islands)", who, mode);
    BC_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0, "%s: out must be aligned to 4 bytes", who);
    return mr_geometry(who, masks, n, H, W, labels, g);
}

}  // namespace

extern "C" int bc_mask_label(const unsigned char* masks, int n, int H, int W, int fg, int* labels, bc_stream stream) {
    MaskGeom g;
    if (mr_geometry("bc_mask_label", masks, n, H, W, labels, g)) return 1;
    for (int phase = 0; phase < 3; ++phase) {
        const int rc = mr_label_phase<false>(phase, masks, n, H, W, fg, labels, nullptr, nullptr, g, reinterpret_cast<hipStream_t>(stream));
        if (rc) return rc;
    }
    return 0;
}

extern "C" int bc_mask_remove_small_phase(unsigned char* masks, int n, int H, int W, int area_thresh, int mode, int* labels, int* areas, int* out,
                                          int phase, bc_stream stream) {
    MaskGeom g;
    if (mr_remove_args("bc_mask_remove_small_phase", masks, n, H, W, area_thresh, mode, labels, areas, out, g)) return 1;
    BC_CHECK_ARG(phase >= 0 && phase < BC_MASK_REGION_PHASES, "bc_mask_remove_small_phase: phase %d outside 0 .. %d", phase, BC_MASK_REGION_PHASES - 1);
    return mr_remove_phase(phase, masks, n, H, W, area_thresh, mode, labels, areas, out, g, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int bc_mask_remove_small(unsigned char* masks, int n, int H, int W, int area_thresh, int mode, int* labels, int* areas, int* out,
                                    bc_stream stream) {
    MaskGeom g;
    if (mr_remove_args("bc_mask_remove_small", masks, n, H, W, area_thresh, mode, labels, areas, out, g)) return 1;
    for (int phase = 0; phase < BC_MASK_REGION_PHASES; ++phase) {
        const int rc = mr_remove_phase(phase, masks, n, H, W, area_thresh, mode, labels, areas, out, g, reinterpret_cast<hipStream_t>(stream));
        if (rc) return rc;
    }
    return 0;
}
