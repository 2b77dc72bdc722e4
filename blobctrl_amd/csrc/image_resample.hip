// Pillow's 8-bit image resize on the device (include/blobctrl_resample.h): two table-driven passes over interleaved uint8 RGB.  gfx950.
//
//   rs_horizontal    tmp[i][r][x][c] from row r0 + r of the source, for the rows the vertical pass reads and the window's columns.
//   rs_vertical_u8   the window of the resized frame as uint8, from the intermediate (or from the source when the width stays).
//   rs_vertical_f32  the same value through a [3][256] table of floats into a planar fp32 frame, zero outside the window.
//
// Integer arithmetic only: 2^21 + sum coeff * byte in 32 bits (unsigned, so a table the host would never build wraps instead of being
// undefined), an arithmetic shift by 22, a clamp.  Byte-bound and tiny, so the one thing that matters is that a wave's traffic is
// contiguous: a thread takes RS_PER consecutive bytes of the output (one 32-bit store, or RS_PER consecutive floats in one 128-bit store,
// where the address allows it), consecutive lanes take consecutive groups, and the taps of a group are bytes of one source row (horizontal)
// or the same RS_PER bytes of consecutive rows (vertical).  The tables are a few KiB and stay in cache.  The tables are in device memory,
// where the library cannot check them: every source index is tested against the input before it is used.
#include "bc_common.h"
#include "../../include/blobctrl_resample.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PER = 4;                              // consecutive output elements per thread
constexpr int RS_BITS = 22;                            // Pillow's PRECISION_BITS for 8-bit channels
constexpr int RS_MAX_KSIZE = 6 * BC_EDIT_MAX_DIM + 1;  // lanczos (support 3) reducing BC_EDIT_MAX_DIM to 1: ceil(3 * 16384) * 2 + 1

__device__ __forceinline__ unsigned rs_clip(unsigned acc) {
    const int v = (int)acc >> RS_BITS;
    return (unsigned)min(max(v, 0), 255);
}

// One output byte of a pass: taps at `base + index * stride` for index = first + t - origin, kept when 0 <= index < extent.
__device__ __forceinline__ unsigned rs_pass(const unsigned char* __restrict__ base, long long stride, int origin, int extent,
                                            const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize, int o) {
    const long long first = (long long)bounds[2 * (long long)o] - origin;
    const int taps = min(bounds[2 * (long long)o + 1], ksize);
    const int* __restrict__ k = coeffs + (long long)o * ksize;
    unsigned acc = 1u << (RS_BITS - 1);
    for (int t = 0; t < taps; ++t) {
        const long long s = first + t;
        if (s >= 0 && s < extent) acc += (unsigned)k[t] * (unsigned)base[s * stride];
    }
    return rs_clip(acc);
}

__device__ __forceinline__ void rs_put_bytes(unsigned char* dst, unsigned v, int cnt) {
    if (cnt == RS_PER && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
        *reinterpret_cast<unsigned*>(dst) = v;
    } else {
        for (int j = 0; j < cnt; ++j) dst[j] = (unsigned char)(v >> (8 * j));
    }
}

// total = rows * cw * 3 bytes of tmp per image, chunks = workgroups per image
__global__ __launch_bounds__(RS_THREADS) void rs_horizontal_kernel(const unsigned char* __restrict__ src, int H, int W, int r0,
                                                                   const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize,
                                                                   int x0, int cw, int total, int chunks, unsigned char* __restrict__ tmp) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p0 = (c * RS_THREADS + (int)threadIdx.x) * RS_PER;          // < total + 1024 <= 3 * 2^28 + 1024
    if (p0 >= total) return;
    const int rb = cw * 3;
    int r = p0 / rb, x = (p0 - r * rb) / 3, ch = p0 - r * rb - x * 3;
    const int cnt = min(RS_PER, total - p0);
    unsigned v = 0;
    for (int j = 0; j < cnt; ++j) {
        const unsigned char* row = src + ((long long)i * H + r0 + r) * W * 3 + ch;
        v |= rs_pass(row, 3, 0, W, bounds, coeffs, ksize, x0 + x) << (8 * j);
        if (++ch == 3) { ch = 0; if (++x == cw) { x = 0; ++r; } }
    }
    rs_put_bytes(tmp + (long long)i * total + p0, v, cnt);
}

// total = ch * cw * 3 bytes of out per image
__global__ __launch_bounds__(RS_THREADS) void rs_vertical_u8_kernel(const unsigned char* __restrict__ in, int IH, int IW, int r0, int xin0,
                                                                    const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize,
                                                                    int y0, int cw, int total, int chunks, unsigned char* __restrict__ out) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p0 = (c * RS_THREADS + (int)threadIdx.x) * RS_PER;
    if (p0 >= total) return;
    const int rb = cw * 3;
    int y = p0 / rb, b = p0 - y * rb;
    const int cnt = min(RS_PER, total - p0);
    const unsigned char* frame = in + ((long long)i * IH * IW + xin0) * 3;
    unsigned v = 0;
    for (int j = 0; j < cnt; ++j) {
        v |= rs_pass(frame + b, (long long)IW * 3, r0, IH, bounds, coeffs, ksize, y0 + y) << (8 * j);
        if (++b == rb) { b = 0; ++y; }
    }
    rs_put_bytes(out + (long long)i * total + p0, v, cnt);
}

// total = 3 * PH * PW floats of out per image
__global__ __launch_bounds__(RS_THREADS) void rs_vertical_f32_kernel(const unsigned char* __restrict__ in, int IH, int IW, int r0, int xin0,
                                                                     const int* __restrict__ bounds, const int* __restrict__ coeffs, int ksize,
                                                                     int y0, int ch, int cw, const float* __restrict__ lut, int PH, int PW,
                                                                     int total, int chunks, float* __restrict__ out) {
    const int i = blockIdx.x / chunks, c = blockIdx.x - i * chunks;
    const int p0 = (c * RS_THREADS + (int)threadIdx.x) * RS_PER;
    if (p0 >= total) return;
    const int plane = PH * PW;
    int k = p0 / plane, y = (p0 - k * plane) / PW, x = p0 - k * plane - y * PW;
    const int cnt = min(RS_PER, total - p0);
    const unsigned char* frame = in + ((long long)i * IH * IW + xin0) * 3;
    float f[RS_PER] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < RS_PER; ++j) {
        if (j < cnt) {
            if (y < ch && x < cw)
                f[j] = lut[k * 256 + (int)rs_pass(frame + (long long)x * 3 + k, (long long)IW * 3, r0, IH, bounds, coeffs, ksize, y0 + y)];
            if (++x == PW) { x = 0; if (++y == PH) { y = 0; ++k; } }
        }
    }
    float* dst = out + (long long)i * total + p0;
    if (cnt == RS_PER && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
#pragma unroll
        for (int j = 0; j < RS_PER; ++j)
            if (j < cnt) dst[j] = f[j];
    }
}

// what both entry points ask of a pass's tables and of an axis of sizes; 1 with bc_last_error() set when the arguments are bad
int rs_tables(const char* who, const char* axis, const int* bounds, const int* coeffs, int ksize) {
    BC_CHECK_ARG(bounds && coeffs, "%s: bad args (null pointer: bounds_%s or coeffs_%s)", who, axis, axis);
    BC_CHECK_ARG(((reinterpret_cast<uintptr_t>(bounds) | reinterpret_cast<uintptr_t>(coeffs)) & 3) == 0,
                 "%s: bounds_%s and coeffs_%s must be aligned to 4 bytes", who, axis, axis);
    BC_CHECK_ARG(ksize >= 1 && ksize <= RS_MAX_KSIZE, "%s: ksize = %d taps a row (it must be 1 .. %d)", who, ksize, RS_MAX_KSIZE);
    return 0;
}

int rs_chunks(const char* who, int n, long long total, int& chunks) {
    chunks = bc_ceil_div(total, (long long)RS_THREADS * RS_PER);
    BC_CHECK_ARG((long long)n * chunks <= 0x7fffffffll, "%s: %d images of %lld output elements exceed the grid", who, n, total);
    return 0;
}

}  // namespace

extern "C" int bc_resample_horizontal(const unsigned char* src, int n, int H, int W, int r0, int rows, const int* bounds_x, const int* coeffs_x,
                                      int ksize, int ow, int x0, int cw, unsigned char* tmp, bc_stream stream) {
    const char* who = "bc_resample_horizontal";
    BC_CHECK_ARG(src && tmp, "%s: bad args (null pointer)", who);
    if (rs_tables(who, "x", bounds_x, coeffs_x, ksize)) return 1;
    BC_CHECK_ARG(n > 0 && H > 0 && W > 0 && ow > 0, "%s: bad args (n, H, W, ow <= 0)", who);
    BC_CHECK_ARG(H <= BC_EDIT_MAX_DIM && W <= BC_EDIT_MAX_DIM && ow <= BC_EDIT_MAX_DIM,
                 "%s: %d x %d -> width %d exceeds the limit of %d a side", who, H, W, ow, BC_EDIT_MAX_DIM);
    BC_CHECK_ARG(r0 >= 0 && rows > 0 && (long long)r0 + rows <= H, "%s: rows [%d, %d + %d) leave the source of %d rows", who, r0, r0, rows, H);
    BC_CHECK_ARG(x0 >= 0 && cw > 0 && (long long)x0 + cw <= ow, "%s: window columns [%d, %d + %d) leave the resized frame of %d columns", who, x0, x0, cw,
                 ow);
    const long long total = (long long)rows * cw * 3;
    int chunks;
    if (rs_chunks(who, n, total, chunks)) return 1;
    hipLaunchKernelGGL(rs_horizontal_kernel, dim3(n * chunks), dim3(RS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), src, H, W, r0, bounds_x,
                       coeffs_x, ksize, x0, cw, (int)total, chunks, tmp);
    BC_CHECK_LAUNCH();
    return 0;
}

extern "C" int bc_resample_vertical(const unsigned char* in, int n, int IH, int IW, int r0, int xin0, const int* bounds_y, const int* coeffs_y,
                                    int ksize, int oh, int y0, int ch, int cw, unsigned char* out_u8, float* out_f32, const float* lut, int PH,
                                    int PW, bc_stream stream) {
    const char* who = "bc_resample_vertical";
    BC_CHECK_ARG(in && (out_u8 || out_f32), "%s: bad args (null pointer)", who);
    BC_CHECK_ARG(!(out_u8 && out_f32), "%s: one epilogue a launch (out_u8 and out_f32 are both set)", who);
    BC_CHECK_ARG(out_f32 ? lut != nullptr : lut == nullptr, "%s: lut goes with out_f32 and with it only (null pointer, or set beside out_u8)", who);
    if (rs_tables(who, "y", bounds_y, coeffs_y, ksize)) return 1;
    BC_CHECK_ARG(n > 0 && IH > 0 && IW > 0 && oh > 0, "%s: bad args (n, IH, IW, oh <= 0)", who);
    BC_CHECK_ARG(IH <= BC_EDIT_MAX_DIM && IW <= BC_EDIT_MAX_DIM && oh <= BC_EDIT_MAX_DIM,
                 "%s: %d x %d -> height %d exceeds the limit of %d a side", who, IH, IW, oh, BC_EDIT_MAX_DIM);
    BC_CHECK_ARG(r0 >= 0 && r0 <= BC_EDIT_MAX_DIM, "%s: r0 = %d (the source row of row 0 of `in`: 0 .. %d)", who, r0, BC_EDIT_MAX_DIM);
    BC_CHECK_ARG(y0 >= 0 && ch > 0 && (long long)y0 + ch <= oh, "%s: window rows [%d, %d + %d) leave the resized frame of %d rows", who, y0, y0, ch, oh);
    BC_CHECK_ARG(xin0 >= 0 && cw > 0 && (long long)xin0 + cw <= IW, "%s: window columns [%d, %d + %d) leave the input of %d columns", who, xin0, xin0, cw,
                 IW);
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int chunks;
    if (out_u8) {
        const long long total = (long long)ch * cw * 3;
        if (rs_chunks(who, n, total, chunks)) return 1;
        hipLaunchKernelGGL(rs_vertical_u8_kernel, dim3(n * chunks), dim3(RS_THREADS), 0, s, in, IH, IW, r0, xin0, bounds_y, coeffs_y, ksize, y0, cw,
                           (int)total, chunks, out_u8);
    } else {
        BC_CHECK_ARG(((reinterpret_cast<uintptr_t>(out_f32) | reinterpret_cast<uintptr_t>(lut)) & 3) == 0,
                     "%s: out_f32 and lut must be aligned to 4 bytes", who);
        BC_CHECK_ARG(PH >= ch && PW >= cw && PH <= BC_EDIT_MAX_DIM && PW <= BC_EDIT_MAX_DIM,
                     "%s: a frame of %d x %d must hold the window of %d x %d within the limit of %d a side", who, PH, PW, ch, cw, BC_EDIT_MAX_DIM);
        const long long total = 3ll * PH * PW;
        if (rs_chunks(who, n, total, chunks)) return 1;
        hipLaunchKernelGGL(rs_vertical_f32_kernel, dim3(n * chunks), dim3(RS_THREADS), 0, s, in, IH, IW, r0, xin0, bounds_y, coeffs_y, ksize, y0, ch,
                           cw, lut, PH, PW, (int)total, chunks, out_f32);
    }
    BC_CHECK_LAUNCH();
    return 0;
}
