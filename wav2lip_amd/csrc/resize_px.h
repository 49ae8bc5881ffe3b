// The device functions of cv::resize(INTER_LINEAR) for CV_8UC3 (OpenCV 4.1.0 modules/imgproc/src/resize.cpp), shared by the resize
// kernels (resize.hip) and the detector's reduced-resolution pack (detect.hip: w2l_s3fd_pack_rows_scaled), so that both compute a
// destination pixel with the same operations: byte-equal results.
#pragma once
#include "w2l_common.h"

namespace w2l {

struct AxisTap {
    int s0, s1;     // source indices
    int a0, a1;     // 11-bit coefficients
};

// horizontal convention (coefficient zeroed at the clamped edges); vertical = the same without the edge zeroing, rows clipped
__device__ __forceinline__ AxisTap axis_tap(int d, int ssize, int dsize, bool horizontal) {
    const double inv = __ddiv_rn((double)dsize, (double)ssize);
    const double scale = __ddiv_rn(1.0, inv);
    float f = (float)__dsub_rn(__dmul_rn((double)d + 0.5, scale), 0.5);
    int s = (int)floorf(f);
    f = __fsub_rn(f, (float)s);
    AxisTap t;
    if (horizontal) {
        if (s < 0) { s = 0; f = 0.f; }
        if (s >= ssize - 1) { s = ssize - 1; f = 0.f; }
        t.s0 = s;
        t.s1 = min(s + 1, ssize - 1);
    } else {
        t.s0 = min(max(s, 0), ssize - 1);
        t.s1 = min(max(s + 1, 0), ssize - 1);
    }
    t.a1 = (int)rintf(__fmul_rn(f, 2048.f));
    t.a0 = (int)rintf(__fmul_rn(__fsub_rn(1.f, f), 2048.f));
    return t;
}

// the bilinear path of resize_px for taps already computed: r0 / r1 = the two source lines of the vertical tap
__device__ __forceinline__ void lerp_px(const uint8_t* __restrict__ r0, const uint8_t* __restrict__ r1, const AxisTap tx,
                                        const AxisTap ty, uint8_t out[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int h0 = (int)r0[tx.s0 * 3 + c] * tx.a0 + (int)r0[tx.s1 * 3 + c] * tx.a1;
        const int h1 = (int)r1[tx.s0 * 3 + c] * tx.a0 + (int)r1[tx.s1 * 3 + c] * tx.a1;
        int v = (((ty.a0 * (h0 >> 4)) >> 16) + ((ty.a1 * (h1 >> 4)) >> 16) + 2) >> 2;
        out[c] = (uint8_t)min(max(v, 0), 255);
    }
}

// true when resize_px takes one of its two tap-free branches (the equal-size copy, the exact 2x INTER_AREA average)
__device__ __forceinline__ bool resize_is_direct(int Hs, int Ws, int h, int w) {
    return (Hs == h && Ws == w) || (Hs == 2 * h && Ws == 2 * w);
}

// src: pointer to pixel (0,0) of the source region, row stride in bytes; Hs x Ws -> pixel (dx,dy) of an h x w result
__device__ __forceinline__ void resize_px(const uint8_t* __restrict__ src, long long row_stride, int Hs, int Ws, int dx,
                                          int dy, int w, int h, uint8_t out[3]) {
    if (Hs == h && Ws == w) {
        const uint8_t* p = src + dy * row_stride + dx * 3;
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
        return;
    }
    if (Hs == 2 * h && Ws == 2 * w) {
        const uint8_t* p0 = src + (2 * dy) * row_stride + (2 * dx) * 3;
        const uint8_t* p1 = p0 + row_stride;
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = (uint8_t)(((int)p0[c] + p0[3 + c] + p1[c] + p1[3 + c] + 2) >> 2);
        return;
    }
    const AxisTap tx = axis_tap(dx, Ws, w, true);
    const AxisTap ty = axis_tap(dy, Hs, h, false);
    lerp_px(src + ty.s0 * row_stride, src + ty.s1 * row_stride, tx, ty, out);
}

}  // namespace w2l
