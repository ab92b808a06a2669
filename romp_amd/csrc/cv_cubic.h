// cv_cubic.h -- cv::resize(INTER_CUBIC) of a zero-padded square image in OpenCV's own fixed-point arithmetic, shared by the
// single-frame pre-processing (post.hip) and the crowd-mode crop batch (crowd.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace romp {

// cv::resize(INTER_CUBIC) tables for one destination coordinate, exactly as OpenCV builds them (resize.cpp: the sampling
// position in double, the cubic weights in float with A = -0.75, then 11-bit fixed point with round-half-even).  `fp contract(off)`
// keeps hipcc from fusing a*b+c into an FMA, which OpenCV's scalar code does not do.
__device__ __forceinline__ void cv_cubic_tab(int d, int src, int dst, int& s0, int (&coef)[4]) {
#pragma clang fp contract(off)
    const double scale = 1.0 / ((double)dst / (double)src);
    const double fd = ((double)d + 0.5) * scale - 0.5;
    const float f = (float)fd;
    const int fl = (int)floorf(f);
    const float x = f - (float)fl;
    const float A = -0.75f;
    const float xp = x + 1.f, xm = 1.f - x;
    float c[4];
    c[0] = ((A * xp - 5.f * A) * xp + 8.f * A) * xp - 4.f * A;
    c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    c[2] = ((A + 2.f) * xm - (A + 3.f)) * xm * xm + 1.f;
    c[3] = 1.f - c[0] - c[1] - c[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) coef[k] = min(max((int)rintf(c[k] * 2048.f), -32768), 32767);
    s0 = fl - 1;
}

// Output pixel (ox, oy) of the S x S resize of a side x side square that holds a window of a BGR uint8 frame at (top, left) on
// zero padding (replicated border of the square): the 4x4 taps, horizontal pass to int32, vertical pass, (v + 2^21) >> 22,
// saturate, written as RGB float.  Window pixel (y, x) is frame pixel (y0 + y, x0 + x) at src + (y0 + y) * row_stride + (x0 + x) * 3;
// it exists for ylo <= y < yhi, xlo <= x < xhi (the caller intersects the window with the frame) and is zero elsewhere.
__device__ __forceinline__ void cv_cubic_pixel(const unsigned char* __restrict__ src, size_t row_stride, int y0, int x0, int ylo,
                                               int yhi, int xlo, int xhi, int side, int top, int left, int ox, int oy, int S,
                                               float* __restrict__ dst) {
    int sx, sy, ca[4], cb[4];
    cv_cubic_tab(ox, side, S, sx, ca);
    cv_cubic_tab(oy, side, S, sy, cb);
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int py = min(max(sy + a, 0), side - 1) - top;             // replicated border of the PADDED image
        int row[3] = {0, 0, 0};
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int px = min(max(sx + b, 0), side - 1) - left;
            // branch-free (taps in the zero padding read pixel 0 with weight 0): all 48 byte loads of a thread in flight
            const bool ok = (unsigned)(py - ylo) < (unsigned)(yhi - ylo) && (unsigned)(px - xlo) < (unsigned)(xhi - xlo);
            const unsigned char* p = src + (ok ? (size_t)(y0 + py) * row_stride + (size_t)(x0 + px) * 3 : 0);
            const int wgt = ok ? ca[b] : 0;
            row[0] += wgt * (int)p[2]; row[1] += wgt * (int)p[1]; row[2] += wgt * (int)p[0];       // BGR -> RGB
        }
        acc[0] += row[0] * cb[a]; acc[1] += row[1] * cb[a]; acc[2] += row[2] * cb[a];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = (float)min(max((acc[c] + (1 << 21)) >> 22, 0), 255);
}

}  // namespace romp
