// Device code of the bicubic backward warp shared by warp.hip (the stand-alone warps) and netin.hip (the warps inside the
// network input): the x2 flow upsample, the taps of a pixel, and the 3-channel gather and sum.  File-local in every
// translation unit that includes it.
#pragma once
#include "rvdd_internal.h"

namespace {

// Cubic-convolution weights, A = -0.75 (ATen UpSample.h get_cubic_upsample_coefficients).
__device__ __forceinline__ void cubic_w(float t, float w[4]) {
    const float A = -0.75f;
    float x = t + 1.f;
    w[0] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
    x = t;
    w[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    x = 1.f - t;
    w[2] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
    x = 2.f - t;
    w[3] = ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A;
}

// full-resolution flow at (y,x) from the raw-resolution one:
// F.interpolate(x2, bilinear, align_corners=True) * 2  (util/flow_utils.py:159-174,
// models/recurrent_model.py:128-129)
struct FlowQ {      // the four raw-resolution flow vectors around a pixel and their bilinear weights
    float f[2][4];
    float ly0, ly1, lx0, lx1;
};
__device__ __forceinline__ void flow_fetch(const float* __restrict__ fr, int h, int w, int H, int W, int y, int x, FlowQ& q) {
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float py = sy * (float)y, px = sx * (float)x;
    const int y0 = (int)py, x0 = (int)px;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    q.ly1 = py - (float)y0;
    q.lx1 = px - (float)x0;
    q.ly0 = 1.f - q.ly1;
    q.lx0 = 1.f - q.lx1;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* f = fr + (size_t)c * h * w;
        q.f[c][0] = f[y0 * w + x0];
        q.f[c][1] = f[y0 * w + x1];
        q.f[c][2] = f[y1 * w + x0];
        q.f[c][3] = f[y1 * w + x1];
    }
}
__device__ __forceinline__ void flow_combine(const FlowQ& q, float& fx, float& fy) {
    fx = (q.ly0 * (q.lx0 * q.f[0][0] + q.lx1 * q.f[0][1]) + q.ly1 * (q.lx0 * q.f[0][2] + q.lx1 * q.f[0][3])) * 2.f;
    fy = (q.ly0 * (q.lx0 * q.f[1][0] + q.lx1 * q.f[1][1]) + q.ly1 * (q.lx0 * q.f[1][2] + q.lx1 * q.f[1][3])) * 2.f;
}
__device__ __forceinline__ void flow_at(const float* __restrict__ fr, int h, int w, int H, int W, int y,
                                        int x, float& fx, float& fy) {
    FlowQ q;
    flow_fetch(fr, h, w, H, W, y, x, q);
    flow_combine(q, fx, fy);
}

// util/flow_utils.py:90-99 + ATen grid_sampler (bicubic, border, align_corners=True)
struct Taps {
    int xi[4], yi[4];
    float wx[4], wy[4];
};
__device__ __forceinline__ void make_taps(float fx, float fy, int x, int y, int H, int W, Taps& t) {
    const float vx = (float)x + fx, vy = (float)y + fy;
    const float gx = 2.0f * vx / (float)(W - 1) - 1.0f;
    const float gy = 2.0f * vy / (float)(H - 1) - 1.0f;
    const float ix = ((gx + 1.f) / 2.f) * (float)(W - 1);
    const float iy = ((gy + 1.f) / 2.f) * (float)(H - 1);
    const float x0 = floorf(ix), y0 = floorf(iy);
    cubic_w(ix - x0, t.wx);
    cubic_w(iy - y0, t.wy);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // clip_coordinates on the float tap coordinate, then the integer cast
        float cx = x0 - 1.f + (float)i, cy = y0 - 1.f + (float)i;
        cx = fminf((float)(W - 1), fmaxf(cx, 0.f));
        cy = fminf((float)(H - 1), fmaxf(cy, 0.f));
        t.xi[i] = (int)cx;
        t.yi[i] = (int)cy;
    }
}

// The 16 taps of a pixel of an NHWC4 frame loaded TOGETHER, then summed in warp3_kernel's order (netin.hip puts the
// demosaic's arithmetic between the two)
__device__ __forceinline__ void warp3_gather(const f32x4* __restrict__ s, const Taps& t, int W, f32x4 (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[4 * j + i] = s[(size_t)t.yi[j] * W + t.xi[i]];
}
__device__ __forceinline__ f32x4 warp3_sum(const Taps& t, const f32x4 (&v)[16]) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) row = row + v[4 * j + i] * t.wx[i];
        acc = acc + row * t.wy[j];
    }
    return acc;
}

}  // namespace
