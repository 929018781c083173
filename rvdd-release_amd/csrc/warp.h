// Device code of the bicubic backward warp shared by warp.hip (the stand-alone warps) and netin.hip (the warps inside the
// network input): the x2 flow upsample, the taps of a pixel, the 3-channel gather and sum, and the gather of the two
// 48-channel feature warps by 2 x 2 quads.  File-local in every translation unit that includes it.
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

// ---- the gather of the 48-channel feature warps (warp48_kernel, warp48_proj_kernel) ---------------------------------------------
// A workgroup of 192 threads owns 32 x `rows` pixels (warp48_kernel 2: 16 quads of 2 x 2 pixels x 12 float4 channel pieces;
// warp48_proj_kernel 1: 16 pairs).  The taps of its pixels are formed once by the first 32 x rows threads (rows = 2: one full
// wave) and shared through LDS: s_i = xi[4], yi[4] * W and s_w = wx[4], wy[4] of pixel 32 * row + column.
struct PieceTaps {      // a pixel's taps as a gathering lane holds them; yi is premultiplied by W
    int xi[4], yi[4];
    float wx[4], wy[4];
};
__device__ __forceinline__ void warp48_make_taps(const float* __restrict__ fr, int H, int W, int x0, int y0, int rows, int (*s_i)[8],
                                                 float (*s_w)[8]) {
    if (threadIdx.x >= 32 * rows) return;
    const int x = x0 + (threadIdx.x & 31), y = y0 + (threadIdx.x >> 5);
    if (x >= W || y >= H) return;
    float fx, fy;
    flow_at(fr, H / 2, W / 2, H, W, y, x, fx, fy);
    Taps t;
    make_taps(fx, fy, x, y, H, W, t);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s_i[threadIdx.x][k] = t.xi[k];
        s_i[threadIdx.x][4 + k] = t.yi[k] * W;
        s_w[threadIdx.x][k] = t.wx[k];
        s_w[threadIdx.x][4 + k] = t.wy[k];
    }
}
__device__ __forceinline__ void warp48_read_taps(const int (*s_i)[8], const float (*s_w)[8], int p, PieceTaps& t) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        t.xi[k] = s_i[p][k];
        t.yi[k] = s_i[p][4 + k];
        t.wx[k] = s_w[p][k];
        t.wy[k] = s_w[p][4 + k];
    }
}
// the footprints of two horizontally adjacent pixels are the same four rows and the columns shifted by one (on the clamped
// indices, so the frame's border needs no case of its own)
__device__ __forceinline__ bool warp48_lined_up(const PieceTaps& a, const PieceTaps& b) {
    return b.yi[0] == a.yi[0] && b.yi[1] == a.yi[1] && b.yi[2] == a.yi[2] && b.yi[3] == a.yi[3] && b.xi[0] == a.xi[1] &&
           b.xi[1] == a.xi[2] && b.xi[2] == a.xi[3];
}
// one tap row of a lined-up pair: five values serve both pixels
__device__ __forceinline__ void warp48_row2(const f32x4 (&v)[5], const PieceTaps& a, const PieceTaps& b, int j, f32x4& acca,
                                            f32x4& accb) {
    f32x4 ra = {0.f, 0.f, 0.f, 0.f}, rb = {0.f, 0.f, 0.f, 0.f};
    ra = ra + v[0] * a.wx[0]; ra = ra + v[1] * a.wx[1]; ra = ra + v[2] * a.wx[2]; ra = ra + v[3] * a.wx[3];
    rb = rb + v[1] * b.wx[0]; rb = rb + v[2] * b.wx[1]; rb = rb + v[3] * b.wx[2]; rb = rb + v[4] * b.wx[3];
    acca = acca + ra * a.wy[j];
    accb = accb + rb * b.wy[j];
}
__device__ __forceinline__ f32x4 warp48_single(const f32x4* __restrict__ s, const PieceTaps& t) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) row = row + s[(t.yi[j] + t.xi[i]) * 12] * t.wx[i];
        acc = acc + row * t.wy[j];
    }
    return acc;
}
// row-pair level: 20 loads for a lined-up pair, 2 x 16 otherwise (16 where the right pixel is outside the frame)
__device__ __forceinline__ void warp48_gather_pair(const f32x4* __restrict__ s, const PieceTaps& a, const PieceTaps& b, bool has_b,
                                                   f32x4& acca, f32x4& accb) {
    if (has_b && warp48_lined_up(a, b)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v[5] = {s[(a.yi[j] + a.xi[0]) * 12], s[(a.yi[j] + a.xi[1]) * 12], s[(a.yi[j] + a.xi[2]) * 12],
                                s[(a.yi[j] + a.xi[3]) * 12], s[(a.yi[j] + b.xi[3]) * 12]};
            warp48_row2(v, a, b, j, acca, accb);
        }
    } else {
        acca = warp48_single(s, a);
        if (has_b) accb = warp48_single(s, b);
    }
}
// One 16-byte channel piece of the quad a = (x, y), b = (x+1, y), c = (x, y+1), d = (x+1, y+1): s points at the piece of
// pixel (0, 0) of the sequence, pa is a's pixel in s_i / s_w (b, c, d: pa + 1, pa + 32, pa + 33), acc receives the four sums
// (zero for a pixel outside the frame: has_b, has_c).
//  * Quad level.  Under a smooth flow the four footprints are the same five rows and five columns -- both rows are lined-up
//    pairs, c's rows are a's shifted by one, c has a's columns and d's last column is b's: 25 loads serve the quad (6.25 per
//    pixel) where two lined-up pairs take 40 and four single pixels 64.  Row r of the five is tap row r of a and b and tap row
//    r - 1 of c and d; the rows stream through two buffers, the next one in flight under the sums of this one (all 25 in
//    flight cost 164 registers and three waves per SIMD, and the kernel was slower than the pair form; this way 116 and four).
//  * Otherwise each row takes the row-pair level by itself, and below that the single pixels.  The fallback reads its taps
//    again from LDS (the compiler barrier keeps them out of the registers the quad level lives in).
// Whatever the level, a pixel's sum is row = ((0 + v0 wx0) + v1 wx1) + ..., acc = acc + row wy[j], j ascending: the same
// values, weights and order, the same bits.  pairs_only stops at the row-pair level (option "warp48_pairs").
__device__ __forceinline__ void warp48_gather_quad(const f32x4* __restrict__ s, const int (*s_i)[8], const float (*s_w)[8], int pa,
                                                   bool has_b, bool has_c, bool pairs_only, f32x4 (&acc)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    bool quad = !pairs_only && has_b && has_c;
    int col[5], row[5];
    {
        int xi[4][4], yi[4][4];      // a, b, c, d
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                xi[q][k] = s_i[pa + 32 * (q >> 1) + (q & 1)][k];
                yi[q][k] = s_i[pa + 32 * (q >> 1) + (q & 1)][4 + k];
            }
#pragma unroll
        for (int k = 0; k < 4; ++k) quad = quad && yi[1][k] == yi[0][k] && yi[3][k] == yi[2][k] && xi[2][k] == xi[0][k];
#pragma unroll
        for (int k = 0; k < 3; ++k) quad = quad && xi[1][k] == xi[0][k + 1] && xi[3][k] == xi[2][k + 1] && yi[2][k] == yi[0][k + 1];
        quad = quad && xi[3][3] == xi[1][3];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            col[k] = xi[0][k];
            row[k] = yi[0][k];
        }
        col[4] = xi[1][3];
        row[4] = yi[2][3];
    }
    if (quad) {
        float wx[4][4], wy[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                wx[q][k] = s_w[pa + 32 * (q >> 1) + (q & 1)][k];
                wy[q][k] = s_w[pa + 32 * (q >> 1) + (q & 1)][4 + k];
            }
        f32x4 v[2][5];
#pragma unroll
        for (int k = 0; k < 5; ++k) v[0][k] = s[(row[0] + col[k]) * 12];
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            if (r < 4) {
#pragma unroll
                for (int k = 0; k < 5; ++k) v[(r + 1) & 1][k] = s[(row[r + 1] + col[k]) * 12];
            }
            __builtin_amdgcn_sched_barrier(0);      // the next row's loads stay in front of this row's sums, and no further
            const f32x4 (&u)[5] = v[r & 1];
            if (r < 4) {
                f32x4 ra = {0.f, 0.f, 0.f, 0.f}, rb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ra = ra + u[i] * wx[0][i];
                    rb = rb + u[i + 1] * wx[1][i];
                }
                acc[0] = acc[0] + ra * wy[0][r];
                acc[1] = acc[1] + rb * wy[1][r];
            }
            if (r > 0) {
                f32x4 rc = {0.f, 0.f, 0.f, 0.f}, rd = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    rc = rc + u[i] * wx[2][i];
                    rd = rd + u[i + 1] * wx[3][i];
                }
                acc[2] = acc[2] + rc * wy[2][r - 1];
                acc[3] = acc[3] + rd * wy[3][r - 1];
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        asm volatile("" ::: "memory");
        PieceTaps a, b;
        warp48_read_taps(s_i, s_w, pa, a);
        warp48_read_taps(s_i, s_w, pa + 1, b);
        warp48_gather_pair(s, a, b, has_b, acc[0], acc[1]);
        if (has_c) {
            asm volatile("" ::: "memory");
            warp48_read_taps(s_i, s_w, pa + 32, a);
            warp48_read_taps(s_i, s_w, pa + 33, b);
            warp48_gather_pair(s, a, b, has_b, acc[2], acc[3]);
        }
    }
}

}  // namespace
