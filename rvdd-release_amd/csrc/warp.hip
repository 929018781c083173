// Bicubic backward warps with the raw-resolution flow (its x2 bilinear upsample fused): 3 channels of an NHWC4 frame, the 48
// feature channels (plain, and with a 48 -> 48 projection on the way out), a generic NCHW warp with a full-resolution flow, and
// the flow upsample alone.  Compiled with -ffp-contract=off: the warp round-trips its coordinates through the [-1,1]
// normalisation in fp32 (util/flow_utils.py:93-94), kept operation for operation as the reference's ATen ops evaluate it.
// The flow, tap and gather arithmetic is in warp.h.
#include "warp.h"

namespace {

__global__ void warp3_kernel(const float* __restrict__ src4, const float* __restrict__ flow_raw,
                             float* __restrict__ dst, int dpstride, int B, int H, int W) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * H * W) return;
    const int x = idx % W;
    const int y = (idx / W) % H;
    const int b = idx / ((size_t)W * H);
    const int h = H / 2, w = W / 2;
    const f32x4* s = reinterpret_cast<const f32x4*>(src4) + (size_t)b * H * W;
    if (!flow_raw) {        // --no_warp: warp_frame returns its input (models/recurrent_model.py:156-158)
        const f32x4 v = s[(size_t)y * W + x];
        float* o = dst + idx * dpstride;
        o[0] = v[0];
        o[1] = v[1];
        o[2] = v[2];
        return;
    }
    float fx, fy;
    flow_at(flow_raw + (size_t)b * 2 * h * w, h, w, H, W, y, x, fx, fy);
    Taps t;
    make_taps(fx, fy, x, y, H, W, t);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f32x4 row = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) row = row + s[(size_t)t.yi[j] * W + t.xi[i]] * t.wx[i];
        acc = acc + row * t.wy[j];
    }
    float* o = dst + idx * dpstride;
    o[0] = acc[0];
    o[1] = acc[1];
    o[2] = acc[2];
}

// grid = (ceil(W/32), ceil(H/2), B), 192 threads = 16 QUADS of 2 x 2 pixels x 12 float4 chunks.
//  * The 16 taps of a pixel (flow upsample, coordinate round trip, cubic weights: ~150 VALU instructions) are
//    computed ONCE per pixel, by the first 64 threads for the 64 pixels, and shared through LDS; computed by each of
//    the 12 lanes of a pixel they cost as much SIMD time as the gather itself.
//  * The gather is bound by the texture-address path (16-B loads per lane, not by HBM: neighbouring pixels re-read
//    the same lines from L1).  Where the flow is smooth the 4x4 footprints of the four pixels of a quad are the same
//    five rows and five columns: 25 loads serve all four instead of 64.  Quads whose footprints do not line up (flow
//    discontinuities, the clamped image border) fall back row by row to the pair form (20 loads for two pixels) and
//    to the plain 16 loads per pixel; the arithmetic of a pixel is the same in all three (warp.h warp48_gather_quad).
//    pairs = 1 (option "warp48_pairs"): never the quad form, the A/B reference.
__global__ __launch_bounds__(192) void warp48_kernel(const float* __restrict__ src,
                                                     const float* __restrict__ flow_raw,
                                                     float* __restrict__ dst, int B, int H, int W, int64_t fbs, int pairs) {
    __shared__ int s_i[64][8];      // xi[4], yi[4] * W
    __shared__ float s_w[64][8];    // wx[4], wy[4]
    const int y = blockIdx.y * 2, b = blockIdx.z, x0 = blockIdx.x * 32;
    warp48_make_taps(flow_raw + (size_t)b * fbs, H, W, x0, y, 2, s_i, s_w);
    __syncthreads();
    const int p = threadIdx.x / 12;
    const int c4 = threadIdx.x - p * 12;
    const int xa = x0 + 2 * p;
    if (xa >= W) return;
    const bool has_b = xa + 1 < W, has_c = y + 1 < H;
    const f32x4* s = reinterpret_cast<const f32x4*>(src) + (size_t)b * H * W * 12 + c4;
    f32x4* o = reinterpret_cast<f32x4*>(dst) + (((size_t)b * H + y) * W + xa) * 12 + c4;
    f32x4 acc[4];
    warp48_gather_quad(s, s_i, s_w, 2 * p, has_b, has_c, pairs != 0, acc);
    o[0] = acc[0];
    if (has_b) o[12] = acc[1];
    if (has_c) {
        o[(size_t)W * 12] = acc[2];
        if (has_b) o[(size_t)W * 12 + 12] = acc[3];
    }
}

// The feature warp with a 48 -> 48 projection of the warped pixel on its way out: dst = W warp(src) + bias.  One row of 32 pixels
// per workgroup, grid = (ceil(W/32), H, B), and warp.h's gather at its row-pair level: the 32 x 2 form with the quad level
// (64 pixels staged, two 16-pixel groups per projecting wave) gave bits that changed from run to run at 720p, B = 8 -- cause
// not found, LABBOOK.md -- so this kernel keeps the geometry it had.  ConvNeXtUnet's first
// encoder block projects cat[y, warped features] 96 -> 48 (networks/new_unet.py:381-382, 85-88); the projection is linear
// in the two maps and the warped features have no other reader, so their half of it rides here and the other half in the
// epilogue of the block that forms y (convnext.hip PROJ) -- the projection kernel and its 4 S of traffic are gone.
// The 32 warped pixels of the workgroup change lanes through LDS (pixel pitch 52 floats: the 16 lanes of a ds_read_b128 group
// on 16 distinct bank quads); waves 0 and 1 then project one 16-pixel group each on the F16 matrix pipe exactly as convnext.hip's
// PROJ epilogue does: per-pixel power of two (the features have no a-priori bound), split into f16 halves, fc1's five-MFMA
// pattern on the three 16-row blocks of 2^s W (frag: net_convnext.hip's half[1] fragments, 9 KiB, copied to LDS once per
// workgroup), one fma back.  (The first form multiplied f32 on v_mfma_f32_16x16x4_f32: 72 per workgroup at 32 cycles each ON the
// vector lanes the gather's FMAs need -- 1 247 us against warp48_kernel's 899.)
typedef _Float16 wp_h8 __attribute__((ext_vector_type(8)));
typedef __fp16 wp_fp16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 wp_h2 __attribute__((ext_vector_type(2)));
typedef unsigned int wp_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void wp_split4(f32x4 x, unsigned (&hi)[2], unsigned (&lo)[2]) {      // convnext.hip split4h
    const wp_fp16x2 h01 = __builtin_amdgcn_cvt_pkrtz(x[0], x[1]);
    const wp_fp16x2 h23 = __builtin_amdgcn_cvt_pkrtz(x[2], x[3]);
    const unsigned u01 = __builtin_bit_cast(unsigned, h01), u23 = __builtin_bit_cast(unsigned, h23);
    float r0, r1, r2, r3;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(u01), "v"(x[0]));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(u01), "v"(x[1]));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r2) : "v"(u23), "v"(x[2]));
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r3) : "v"(u23), "v"(x[3]));
    const wp_h2 l01 = {(_Float16)r0, (_Float16)r1};
    const wp_h2 l23 = {(_Float16)r2, (_Float16)r3};
    hi[0] = u01; hi[1] = u23;
    lo[0] = __builtin_bit_cast(unsigned, l01); lo[1] = __builtin_bit_cast(unsigned, l23);
}
__global__ __launch_bounds__(192, 4) void warp48_proj_kernel(const float* __restrict__ src, const float* __restrict__ flow_raw,
                                                          float* __restrict__ dst, int B, int H, int W, int64_t fbs,
                                                          const float* __restrict__ frag, int inv_e, const float* __restrict__ bias) {
    __shared__ int s_i[32][8];      // xi[4], yi[4] * W
    __shared__ float s_w[32][8];    // wx[4], wy[4]
    __shared__ __attribute__((aligned(16))) float s_t[32][52];
    __shared__ __attribute__((aligned(16))) float s_f[2304];       // the projection's fragments: [m 3][Fa Fb Fc][64 lanes][16 B]
    const int y = blockIdx.y, b = blockIdx.z, x0 = blockIdx.x * 32;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        reinterpret_cast<f32x4*>(s_f)[threadIdx.x + 192 * k] = reinterpret_cast<const f32x4*>(frag)[threadIdx.x + 192 * k];
    warp48_make_taps(flow_raw + (size_t)b * fbs, H, W, x0, y, 1, s_i, s_w);
    __syncthreads();
    const int p = threadIdx.x / 12;
    const int c4 = threadIdx.x - p * 12;
    const int pa = 2 * p, pb = 2 * p + 1, xa = x0 + pa;
    f32x4 acca = {0.f, 0.f, 0.f, 0.f}, accb = {0.f, 0.f, 0.f, 0.f};
    if (xa < W) {
        const bool has_b = xa + 1 < W;
        const f32x4* s = reinterpret_cast<const f32x4*>(src) + (size_t)b * H * W * 12 + c4;
        PieceTaps ta, tb;
        warp48_read_taps(s_i, s_w, pa, ta);
        warp48_read_taps(s_i, s_w, pb, tb);
        warp48_gather_pair(s, ta, tb, has_b, acca, accb);
    }
    *reinterpret_cast<f32x4*>(&s_t[pa][4 * c4]) = acca;
    *reinterpret_cast<f32x4*>(&s_t[pb][4 * c4]) = accb;
    __syncthreads();
    if (wv >= 2) return;
    // ---- waves 0, 1: the 16 pixels of group wv, all 48 output channels
    f32x4 v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = *reinterpret_cast<const f32x4*>(&s_t[16 * wv + lr][16 * j + 4 * g]);
    float mx = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) mx = absmax4(mx, v[j]);
    unsigned mb = __float_as_uint(mx);
    auto s32 = __builtin_amdgcn_permlane32_swap(mb, mb, false, false);
    mb = max(s32[0], s32[1]);
    auto s16 = __builtin_amdgcn_permlane16_swap(mb, mb, false, false);
    mb = max(s16[0], s16[1]);
    const int e = min((int)(mb >> 23) & 0xff, 252);
    const float fwd = __uint_as_float((unsigned)(253 - e) << 23);
    const float back = __uint_as_float((unsigned)min(max(e + 1 + inv_e, 1), 254) << 23);
    unsigned xh[3][2], xl[3][2];
#pragma unroll
    for (int j = 0; j < 3; ++j) wp_split4(v[j] * fwd, xh[j], xl[j]);
    const wp_h8 P1 = __builtin_bit_cast(wp_h8, wp_u32x4{xh[0][0], xh[0][1], xh[1][0], xh[1][1]});
    const wp_h8 P2 = __builtin_bit_cast(wp_h8, wp_u32x4{xl[0][0], xl[0][1], xl[1][0], xl[1][1]});
    const wp_h8 P3 = __builtin_bit_cast(wp_h8, wp_u32x4{xh[2][0], xh[2][1], xh[2][0], xh[2][1]});
    const wp_h8 P4 = __builtin_bit_cast(wp_h8, wp_u32x4{xl[2][0], xl[2][1], 0u, 0u});
    const int x = x0 + 16 * wv + lr;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const wp_h8 fa = __builtin_bit_cast(wp_h8, *reinterpret_cast<const f32x4*>(s_f + (m * 3 + 0) * 256 + lane * 4));
        const wp_h8 fb = __builtin_bit_cast(wp_h8, *reinterpret_cast<const f32x4*>(s_f + (m * 3 + 1) * 256 + lane * 4));
        const wp_h8 fc = __builtin_bit_cast(wp_h8, *reinterpret_cast<const f32x4*>(s_f + (m * 3 + 2) * 256 + lane * 4));
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, P2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fb, P1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fc, P4, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fc, P3, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa, P1, acc, 0, 0, 0);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 16 * m + 4 * g);
        if (x < W) *reinterpret_cast<f32x4*>(dst + (((size_t)b * H + y) * W + x) * kF + 16 * m + 4 * g) = acc * back + bv;
    }
}

__global__ void warp_nchw_kernel(const float* __restrict__ xin, const float* __restrict__ flow,
                                 float* __restrict__ yout, int n, int c, int H, int W) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * H * W) return;
    const int x = idx % W;
    const int y = (idx / W) % H;
    const int b = idx / ((size_t)W * H);
    const size_t hw = (size_t)H * W;
    const float fx = flow[((size_t)b * 2 + 0) * hw + (size_t)y * W + x];
    const float fy = flow[((size_t)b * 2 + 1) * hw + (size_t)y * W + x];
    Taps t;
    make_taps(fx, fy, x, y, H, W, t);
    for (int ch = 0; ch < c; ++ch) {
        const float* s = xin + ((size_t)b * c + ch) * hw;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float row = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) row = row + s[(size_t)t.yi[j] * W + t.xi[i]] * t.wx[i];
            acc = acc + row * t.wy[j];
        }
        yout[((size_t)b * c + ch) * hw + (size_t)y * W + x] = acc;
    }
}

__global__ void upsample_flow_kernel(const float* __restrict__ t, float* __restrict__ out, int nc, int h,
                                     int w, float mul) {
    const int H = 2 * h, W = 2 * w;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)nc * H * W) return;
    const int x = idx % W;
    const int y = (idx / W) % H;
    const int p = idx / ((size_t)W * H);
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f;
    const float sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float py = sy * (float)y, px = sx * (float)x;
    const int y0 = (int)py, x0 = (int)px;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly1 = py - (float)y0, lx1 = px - (float)x0;
    const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
    const float* f = t + (size_t)p * h * w;
    out[idx] = (ly0 * (lx0 * f[y0 * w + x0] + lx1 * f[y0 * w + x1]) +
                ly1 * (lx0 * f[y1 * w + x0] + lx1 * f[y1 * w + x1])) * mul;
}

}  // namespace

hipError_t launch_warp3(const float* src4, const float* flow_raw, float* dst, int dpstride, int B, int H,
                        int W, hipStream_t s) {
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(warp3_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, src4, flow_raw, dst, dpstride, B,
                       H, W);
    return hipGetLastError();
}

hipError_t launch_warp48(const float* src, const float* flow_raw, float* dst, int B, int H, int W,
                         hipStream_t s, int64_t flow_bstride, bool pairs) {
    if (!B || !H || !W) return hipSuccess;
    hipLaunchKernelGGL(warp48_kernel, dim3((W + 31) / 32, (H + 1) / 2, B), dim3(192), 0, s, src, flow_raw, dst, B, H, W,
                       flow_bstride ? flow_bstride : (int64_t)2 * (H / 2) * (W / 2), (int)pairs);
    return hipGetLastError();
}

hipError_t launch_warp48_proj(const float* src, const float* flow_raw, float* dst, int B, int H, int W, const float* frag,
                              int inv_e, const float* bias, hipStream_t s, int64_t flow_bstride) {
    if (!B || !H || !W) return hipSuccess;
    const int64_t fbs = flow_bstride ? flow_bstride : (int64_t)2 * (H / 2) * (W / 2);
    hipLaunchKernelGGL(warp48_proj_kernel, dim3((W + 31) / 32, H, B), dim3(192), 0, s, src, flow_raw, dst, B, H, W, fbs, frag, inv_e, bias);
    return hipGetLastError();
}

hipError_t launch_warp_nchw(const float* x, const float* flow, float* y, int n, int c, int H, int W,
                            hipStream_t s) {
    const size_t np = (size_t)n * H * W;
    if (!np) return hipSuccess;
    hipLaunchKernelGGL(warp_nchw_kernel, dim3(nblocks(np, 256)), dim3(256), 0, s, x, flow, y, n, c, H, W);
    return hipGetLastError();
}

hipError_t launch_upsample_flow(const float* t, float* out, int nc, int h, int w, float mul, hipStream_t s) {
    const size_t n = (size_t)nc * 4 * h * w;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(upsample_flow_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, t, out, nc, h, w, mul);
    return hipGetLastError();
}
