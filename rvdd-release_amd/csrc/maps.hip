// The map primitives of the nets, all HBM-bound: bilinear x2 upsample and 2x2 max-pool of NHWC48 maps, NCHW <-> NHWC, the
// final 1x1 conv 48 -> 3, and the fp64 loss reduction.  Compiled with -ffp-contract=off: the 1x1 conv and the loss sums are
// kept one operation at a time (the upsample's fused multiply-adds are written out as such).
#include "rvdd_internal.h"

namespace {

// nn.Upsample(scale_factor=2, mode="bilinear"[, align_corners]) on NHWC48,
// 12 threads per output pixel.  ATen upsample_bilinear2d source index:
//   align_corners=False: src = max(0.5*(dst+0.5)-0.5, 0);  True: src = dst*(in-1)/(out-1)
// grid = (ceil(Wout/16), Hout, B), 192 threads = 16 output pixels of one row x 12 float4 chunks: the row terms
// (source rows, vertical weights) depend on blockIdx only and stay in scalar registers, no 64-bit divisions
__global__ __launch_bounds__(192) void upsample2x_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int h,
                                                         int w, int Hout, int Wout, int oy, int ox, int align) {
    const int p = threadIdx.x / 12, c4 = threadIdx.x - p * 12;
    const int X = blockIdx.x * 16 + p, Y = blockIdx.y, b = blockIdx.z;
    if (X >= Wout) return;
    const int y = Y - oy, x = X - ox;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)y < (unsigned)(2 * h) && (unsigned)x < (unsigned)(2 * w)) {
        float py, px;
        if (align) {
            const float sy = 2 * h > 1 ? (float)(h - 1) / (float)(2 * h - 1) : 0.f;
            const float sx = 2 * w > 1 ? (float)(w - 1) / (float)(2 * w - 1) : 0.f;
            py = sy * (float)y;
            px = sx * (float)x;
        } else {
            py = fmaxf(0.5f * ((float)y + 0.5f) - 0.5f, 0.f);
            px = fmaxf(0.5f * ((float)x + 0.5f) - 0.5f, 0.f);
        }
        const int y0 = (int)py, x0 = (int)px;
        const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
        const float ly1 = py - (float)y0, lx1 = px - (float)x0;
        const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
        const f32x4* s = reinterpret_cast<const f32x4*>(in) + (size_t)b * h * w * 12 + c4;
        const f32x4 v00 = s[(y0 * w + x0) * 12], v01 = s[(y0 * w + x1) * 12];
        const f32x4 v10 = s[(y1 * w + x0) * 12], v11 = s[(y1 * w + x1) * 12];
        // vertical pass, then horizontal, each "a * wa, then one fused multiply-add": the expression of the fused
        // upsample in wino3x3.hip (`interp`), so that the two paths produce the same bits
        auto fma4 = [](f32x4 a, float s, f32x4 c) { return __builtin_elementwise_fma(a, f32x4{s, s, s, s}, c); };
        const f32x4 c0 = fma4(v10, ly1, v00 * ly0), c1 = fma4(v11, ly1, v01 * ly0);
        v = fma4(c1, lx1, c0 * lx0);
    }
    reinterpret_cast<f32x4*>(out)[(((size_t)b * Hout + Y) * Wout + X) * 12 + c4] = v;
}

__global__ void maxpool2_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int H,
                                int W) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t pix = gid / 12;
    const int c4 = gid - pix * 12;
    if (pix >= (size_t)B * Ho * Wo) return;
    const int x = pix % Wo;
    const int y = (pix / Wo) % Ho;
    const int b = pix / ((size_t)Wo * Ho);
    const f32x4* s = reinterpret_cast<const f32x4*>(in) + (size_t)b * H * W * 12 + c4;
    const f32x4 a = s[((size_t)(2 * y) * W + 2 * x) * 12], bb = s[((size_t)(2 * y) * W + 2 * x + 1) * 12];
    const f32x4 c = s[((size_t)(2 * y + 1) * W + 2 * x) * 12],
                d = s[((size_t)(2 * y + 1) * W + 2 * x + 1) * 12];
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = fmaxf(fmaxf(a[r], bb[r]), fmaxf(c[r], d[r]));
    reinterpret_cast<f32x4*>(out)[gid] = v;
}

__global__ void nchw_to_nhwc_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int C,
                                    int H, int W, int Cpad) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B*H*W*Cpad
    const size_t hw = (size_t)H * W;
    if (idx >= (size_t)B * hw * Cpad) return;
    const int c = idx % Cpad;
    const size_t p = (idx / Cpad) % hw;
    const int b = idx / ((size_t)Cpad * hw);
    out[idx] = c < C ? in[((size_t)b * C + c) * hw + p] : 0.f;
}

__global__ void nhwc_to_nchw_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int C,
                                    int H, int W, int Cpad) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // over B*C*H*W
    const size_t hw = (size_t)H * W;
    if (idx >= (size_t)B * C * hw) return;
    const size_t p = idx % hw;
    const int c = (idx / hw) % C;
    const int b = idx / ((size_t)C * hw);
    out[idx] = in[((size_t)b * hw + p) * Cpad + c];
}

// PostConvs[1]: 1x1 conv 48 -> 3 (networks/unet.py:713-720)
__global__ void conv1x1_out_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                   const float* __restrict__ bias, float* __restrict__ out_nchw,
                                   float* __restrict__ out_nhwc4, int B, int H, int W) {
    __shared__ float ws[3 * 48 + 3];
    if (threadIdx.x < 147) ws[threadIdx.x] = threadIdx.x < 144 ? w[threadIdx.x] : bias[threadIdx.x - 144];
    __syncthreads();
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t hw = (size_t)H * W;
    if (idx >= (size_t)B * hw) return;
    const f32x4* f = reinterpret_cast<const f32x4*>(feat) + idx * 12;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const f32x4 v = f[q];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o0 += v[r] * ws[4 * q + r];
            o1 += v[r] * ws[48 + 4 * q + r];
            o2 += v[r] * ws[96 + 4 * q + r];
        }
    }
    o0 += ws[144];
    o1 += ws[145];
    o2 += ws[146];
    const size_t b = idx / hw, p = idx - b * hw;
    if (out_nchw) {
        out_nchw[(b * 3 + 0) * hw + p] = o0;
        out_nchw[(b * 3 + 1) * hw + p] = o1;
        out_nchw[(b * 3 + 2) * hw + p] = o2;
    }
    if (out_nhwc4) reinterpret_cast<f32x4*>(out_nhwc4)[idx] = f32x4{o0, o1, o2, 0.f};
}

// sum |a-b| and sum (a-b)^2 (models/recurrent_model.py:512-525, util/util.py:9-20)
__global__ void loss_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                    double* __restrict__ partial) {
    // slice blockIdx.y of a batch (launch_loss_reduce_batch): the same blocks over the same elements as a call of its own
    a += (size_t)blockIdx.y * n;
    b += (size_t)blockIdx.y * n;
    partial += (size_t)blockIdx.y * 2 * gridDim.x;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float d = a[i] - b[i];
        s1 += (double)fabsf(d);
        s2 += (double)d * (double)d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o);
        s2 += __shfl_down(s2, o);
    }
    __shared__ double sh[2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        sh[0][wv] = s1;
        sh[1][wv] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
        partial[2 * blockIdx.x + 1] = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
    }
}
__global__ void loss_final_kernel(const double* __restrict__ partial, int nblk, double* __restrict__ res) {
    partial += (size_t)blockIdx.x * 2 * nblk;      // one block per slice
    res += 2 * blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) {
        s1 += partial[2 * i];
        s2 += partial[2 * i + 1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_down(s1, o);
        s2 += __shfl_down(s2, o);
    }
    if (threadIdx.x == 0) {
        res[0] = s1;
        res[1] = s2;
    }
}

}  // namespace

hipError_t launch_upsample2x(const float* in, float* out, int B, int h, int w, int Hout, int Wout, int oy,
                             int ox, bool align_corners, hipStream_t s) {
    if (!B || !Hout || !Wout) return hipSuccess;
    hipLaunchKernelGGL(upsample2x_kernel, dim3((Wout + 15) / 16, Hout, B), dim3(192), 0, s, in, out, B, h, w, Hout, Wout,
                       oy, ox, align_corners ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_maxpool2(const float* in, float* out, int B, int H, int W, hipStream_t s) {
    const size_t n = (size_t)B * (H / 2) * (W / 2) * 12;
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(maxpool2_kernel, dim3(nblocks(n, 192)), dim3(192), 0, s, in, out, B, H, W);
    return hipGetLastError();
}

hipError_t launch_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, int Cpad,
                               hipStream_t s) {
    const size_t n = (size_t)B * H * W * Cpad;
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, in, out, B, C, H, W, Cpad);
    return hipGetLastError();
}

hipError_t launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, int Cpad,
                               hipStream_t s) {
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, in, out, B, C, H, W, Cpad);
    return hipGetLastError();
}

hipError_t launch_conv1x1_out(const float* feat, const float* w3x48, const float* b3, float* out_nchw,
                              float* out_nhwc4, int B, int H, int W, hipStream_t s) {
    const size_t n = (size_t)B * H * W;
    hipLaunchKernelGGL(conv1x1_out_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, feat, w3x48, b3, out_nchw,
                       out_nhwc4, B, H, W);
    return hipGetLastError();
}

hipError_t launch_loss_reduce_batch(const float* a, const float* b, int nslices, int64_t n, double* partial, int nblk,
                                    double* result2, hipStream_t s) {
    if (nslices <= 0) return hipSuccess;
    hipLaunchKernelGGL(loss_partial_kernel, dim3(nblk, nslices), dim3(256), 0, s, a, b, n, partial);
    hipLaunchKernelGGL(loss_final_kernel, dim3(nslices), dim3(64), 0, s, partial, nblk, result2);
    return hipGetLastError();
}
