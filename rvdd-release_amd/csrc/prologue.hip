// The prologue of the composed first layer (net_convunet.hip compose_pre_enc0): the fix of its border ring, the second pass
// of EncoderConvs[0][0] over an all-zero source, and the amax words of maps that no kernel of a frame-step wrote.  Compiled
// with -ffp-contract=off: the chains are written with fmaf where the conv fuses, and nothing else may be contracted.
#include "rvdd_internal.h"

namespace {

// max |x| per sequence of a dense map [B][n] (rvdd_internal.h: amax words of the maps that no kernel of a frame-step wrote --
// caller-supplied network inputs and features, a recurrent state handed in through rvdd_set_state)
// (`up`: binades added to the maximum, for a map that stands for something up to 2^up times larger)
__global__ __launch_bounds__(256) void amax_reduce_kernel(const float* __restrict__ map, int64_t n, unsigned* __restrict__ words, int up) {
    __shared__ unsigned red[4];
    const int b = blockIdx.y;
    const f32x4* p = reinterpret_cast<const f32x4*>(map + (size_t)b * n);
    const int64_t n4 = n >> 2;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) m = absmax4(m, p[i]);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) m = fmaxf(m, fabsf(map[(size_t)b * n + 4 * n4 + threadIdx.x]));
    unsigned bits = __float_as_uint(m);
    const unsigned e = (bits >> 23) & 0xffu;
    if (up && e >= 1 && e + up < 254) bits += (unsigned)up << 23;
    amax_commit_block(words, b, blockIdx.x, __uint_as_float(bits), red);
}

// The border ring of the composed first layer (net_convunet.hip compose_pre_enc0).  The composition treats the preprocessing
// layer's output y as if it existed outside the image (b1 + partial windows of the zero-extended input); the reference pads it
// with ZEROS (networks/unet.py:742-743, padding=1 on both convs).  For a border pixel p the composed sum therefore carries
// sum over the taps d with q = p + d - 1 outside the image of W2[d] y~(q), y~(q) = b1 + sum over taps e with q + e - 1 inside of
// W1[e] x(q + e - 1): subtracted here.
// netin NHWC16, w1 [9][16][48 m], w2 [9][48 m][48 o], part NHWC48.
// One 256-thread block per RUN of up to 16 consecutive ring pixels of one side of one sequence (the top and bottom rows whole,
// corners included; the left and right columns between them), wave = a share of the run, lane = channel.  (One 64-thread block
// per ring pixel -- 32 000 of them at 720p B = 8 -- formed every outside y~(q) again in each of the up to three pixels that touch
// it, one dependent round trip after another: 83 us per frame-step for 4 000 pixels per sequence.)  The run's outside positions
// -- the 18 next to it in the row or column beyond the edge, and beside a corner the two in the column beyond the side edge --
// are formed ONCE into LDS, each by the chain of the one-pixel kernel (b1, taps e ascending, channels c ascending); then every
// pixel's corr by its chain (outside taps d ascending, m = 0..47) and the subtraction last: the same bits.  The four pixels of a
// wave share each w2 row they need (a 192-B coalesced load) and run their chains side by side.
constexpr int kFixRun = 16;                  // ring pixels per block
constexpr int kFixSlots = kFixRun + 2 + 4;   // outside positions of a run: the line beyond the edge, two per corner
__global__ __launch_bounds__(256) void pre_border_fix_kernel(const float* __restrict__ netin, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            float* __restrict__ part, int H, int W) {
    __shared__ float ys[kFixSlots][48];
    const int b = blockIdx.y, t = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int nxr = (W + kFixRun - 1) / kFixRun, nyr = (H - 2 + kFixRun - 1) / kFixRun;
    // the run: `horiz` along row py0 from column px0, else along column px0 from row py0; n pixels; (oy, ox) the line beyond the edge
    int i = blockIdx.x, py0, px0, n;
    const bool horiz = i < 2 * nxr;
    if (horiz) {
        py0 = i < nxr ? 0 : H - 1;
        px0 = (i < nxr ? i : i - nxr) * kFixRun;
        n = min(kFixRun, W - px0);
    } else {
        i -= 2 * nxr;
        px0 = i < nyr ? 0 : W - 1;
        py0 = 1 + (i < nyr ? i : i - nyr) * kFixRun;
        n = min(kFixRun, H - 1 - py0);
    }
    const int oy = py0 == 0 ? -1 : H, ox = px0 == 0 ? -1 : W;      // (horiz: oy; else: ox)
    const int iny = py0 == 0 ? 1 : H - 2;                          // horiz: the row next to the run's, towards the inside
    const bool c_lo = horiz && px0 == 0, c_hi = horiz && px0 + n == W;
    const float* x = netin + (size_t)b * H * W * kNetInC;
    // ---- y~(q) of every outside position the run touches: slots 0 .. n + 1 along the line beyond the edge, kFixRun + 2 .. + 5
    // the positions (py0, -1), (iny, -1), (py0, W), (iny, W) beside the corners
#pragma unroll 1
    for (int sl = g; sl < kFixSlots; sl += 4) {
        int qy, qx;
        if (sl < kFixRun + 2) {
            if (sl > n + 1) continue;
            qy = horiz ? oy : py0 - 1 + sl;
            qx = horiz ? px0 - 1 + sl : ox;
        } else {
            const int k = sl - (kFixRun + 2);
            if (!(k < 2 ? c_lo : c_hi)) continue;
            qy = (k & 1) ? iny : py0;
            qx = k < 2 ? -1 : W;
        }
        // the taps e whose pixel q + e - 1 lies inside: at most three (q is one step outside in a row or in a column), ascending;
        // their loads all together, then the chain
        int ek[3];
        {
            int e = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                while (e < 9 && ((unsigned)(qy + e / 3 - 1) >= (unsigned)H || (unsigned)(qx + e % 3 - 1) >= (unsigned)W)) ++e;
                ek[k] = e;
                e = e < 9 ? e + 1 : 9;
            }
        }
        if (t < 48) {
            float xv[3][kNetInC], wv[3][kNetInC];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (ek[k] >= 9) continue;
                // (the same pixel for every lane: a scalar offset, the 16 channels from the scalar cache)
                const int off = __builtin_amdgcn_readfirstlane(((qy + ek[k] / 3 - 1) * W + (qx + ek[k] % 3 - 1)) * kNetInC);
#pragma unroll
                for (int c = 0; c < kNetInC; ++c) xv[k][c] = x[off + c];
#pragma unroll
                for (int c = 0; c < kNetInC; ++c) wv[k][c] = w1[(ek[k] * kNetInC + c) * 48 + t];
            }
            float y = b1[t];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (ek[k] >= 9) continue;
#pragma unroll
                for (int c = 0; c < kNetInC; ++c) y = fmaf(wv[k][c], xv[k][c], y);
            }
            ys[sl][t] = y;
        }
    }
    __syncthreads();
    // ---- pixels 4 g .. 4 g + 3 of the run
    if (t >= 48) return;
    int py[4], px[4];
    bool live[4];
    float corr[4] = {0.f, 0.f, 0.f, 0.f}, pv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 4 * g + k;
        live[k] = j < n;
        py[k] = horiz ? py0 : py0 + j;
        px[k] = horiz ? px0 + j : px0;
        pv[k] = live[k] ? part[((size_t)b * H * W + (size_t)py[k] * W + px[k]) * kF + t] : 0.f;      // (on its way under the chains)
    }
#pragma unroll 1
    for (int d = 0; d < 9; ++d) {
        int slot[4];
        bool any = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qy = py[k] + d / 3 - 1, qx = px[k] + d % 3 - 1;
            slot[k] = -1;
            if (!live[k] || ((unsigned)qy < (unsigned)H && (unsigned)qx < (unsigned)W)) continue;      // q inside: the composition is right
            if (!horiz) slot[k] = qy - (py0 - 1);
            else if (qy == oy) slot[k] = qx - (px0 - 1);
            else slot[k] = kFixRun + 2 + (qx < 0 ? 0 : 2) + (qy == py0 ? 0 : 1);
            any = true;
        }
        if (!any) continue;
        const float* wd = w2 + (size_t)d * 48 * 48 + t;
        float wv[48];
#pragma unroll
        for (int m = 0; m < 48; ++m) wv[m] = wd[m * 48];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (slot[k] < 0) continue;
#pragma unroll
            for (int m = 0; m < 48; ++m) corr[k] = fmaf(wv[m], ys[slot[k]][m], corr[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (live[k]) part[((size_t)b * H * W + (size_t)py[k] * W + px[k]) * kF + t] = pv[k] - corr[k];
}

// The second pass of EncoderConvs[0][0] on the first step of a video.  Its source, the warped recurrent features, is all +0
// there (a bicubic gather of +0 sums +0 products from +0), so the pass of conv3x3h_kernel<48, EPI_RELU, ACC_IN> computes
// fma(acc, ws, part) with acc = +0 (an MFMA chain from +0 over +-0 products) and ws finite: part + 0 -- which is part, with -0
// made +0 -- then its one-instruction ReLU, and commits max |out| per sequence to the layer's amax words (every reader takes the
// maximum over a sequence's lines: which line a workgroup's maximum lands on is free).  The same here without the 1.4 GB of
// zeros read: 16-B loads and stores, grid (blocks, B), grid-stride inside a sequence.
__global__ __launch_bounds__(256) void relu_part_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t n4,
                                                        unsigned* __restrict__ words) {
    __shared__ unsigned red[4];
    const int b = blockIdx.y;
    const f32x4* p = reinterpret_cast<const f32x4*>(part) + (size_t)b * n4;
    f32x4* o = reinterpret_cast<f32x4*>(out) + (size_t)b * n4;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        f32x4 x = p[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = __builtin_amdgcn_fmed3f(x[e] + 0.0f, 0.f, __builtin_inff());
        o[i] = x;
        m = absmax4(m, x);
    }
    if (words) amax_commit_block(words, b, blockIdx.x, m, red);
}

}  // namespace

hipError_t launch_amax_reduce(const float* map, int B, int64_t hw_c, unsigned* words, hipStream_t s, int up) {
    if (B <= 0 || hw_c <= 0) return hipSuccess;
    if ((hw_c & 3) && B > 1) return hipErrorInvalidValue;      // 16-B loads per sequence
    int nblk = (int)((hw_c / 4 + 256 * 8 - 1) / (256 * 8));
    nblk = nblk < 1 ? 1 : (nblk > 128 ? 128 : nblk);
    hipLaunchKernelGGL(amax_reduce_kernel, dim3(nblk, B), dim3(256), 0, s, map, hw_c, words, up);
    return hipGetLastError();
}

hipError_t launch_pre_border_fix(const float* netin, const float* w1, const float* b1, const float* w2, float* part, int B, int H, int W,
                                 hipStream_t s) {
    if (B <= 0 || H < 2 || W < 2) return hipSuccess;
    const int nxr = (W + kFixRun - 1) / kFixRun, nyr = (H - 2 + kFixRun - 1) / kFixRun;
    hipLaunchKernelGGL(pre_border_fix_kernel, dim3(2 * nxr + 2 * nyr, B), dim3(256), 0, s, netin, w1, b1, w2, part, H, W);
    return hipGetLastError();
}

hipError_t launch_relu_part(const float* part, float* out, int B, int64_t n, unsigned* words, hipStream_t s) {
    if (B <= 0 || n <= 0) return hipSuccess;
    if (n & 3) return hipErrorInvalidValue;
    int64_t nblk = (n / 4 + 256 * 4 - 1) / (256 * 4);        // four 16-B loads and stores per thread, at most 2048 blocks per sequence
    nblk = nblk < 1 ? 1 : (nblk > 2048 ? 2048 : nblk);
    hipLaunchKernelGGL(relu_part_kernel, dim3((unsigned)nblk, B), dim3(256), 0, s, part, out, n / 4, words);
    return hipGetLastError();
}
