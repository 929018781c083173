// Green imbalance of packed raw frames: the gain of the green sites of CFA row 0 (plane A) relative to those of CFA row 1 (plane B),
// estimated per frame and block of 32 x 32 cells (rvdd_green_estimate), pooled over the frames on the host (rvdd_green_fit,
// noise_fit.hip) and taken out in place as a static map (rvdd_green_apply); the stage rvdd_set_green puts behind rvdd_set_rows in
// rvdd_video_push.  The rule is in include/rvdd.h; the gate, the key and the digit-wise median search are line_noise.h's, which
// rows.hip and cols.hip share.  Compiled -ffp-contract=off like cols.hip: every operation is rounded to f32 on its own, so that e,
// level, state and the written samples are the bits of the NumPy restatement (tests/green_ref.py).  What is this file's own:
//
// Estimate.  One workgroup of 256 threads owns one (frame, block).  The block's cells of plane A and of plane B, each with the one
// row and one column of halo the other side's samples reach into, go to LDS in DN once: two tiles of 33 x 33 floats at a pitch of 33
// words -- ODD, so that the 32 lanes of a cell row fall on 32 banks and the second cell row of a wave starts one bank on.  Whatever
// the pattern, the four neighbours of the sample at block cell (lr, lc) are the 2 x 2 quad at (lr, lc) of the OTHER plane's tile; only
// where the site itself lies in its own tile depends on dx.  A thread owns the cells tid, tid + 256, ... of the block, four a side:
// their keys stay in registers.  The counts (samples and used samples of either side, two 16-bit counts to a register: a side has at
// most 1024) and S come from integer wave sums (DPP) added up over the four waves through LDS.  A block that is skipped ends there,
// uniformly; else the two medians are two runs of line_median over line_group_count, one barrier a round.
//
// Apply.  A pure stream in place after cols_apply_kernel.  A thread forms the gain of its cells from the map's four nearest blocks
// (the map is a few hundred floats: the loads hit the scalar or vector cache); where every gain is zero it leaves after that.  The
// two planes that are not green are read for the gray value alone, and not at all without a gray plane.
#include "../../include/rvdd.h"
#include "line_noise.h"

namespace {

constexpr int kGreenBlock = RVDD_GREEN_BLOCK;
constexpr int kGreenThreads = kLineApplyThreads;                     // both kernels
constexpr int kGreenWaves = kGreenThreads / 64;
constexpr int kGreenKeys = kGreenBlock * kGreenBlock / kGreenThreads;      // cells per thread, and keys per thread and side
constexpr int kGreenTile = kGreenBlock + 1;                          // a tile's rows, columns and pitch in words
static_assert(kGreenBlock == 32 && kGreenKeys == 4, "a cell row of the block is half a wave; two counts of at most 1024 share a register");

// four values -> the two in the middle, added: five compare-exchanges, of which the sum reads v[1] and v[2]
__device__ __forceinline__ float green_middle(float a, float b, float c, float d) {
    cex(a, b);
    cex(c, d);
    cex(a, c);
    cex(b, d);
    cex(b, c);
    return (b + c) * 0.5f;
}

// plane_a: 0 (GBRG, GRBG) or 1 (RGGB, BGGR); plane B is 3 - plane_a; bpf = gh * gw, the blocks of one frame
__global__ void __launch_bounds__(kGreenThreads) green_estimate_kernel(const float* __restrict__ packed, float* __restrict__ e,
                                                                        float* __restrict__ level, unsigned char* __restrict__ state, int hh,
                                                                        int ww, int gw, unsigned bpf, int plane_a, RowsParams P) {
    __shared__ float tile[2][kGreenTile * kGreenTile];               // plane A's, plane B's
    __shared__ unsigned words[2][kGreenWaves][2];
    __shared__ unsigned sums[kGreenWaves][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned blk = blockIdx.x % bpf, img = blockIdx.x / bpf;
    const int r0 = (int)(blk / (unsigned)gw) * kGreenBlock, c0 = (int)(blk % (unsigned)gw) * kGreenBlock;
    const int64_t hw = (int64_t)hh * ww;
    const int oa = plane_a, ob = 1 - plane_a;                        // dx = +1: A's halo column lies to the left; dx = -1: B's does
    const int dx = plane_a ? 1 : -1;
    {   // A's tile starts at (r0, c0 - oa), B's at (r0 - 1, c0 - ob); a cell outside the plane is no sample's neighbour
        const float* pa = packed + ((int64_t)img * 4 + plane_a) * hw;
        const float* pb = packed + ((int64_t)img * 4 + 3 - plane_a) * hw;
        for (int i = tid; i < kGreenTile * kGreenTile; i += kGreenThreads) {
            const int ty = i / kGreenTile, tx = i - ty * kGreenTile;
            const int ra = r0 + ty, ca = c0 - oa + tx, rb = r0 - 1 + ty, cb = c0 - ob + tx;
            tile[0][i] = ra < hh && ca >= 0 && ca < ww ? dn_of(pa[(int64_t)ra * ww + ca], P.top) : 0.0f;
            tile[1][i] = rb >= 0 && rb < hh && cb >= 0 && cb < ww ? dn_of(pb[(int64_t)rb * ww + cb], P.top) : 0.0f;
        }
    }
    __syncthreads();

    unsigned key[2][kGreenKeys];
    unsigned tot = 0, cnt = 0;                                       // side A in the low half, side B in the high half
    int S = 0;                                                       // at most 8 samples of at most 2^16 a thread
#pragma unroll
    for (int q = 0; q < kGreenKeys; ++q) {
        const int cell = tid + q * kGreenThreads, lr = cell >> 5, lc = cell & 31;
        const int r = r0 + lr, c = c0 + lc;
        const bool in = r < hh && c < ww;
        const bool is[2] = {in && r >= 1 && c + dx >= 0 && c + dx < ww, in && r + 1 < hh && c - dx >= 0 && c - dx < ww};
        const int quad = lr * kGreenTile + lc;
        const int site[2] = {quad + oa, quad + kGreenTile + ob};
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const float* nb = tile[1 - side] + quad;
            const float m = green_middle(nb[0], nb[1], nb[kGreenTile], nb[kGreenTile + 1]);
            const unsigned k = is[side] ? line_gate(tile[side][site[side]], m, P) : kLineNoKey;
            key[side][q] = k;
            tot += is[side] ? 1u << (16 * side) : 0u;
            cnt += k != kLineNoKey ? 1u << (16 * side) : 0u;
            S += k != kLineNoKey ? (int)rintf(m) : 0;
        }
    }
    tot = wave_sum_u32(tot);
    cnt = wave_sum_u32(cnt);
    S = (int)wave_sum_u32((unsigned)S);
    if (lane == 0) {
        sums[wave][0] = tot;
        sums[wave][1] = cnt;
        sums[wave][2] = (unsigned)S;
    }
    __syncthreads();
    tot = cnt = 0;
    long long S64 = 0;
#pragma unroll
    for (int w = 0; w < kGreenWaves; ++w) {
        tot += sums[w][0];
        cnt += sums[w][1];
        S64 += (long long)(int)sums[w][2];
    }
    const unsigned tot_a = tot & 0xffffu, tot_b = tot >> 16, cnt_a = cnt & 0xffffu, cnt_b = cnt >> 16;
    const int64_t out = (int64_t)img * bpf + blk;
    if (!(cnt_a > 0 && cnt_b > 0 && 2 * cnt_a >= tot_a && 2 * cnt_b >= tot_b)) {      // uniform
        if (tid == 0) {
            e[out] = 0.0f;
            level[out] = 0.0f;
            state[out] = 0;
        }
        return;
    }
    int phase = 0;
    float med[2];
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const unsigned(&mine)[kGreenKeys] = key[side];
        const LineMedian lm = line_median(
            0u,                                                      // the block's two conditions are judged above
            [&](const auto& t, auto& c) {
                line_group_count<kGreenWaves>(mine, t, words[phase], lane, wave, c);
                phase ^= 1;
            },
            [&](unsigned prefix) {
                const LineAbove a = line_group_above<kGreenWaves>(mine, prefix, words[phase], lane, wave);
                phase ^= 1;                                          // the next side's rounds go on alternating
                return a;
            });
        med[side] = line_midpoint(lm);
    }
    if (tid == 0) {
        e[out] = (med[0] - med[1]) * 0.5f;
        level[out] = (float)((double)S64 / (double)(cnt_a + cnt_b));
        state[out] = 1;
    }
}

template <int NC>
__global__ void __launch_bounds__(kGreenThreads) green_apply_kernel(float* __restrict__ packed, float* __restrict__ gray,
                                                                     const float* __restrict__ map, int gh, int gw, float black, int hh, int ww,
                                                                     unsigned bpf, int plane_a, float top) {
    const unsigned img = blockIdx.x / bpf;
    const int64_t t = (int64_t)(blockIdx.x % bpf) * kGreenThreads + threadIdx.x;      // the thread inside its frame
    const int wq = ww / NC;
    if (t >= (int64_t)hh * wq) return;
    const int x = NC * (int)(t % wq), y = (int)(t / wq);
    constexpr float kInv = 1.0f / kGreenBlock;
    const float fy = fminf(fmaxf(((float)y + 0.5f) * kInv - 0.5f, 0.0f), (float)(gh - 1));
    const int y0 = (int)fy, y1 = min(y0 + 1, gh - 1);
    const float wy = fy - (float)y0;
    const float *m0 = map + (int64_t)y0 * gw, *m1 = map + (int64_t)y1 * gw;
    float gain[NC], h[NC];
    bool any = false, all = true;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const float fx = fminf(fmaxf(((float)(x + i) + 0.5f) * kInv - 0.5f, 0.0f), (float)(gw - 1));
        const int x0 = (int)fx, x1 = min(x0 + 1, gw - 1);
        const float wx = fx - (float)x0;
        const float a = m0[x0] + wx * (m0[x1] - m0[x0]);
        const float b = m1[x0] + wx * (m1[x1] - m1[x0]);
        gain[i] = a + wy * (b - a);
        h[i] = 0.5f * gain[i];
        any = any || gain[i] != 0.0f;
        all = all && gain[i] != 0.0f;
    }
    if (!any) return;                                                // the cells keep their bits, their gray cells are not written
    const int64_t hw = (int64_t)hh * ww;
    float g[NC] = {};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool green = k == plane_a || k == 3 - plane_a;         // uniform
        if (!green && !gray) continue;
        float* p = packed + ((int64_t)img * 4 + k) * hw + (int64_t)y * ww + x;
        float c[NC], v[NC];
        line_load_cells<NC>(p, c);
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            float d = dn_of(c[i], top);
            v[i] = c[i];
            if (green && gain[i] != 0.0f) {
                const float step = h[i] * (d - black);
                d = k == plane_a ? d - step : d + step;
                v[i] = norm_dn(d, top);                              // a cell without a gain keeps its bits
            }
            g[i] = k ? g[i] + d : d;
        }
        if (green) line_store_cells<NC>(p, v);
    }
    if (gray) {
        float* gp = gray + (int64_t)img * hw + (int64_t)y * ww + x;
        if (all) {
            line_store_gray<NC>(gp, g);
        } else {                                                     // NC == 4 alone gets here
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (gain[i] != 0.0f) gp[i] = g[i] * 0.25f;
        }
    }
}

}  // namespace

void green_grid(int hh, int ww, int* gh, int* gw) {
    *gh = (hh + kGreenBlock - 1) / kGreenBlock;
    *gw = (ww + kGreenBlock - 1) / kGreenBlock;
}

int64_t green_estimate_blocks(int n, int hh, int ww) {
    int gh, gw;
    green_grid(hh, ww, &gh, &gw);
    const int64_t blocks = (int64_t)n * gh * gw;                     // below 2^63: n < 2^31 and gh, gw < 2^26
    return blocks > 0x7fffffffll ? -1 : blocks;
}

hipError_t launch_green_estimate(const float* packed, int n, int hh, int ww, int bit_depth, int bayer, const RowsParams& p, float* e, float* level,
                                 uint8_t* state, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !e || !level || !state || hh < 2 || ww < 2 || bit_depth < 1 || bit_depth > 16 || bayer < 0 || bayer > 3) return hipErrorInvalidValue;
    const int64_t blocks = green_estimate_blocks(n, hh, ww);
    if (blocks < 0) return hipErrorInvalidValue;
    int gh, gw;
    green_grid(hh, ww, &gh, &gw);
    RowsParams P = p;
    P.top = top_of(bit_depth);
    hipLaunchKernelGGL(green_estimate_kernel, dim3((unsigned)blocks), dim3(kGreenThreads), 0, s, packed, e, level, state, hh, ww, gw,
                       (unsigned)(gh * gw), green_plane_a(bayer), P);
    return hipGetLastError();
}

hipError_t launch_green_apply(float* packed, float* gray, const float* map, int gh, int gw, float black, int n, int hh, int ww, int bit_depth,
                              int bayer, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !map || gh < 1 || gw < 1 || hh < 2 || ww < 2 || bit_depth < 1 || bit_depth > 16 || bayer < 0 || bayer > 3) return hipErrorInvalidValue;
    const bool wide = line_apply_wide(ww, packed, gray);
    int64_t bpf = 0;
    const int64_t blocks = line_apply_blocks(n, hh, ww, wide, &bpf);
    if (blocks < 0) return hipErrorInvalidValue;
    const float top = top_of(bit_depth);
    const int a = green_plane_a(bayer);
    if (wide)
        hipLaunchKernelGGL(green_apply_kernel<4>, dim3((unsigned)blocks), dim3(kGreenThreads), 0, s, packed, gray, map, gh, gw, black, hh, ww,
                           (unsigned)bpf, a, top);
    else
        hipLaunchKernelGGL(green_apply_kernel<1>, dim3((unsigned)blocks), dim3(kGreenThreads), 0, s, packed, gray, map, gh, gw, black, hh, ww,
                           (unsigned)bpf, a, top);
    return hipGetLastError();
}
