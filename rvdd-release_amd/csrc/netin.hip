// The network input of a frame-step and the bound of its maximum: per pixel the bicubic warp of the previous output, the
// demosaic of the current frame and the warp of the next one, as the NHWC16 map (netin_kernel), projected 16 -> 48 without
// the map (netin_proj_kernel), or with the green plane and the bound in the same launch (netin_small_kernel); the bound from
// the packed raw frames alone (netin_bound_kernel).  Compiled with -ffp-contract=off like the demosaic and the warp whose
// arithmetic (demosaic.h, warp.h) it repeats bit for bit.
#include "demosaic.h"
#include "warp.h"

namespace {

// The network input of a frame in ONE pass (models/recurrent_model.py:299-324): per pixel the bicubic warp of the
// previous output (3 channels), the red / blue planes of the current frame's Hamilton-Adams demosaic (its green
// plane comes from ha_green_kernel) and, with a future frame, the warp of the demosaicked next frame, written as the
// pixel's whole NHWC16 vector -- three 16-B stores of full sectors.  Written by three kernels (red/blue, two warps)
// every pixel's 64 bytes were touched three times with 12-B partial stores.  Same arithmetic as ha_rb_kernel and
// warp3_kernel (the demosaic stays bit-exact).
// The 16 channels of one network-input pixel: warp3 of prev4 | demosaic of raw_cur | warp3 of next4 (zeros without one) | 0..
struct NetinArgs {
    const float *raw_cur, *green, *prev4, *flow_prev, *next4, *flow_next;
    int B, h, w;
    int bayer;          // enum rvdd_bayer of raw_cur: picks the kernel's instantiation (the kernels read their phase PH, not this)
    int64_t rbs, fbs;
};
// The previous output warped to pixel (y, x) and the demosaic's red and blue there: the taps of the previous output gathered
// together (--no_warp: the pixel itself, models/recurrent_model.py:156-158), the demosaic's arithmetic under the gather's
// flight, then the sum.  `vt`: the gather's 64 registers, the caller's to use again.
template <int PH>
__device__ __forceinline__ f32x4 warp_prev_red_blue(const f32x4* __restrict__ sp, bool warp_p, const FlowQ& fq, const Ring& q, int y, int x,
                                                    int H, int W, f32x4 (&vt)[16], float (&rb)[2]) {
    Taps tp;
    f32x4 p;
    if (warp_p) {
        float fx, fy;
        flow_combine(fq, fx, fy);
        make_taps(fx, fy, x, y, H, W, tp);
        warp3_gather(sp, tp, W, vt);
    } else {
        p = sp[(size_t)y * W + x];
    }
    ha_red_blue<PH>(q, y, x, rb);
    if (warp_p) p = warp3_sum(tp, vt);
    return p;
}
// Three batches of loads, each in flight together: (1) the flow vectors around the pixel (both directions) and the 3x3 rings of the
// green plane and the CFA, (2) the 16 bicubic taps of the previous output, (3) those of the next frame -- with the demosaic's
// arithmetic between them.  Written as one expression after another (round 1-5) the compiler kept the kernel at 8 waves per SIMD by
// issuing every load next to its use: ~60 dependent memory round trips per pixel, waves 75 % of their life in s_waitcnt
// (profiles/r06f_c4_prestage_counters.json).  Same operations on the same values: same bits.
template <int PH>
__device__ __forceinline__ void netin_pixel(const NetinArgs& a, size_t idx, f32x4 (&o)[3]) {
    const int H = 2 * a.h, W = 2 * a.w;
    const unsigned i32 = (unsigned)idx;      // (B H W < 2^32: launch_netin checks; 64-bit divisions are ~100 instructions each)
    const int x = (int)(i32 % (unsigned)W);
    const unsigned yb = i32 / (unsigned)W;
    const int y = (int)(yb % (unsigned)H);
    const int b = (int)(yb / (unsigned)H);
    Cfa c{a.raw_cur + (size_t)b * a.rbs, a.h, a.w, H, W};
    const float* gp = a.green + (size_t)b * H * W;
    const f32x4* sp = reinterpret_cast<const f32x4*>(a.prev4) + (size_t)b * H * W;
    const f32x4* sn = reinterpret_cast<const f32x4*>(a.next4) + (size_t)b * H * W;
    const bool warp_p = a.flow_prev != nullptr, has_n = a.next4 != nullptr, warp_n = has_n && a.flow_next != nullptr;
    // ---- batch 1
    FlowQ fq_p, fq_n;
    if (warp_p) flow_fetch(a.flow_prev + (size_t)b * a.fbs, a.h, a.w, H, W, y, x, fq_p);
    if (warp_n) flow_fetch(a.flow_next + (size_t)b * a.fbs, a.h, a.w, H, W, y, x, fq_n);
    Ring q;
    load_ring<PH>(c, gp, H, W, y, x, q);
    // ---- batch 2
    f32x4 vt[16];
    f32x4 n = {0.f, 0.f, 0.f, 0.f};
    float rb[2];
    const f32x4 p = warp_prev_red_blue<PH>(sp, warp_p, fq_p, q, y, x, H, W, vt, rb);
    const float g0 = q.g[1][1];
    // ---- batch 3: the next frame's taps (one gather's 64 registers at a time: both in flight spill)
    if (warp_n) {
        float fx, fy;
        flow_combine(fq_n, fx, fy);
        Taps tn;
        make_taps(fx, fy, x, y, H, W, tn);
        warp3_gather(sn, tn, W, vt);
        n = warp3_sum(tn, vt);
    } else if (has_n) {
        n = sn[(size_t)y * W + x];
    }
    o[0] = f32x4{p[0], p[1], p[2], rb[0]};
    o[1] = f32x4{g0, rb[1], n[0], n[1]};
    o[2] = f32x4{n[2], 0.f, 0.f, 0.f};
}
// Workgroups go to the eight XCDs in turn; a pixel's stencils and bicubic taps reach two rows up and down, and a row is
// several workgroups long: numbered as they come, vertically adjacent workgroups sit on different XCDs and every L2
// fetches the same rows again.  Each XCD takes a contiguous eighth of the pixels instead.  lin = the workgroup's linear index
// in its grid of n.
__device__ __forceinline__ unsigned xcd_contiguous_block(unsigned lin, unsigned n) {
    const unsigned per = n >> 3;
    return lin < 8u * per ? (lin & 7u) * per + (lin >> 3) : lin;
}

// (at most five waves per SIMD asked of the compiler: with the default target of eight it serialises the loads again to save registers)
template <int PH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void netin_kernel(NetinArgs a, float* __restrict__ netin) {
    const size_t idx = (size_t)xcd_contiguous_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
    if (idx >= (size_t)a.B * 4 * a.h * a.w) return;
    f32x4 v[3];
    netin_pixel<PH>(a, idx, v);
    f32x4* o = reinterpret_cast<f32x4*>(netin) + idx * 4;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
}

// netin_kernel for ConvNeXtUnet: the network input has exactly one reader there, the 1x1 projection 9 | 6 -> 48 of the first
// ConvBlock (networks/new_unet.py:85-88), so the 16-channel map is never written: the 256 pixels of a workgroup change lanes
// through LDS (pixel pitch 24 floats: the 16 lanes of a ds_read_b128 group on 16 distinct bank quads) and each wave projects
// four 16-pixel groups on the f32 matrix pipe (16x16x4, exact f32 products).  pw as proj1x1_kernel<16, 0>'s:
// [m 3][lr 16][g 4][i 4] = W[16m+lr][4g+i] (zero for channels the input does not have).
template <int PH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void netin_proj_kernel(NetinArgs a, const float* __restrict__ pw, const float* __restrict__ bias,
                                                         float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_t[256][24];
    const size_t total = (size_t)a.B * 4 * a.h * a.w;
    const size_t base = (size_t)xcd_contiguous_block(blockIdx.x, gridDim.x) * 256;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, lr = lane & 15, g = lane >> 4;
    f32x4 wa[3], bv[3];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        wa[m] = *reinterpret_cast<const f32x4*>(pw + (((size_t)m * 16 + lr) * 4 + g) * 4);
        bv[m] = *reinterpret_cast<const f32x4*>(bias + 16 * m + 4 * g);
    }
    f32x4 v[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (base + threadIdx.x < total) netin_pixel<PH>(a, base + threadIdx.x, v);
#pragma unroll
    for (int k = 0; k < 3; ++k) *reinterpret_cast<f32x4*>(&s_t[threadIdx.x][4 * k]) = v[k];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int px = 64 * wv + 16 * q + lr;
        f32x4 xb = *reinterpret_cast<const f32x4*>(&s_t[px][4 * (g < 3 ? g : 0)]);
        if (g == 3) xb = f32x4{0.f, 0.f, 0.f, 0.f};           // channels 12..15 do not exist
        f32x4 acc[3] = {bv[0], bv[1], bv[2]};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[m][i], xb[i], acc[m], 0, 0, 0);
        if (base + px < total) {
#pragma unroll
            for (int m = 0; m < 3; ++m) *reinterpret_cast<f32x4*>(out + (base + px) * kF + 16 * m + 4 * g) = acc[m];
        }
    }
}

// housekeeping for the step AFTER this one: its set of amax words and its features slot, which nobody touches meanwhile --
// cleared by all the threads of a two-dimensional grid of 256-thread blocks together (either range nullable)
__device__ __forceinline__ void zero_for_next_step(unsigned* zero_a, size_t zero_na, unsigned* zero_b, size_t zero_nb) {
    const size_t me = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x, all = (size_t)gridDim.x * gridDim.y * 256;
    if (zero_a) for (size_t i = me; i < zero_na; i += all) zero_a[i] = 0u;
    if (zero_b) for (size_t i = me; i < zero_nb; i += all) zero_b[i] = 0u;
}
// x 16: four up on the exponent (a maximum that is zero, denormal, or within 2^4 of overflow stays as it is)
__device__ __forceinline__ float times16(unsigned bits) {
    const unsigned e = (bits >> 23) & 0xffu;
    if (e >= 1 && e < 250) bits += 4u << 23;
    return __uint_as_float(bits);
}

// An upper bound of max |network input| per sequence, for the block floating point of the conv behind it (rvdd_internal.h),
// from what the input is made of instead of from its 16-channel map (a pass over that map, or a maximum inside netin_kernel's
// 28 800 blocks, costs 100 us and more per frame-step at 720p; this kernel reads the packed raw frames, 1/16 of it):
//   |bicubic gather of x| <= 1.375^2 max |x| (A = -0.75: the taps' absolute sum peaks at 1.375 per axis),
//   |Hamilton-Adams(raw)| <= 3 max |raw| (green: a two-sample mean plus a quarter of a Laplacian, <= 2 M; red / blue: a
//   two-sample mean plus a quarter of a Laplacian of those greens, <= 3 M),
// so max |netin| <= 5.7 max(max |raw|, max |previous output|) < 16 max(...) -- and >= max |raw_cur|, whose samples the demosaic
// keeps: the bound is never more than 16 x too large, four of the seventeen binades the split's full precision spans.
// Up to three raw frames (the current one, the next one, and on the first step of a video the previous one, whose demosaic is
// the "previous output"; each nullable); `prev_words` (nullable) = words whose maximum bounds the previous output (the slot
// PostConvs wrote in the last step: features and output frame together); grid (blocks, B).
// `latch` (rvdd_reset_slots): the sequences that start a video on this step (seq_latched) -- they bound from raw_c and ignore
// prev_words, the others ignore raw_c and read prev_words: each sequence gets the bound it would get alone.
__global__ __launch_bounds__(256) void netin_bound_kernel(const float* __restrict__ raw_a, const float* __restrict__ raw_b,
                                                          const float* __restrict__ raw_c, int64_t n, int64_t rbs,
                                                          const unsigned* __restrict__ prev_words, unsigned* __restrict__ words,
                                                          unsigned* __restrict__ zero_a, size_t zero_na, unsigned* __restrict__ zero_b,
                                                          size_t zero_nb, unsigned long long latch) {
    __shared__ unsigned red[4];
    const int b = blockIdx.y;
    const bool lat = raw_c && seq_latched(latch, b);
    zero_for_next_step(zero_a, zero_na, zero_b, zero_nb);
    float m = 0.f;
    for (int pass = 0; pass < 3; ++pass) {
        const float* src = pass == 0 ? raw_a : pass == 1 ? raw_b : lat ? raw_c : nullptr;
        if (!src) continue;
        const f32x4* p = reinterpret_cast<const f32x4*>(src + (size_t)b * rbs);
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < (n >> 2); i += (int64_t)gridDim.x * 256) m = absmax4(m, p[i]);
    }
    unsigned bits = __float_as_uint(m);
    if (blockIdx.x == 0 && prev_words && !lat && threadIdx.x < kAmaxLines)
        bits = max(bits, prev_words[(size_t)b * kAmaxSeqWords + threadIdx.x * kAmaxLineWords]);
    amax_commit_block(words, b, blockIdx.x, times16(bits), red);
}

// The three pre-stage launches of a frame-step -- netin_bound_kernel, ha_green_kernel, netin_kernel -- in ONE for small frames without
// a future frame (round 6: BASELINE's C1 as stated, one 256x256 sequence, is 28 launches of 5-15 us back to back; these three were
// 14.7 us of ~270).  A block owns a 16x16 tile: the green plane of the 18x18 pixels around it goes to LDS (ha_green_at at the
// clamped coordinates, i.e. what the green kernel wrote and netin_kernel read back through a clamped index), then netin_pixel's
// sequence per pixel with the ring's greens from LDS, then netin_bound_kernel's tail: every raw sample of the current frame is some
// thread's own CFA sample.  Same operations on the same values: same bits as the three kernels.  The tail only where the launch is
// small: one atomic per block on the amax words costs 100 us at 28 800 blocks (720p, round 4).  Above 1024 blocks the bound stays in
// netin_bound_kernel (14 us), which also keeps the housekeeping, and this kernel (words == nullptr) replaces ha_green_kernel and
// netin_kernel: the green plane, written to memory and read back nine times per pixel through the address path that bounds
// netin_kernel, stays in LDS.
template <int PH>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 4))) void netin_small_kernel(
    NetinArgs a, float* __restrict__ netin, const float* __restrict__ raw_prev, const unsigned* __restrict__ prev_words,
    unsigned* __restrict__ words, unsigned* __restrict__ zero_a, size_t zero_na, unsigned* __restrict__ zero_b, size_t zero_nb, int tiles_x,
    unsigned long long latch, int xcd_walk) {
    __shared__ float cs[22][24];     // the replicate-padded CFA at (y0 - 3 + r, x0 - 3 + c): what the 18x18 greens and the rings read
    __shared__ float gs[18][20];
    __shared__ unsigned red[4];
    const int H = 2 * a.h, W = 2 * a.w;
    const int t = threadIdx.x;
    // (sequence, tile) of this block.  xcd_walk (the large launches): workgroups go to the eight XCDs in turn in the order
    // x, then y, of the grid; each XCD takes a contiguous eighth of the (sequence, tile) pairs, i.e. a band of tile rows, instead
    unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
    if (xcd_walk) lin = xcd_contiguous_block(lin, gridDim.x * gridDim.y);
    const int b = (int)(lin / gridDim.x), tile = (int)(lin - (unsigned)b * gridDim.x);
    const bool lat = raw_prev && seq_latched(latch, b);      // netin_bound_kernel's choice of bound
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int y0 = ty * 16, x0 = tx * 16;
    zero_for_next_step(zero_a, zero_na, zero_b, zero_nb);
    Cfa c{a.raw_cur + (size_t)b * a.rbs, a.h, a.w, H, W};
    // Every CFA sample the tile needs, once: 22x22 loads per 256 pixels.  (Each green formed from memory -- up to nine loads --
    // and each pixel's ring -- nine more -- went through the address path that bounds this kernel: 301 us against netin_kernel's
    // 253 at 720p B = 8.)  The greens' stencils reach two samples beyond their 18x18 clamped positions, all inside the 22x22.
    for (int i = t; i < 22 * 22; i += 256) {
        const int r = i / 22, cc = i - r * 22;
        cs[r][cc] = c.at(y0 - 3 + r, x0 - 3 + cc);
    }
    const int ly = t >> 4, lx = t & 15, y = y0 + ly, x = x0 + lx;
    const bool inside = y < H && x < W;
    // flow vectors while the samples arrive
    FlowQ fq;
    Ring q;
    const bool warp_p = a.flow_prev != nullptr;
    const f32x4* sp = reinterpret_cast<const f32x4*>(a.prev4) + (size_t)b * H * W;
    if (inside && warp_p) flow_fetch(a.flow_prev + (size_t)b * a.fbs, a.h, a.w, H, W, y, x, fq);
    __syncthreads();
    const auto cfa = [&](int yy, int xx) { return cs[yy - (y0 - 3)][xx - (x0 - 3)]; };
    for (int i = t; i < 18 * 18; i += 256) {
        const int r = i / 18, cc = i - r * 18;
        gs[r][cc] = ha_green_from<PH>(cfa, clampi(y0 - 1 + r, 0, H - 1), clampi(x0 - 1 + cc, 0, W - 1));
    }
    __syncthreads();
    float m = 0.f;
    if (inside) {
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int yy = clampi(y + dy - 1, 0, H - 1), xx = clampi(x + dx - 1, 0, W - 1);
                q.site[dy][dx] = (((yy & 1) << 1) | (xx & 1)) ^ PH;
                q.r[dy][dx] = cfa(yy, xx);
                q.g[dy][dx] = gs[ly + dy][lx + dx];
            }
        f32x4 vt[16];
        float rb[2];
        const f32x4 p = warp_prev_red_blue<PH>(sp, warp_p, fq, q, y, x, H, W, vt, rb);
        const float g0 = q.g[1][1];
        f32x4* o = reinterpret_cast<f32x4*>(netin) + ((size_t)b * H * W + (size_t)y * W + x) * 4;
        o[0] = f32x4{p[0], p[1], p[2], rb[0]};
        o[1] = f32x4{g0, rb[1], 0.f, 0.f};
        o[2] = f32x4{0.f, 0.f, 0.f, 0.f};
        m = fabsf(q.r[1][1]);
        // (the first step of a video: the "previous output" is the demosaic of the previous raw frame, whose samples bound it)
        if (lat) m = fmaxf(m, fabsf(raw_prev[(size_t)b * a.rbs + ((size_t)(q.site[1][1] ^ PH) * c.h + (y >> 1)) * c.w + (x >> 1)]));
    }
    if (words) {      // netin_bound_kernel's tail
        unsigned bits = __float_as_uint(m);
        if (tile == 0 && prev_words && !lat && t < kAmaxLines) bits = max(bits, prev_words[(size_t)b * kAmaxSeqWords + t * kAmaxLineWords]);
        amax_commit_block(words, b, tile, times16(bits), red);
    }
}

}  // namespace

hipError_t launch_netin(const float* raw_cur, float* green_scratch, const float* prev4, const float* flow_prev,
                        const float* next4, const float* flow_next, float* netin, int B, int h, int w, hipStream_t s,
                        int64_t raw_bstride, int64_t flow_bstride, const float* proj_w16, const float* proj_b, float* proj_out, int bayer) {
    const size_t n = (size_t)B * 4 * h * w;
    if (!n) return hipSuccess;
    if (n >= 0x100000000ull) return hipErrorInvalidValue;      // netin_pixel's 32-bit pixel index
    const int64_t rbs = raw_bstride ? raw_bstride : (int64_t)4 * h * w, fbs = flow_bstride ? flow_bstride : (int64_t)2 * h * w;
    const NetinArgs a{raw_cur, green_scratch, prev4, flow_prev, next4, flow_next, B, h, w, bayer, rbs, fbs};
    const hipError_t e = launch_ha_green(raw_cur, green_scratch, B, h, w, rbs, s, bayer);
    if (e != hipSuccess) return e;
    if (proj_w16) {
        RVDD_BAYER_DISPATCH(a.bayer, netin_proj_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, a, proj_w16, proj_b, proj_out);
    } else {
        RVDD_BAYER_DISPATCH(a.bayer, netin_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, a, netin);
    }
    return hipGetLastError();
}

hipError_t launch_netin_bound(const float* raw_a, const float* raw_b, const float* raw_c, int B, int h, int w, int64_t raw_bstride,
                              const unsigned* prev_words, unsigned* words, hipStream_t s, unsigned* zero_a, size_t zero_na,
                              unsigned* zero_b, size_t zero_nb, unsigned long long latch) {
    const int64_t n = (int64_t)4 * h * w;
    if (B <= 0 || n <= 0) return hipSuccess;
    if ((n & 3) || (raw_bstride & 3)) return hipErrorInvalidValue;      // 16-B loads (n = 4hw: always)
    int nblk = (int)((n / 4 + 256 * 8 - 1) / (256 * 8));
    nblk = nblk < 1 ? 1 : (nblk > 64 ? 64 : nblk);
    hipLaunchKernelGGL(netin_bound_kernel, dim3(nblk, B), dim3(256), 0, s, raw_a, raw_b, raw_c, n, raw_bstride ? raw_bstride : n,
                       prev_words, words, zero_a, zero_na, zero_b, zero_nb, latch);
    return hipGetLastError();
}

// Can a frame-step of this size take the one-kernel pre-stage (netin_small_kernel)?  No future frame, at most 1024 tiles of 16x16.
// enabled = false: never (option "small_prestage" 0: the three pre-stage kernels at every size, the A/B reference).
constexpr long kNetinSmallTiles = 1024;
static long netin_tiles(int B, int h, int w) { return (long)B * ((2 * h + 15) / 16) * ((2 * w + 15) / 16); }
bool netin_small_applies(int B, int h, int w, bool future, bool enabled) {
    return netin_tiled_applies(h, w, future, enabled) && netin_tiles(B, h, w) <= kNetinSmallTiles;
}
// ... and the tiled kernel for the network input alone (words == nullptr, nothing to clear) at every size: the bound stays in
// netin_bound_kernel above 1024 tiles, the green plane never goes to memory.
bool netin_tiled_applies(int h, int w, bool future, bool enabled) { return enabled && !future && h >= 1 && w >= 1; }
hipError_t launch_netin_small(const float* raw_cur, const float* raw_prev, const float* prev4, const float* flow_prev, float* netin, int B,
                              int h, int w, int64_t raw_bstride, int64_t flow_bstride, const unsigned* prev_words, unsigned* words,
                              hipStream_t s, unsigned* zero_a, size_t zero_na, unsigned* zero_b, size_t zero_nb, unsigned long long latch,
                              int bayer) {
    if (B <= 0 || h <= 0 || w <= 0) return hipSuccess;
    const int tiles_x = (2 * w + 15) / 16, tiles_y = (2 * h + 15) / 16;
    const int64_t rbs = raw_bstride ? raw_bstride : (int64_t)4 * h * w, fbs = flow_bstride ? flow_bstride : (int64_t)2 * h * w;
    const NetinArgs a{raw_cur, nullptr, prev4, flow_prev, nullptr, nullptr, B, h, w, bayer, rbs, fbs};
    const bool large = netin_tiles(B, h, w) > kNetinSmallTiles;
    if (large && (words || zero_a || zero_b)) return hipErrorInvalidValue;      // one atomic per block: launch_netin_bound's work there
    if ((long)tiles_x * tiles_y * B >= 0x100000000l) return hipErrorInvalidValue;
    RVDD_BAYER_DISPATCH(a.bayer, netin_small_kernel, dim3(tiles_x * tiles_y, B), dim3(256), 0, s, a, netin, raw_prev, prev_words, words,
                        zero_a, zero_na, zero_b, zero_nb, tiles_x, latch, large ? 1 : 0);
    return hipGetLastError();
}
