// Residual statistics of a denoised frame against its noisy input (rvdd_resid_stats, the stage of rvdd_video_push behind rvdd_set_resid;
// the rule is in include/rvdd.h).  Compiled -ffp-contract=off like cuts.hip: the two conversions to DN, the difference, the product with
// the power of two, the clamps and the roundings are each one f32 operation, and every sum is an integer, so that every word of the
// accumulator is the integer of the NumPy restatement (tests/resid_ref.py).
//
// A thread owns V neighbouring cells of a row -- four in the wide form (ww % 4 == 0, both tensors 16-byte aligned: one 16-byte load of
// each packed plane, two of each of the four RGB half-rows the planes' sites lie in), one otherwise -- in all four planes.  A frame is
// walked by at most kResidGroups workgroups, each striding over the frame's items.  The right neighbour of a thread's last cell is the
// first cell of the next item: it comes from the next lane by a shuffle, and is formed again from memory by lane 63 alone.
//
// Binning.  Neighbouring samples share levels, a flat frame has ONE level: 64 lanes of an LDS atomic on one address serialise.  So
//   1. a thread adds up each RUN of equal bins among the V samples it holds of a plane (smooth content: one run per plane);
//   2. the wave combines equal bins before LDS is touched: the lanes that hold the bin of the first lane still waiting are added up
//      with DPP row operations (the others contribute zeros), one lane adds the six sums to the workgroup's table -- a wave of one
//      bin is one pass, a wave of three bins three;
//   3. the workgroup's 64 x 6 table of 64-bit words is folded into the frame's accumulator with one 64-bit integer atomic per non-zero
//      word, lane t on word t: contiguous, and integer, so that the totals do not depend on the order of arrival.
// A wave's sums are reduced in 32-bit pieces: per lane and run n <= 4, sum of rint(dc * 16) < 2^22, |sum rq| <= 2^19, and the two
// 64-bit sums (below 2^36 in magnitude) as their low 24 bits and the rest, so that 64 lanes never overflow a piece.
#include "../../include/rvdd.h"
#include "dpc_rule.h"      // dn_of

#include <algorithm>

namespace {

constexpr int kResidThreads = 256;
constexpr int kResidGroups = 128;         // workgroups per frame at most: what meets on one word of a flat frame's accumulator
constexpr int kResidWords = 6 * 64;       // struct rvdd_resid_acc as 64-bit words: [quantity][bin]

struct Sample {
    int rq, j;
    unsigned mq;
};

// one sample of the rule: p the packed value, r the output's value at its site
__device__ __forceinline__ Sample resid_sample(float p, float r, float top, float S, float bin_scale) {
    const float c = dn_of(p, top), d = dn_of(r, top);
    const float t = fminf(fmaxf((c - d) * S, -131072.0f), 131072.0f);
    const float dc = fminf(fmaxf(d, 0.0f), top);
    Sample s;
    s.rq = (int)rintf(t);
    s.j = min((int)(dc * bin_scale), 63);
    s.mq = (unsigned)rintf(dc * 16.0f);
    return s;
}

// the sums of one run of equal bins
struct Run {
    unsigned n, n11, mq;
    int s1;
    unsigned long long s2;
    long long s11;
};

// Every lane of the wave arrives.  The lanes with `active` add their run to table[quantity * 64 + bin], equal bins combined first.
__device__ __forceinline__ void wave_commit(bool active, int bin, const Run& r, unsigned long long* table, int lane) {
    unsigned long long todo = __ballot(active);
    while (todo) {                                                             // wave-uniform
        const int b = __shfl(bin, (int)__ffsll((long long)todo) - 1);
        const bool mine = active && bin == b;
        todo &= ~__ballot(mine);
        const unsigned cnt = wave_sum_u32(mine ? r.n | (r.n11 << 16) : 0u);    // 64 lanes of at most 4 each: no carry between the halves
        const unsigned mq = wave_sum_u32(mine ? r.mq : 0u);
        const int s1 = (int)wave_sum_u32(mine ? (unsigned)r.s1 : 0u);
        const unsigned s2lo = wave_sum_u32(mine ? (unsigned)(r.s2 & 0xffffffull) : 0u);
        const unsigned s2hi = wave_sum_u32(mine ? (unsigned)(r.s2 >> 24) : 0u);
        const unsigned s11lo = wave_sum_u32(mine ? (unsigned)(r.s11 & 0xffffffll) : 0u);
        const int s11hi = (int)wave_sum_u32(mine ? (unsigned)(int)(r.s11 >> 24) : 0u);      // arithmetic shift: v = hi * 2^24 + lo
        if (lane == 0) {
            atomicAdd(&table[0 * 64 + b], (unsigned long long)(cnt & 0xffffu));
            atomicAdd(&table[1 * 64 + b], (unsigned long long)mq);
            atomicAdd(&table[2 * 64 + b], (unsigned long long)(long long)s1);
            atomicAdd(&table[3 * 64 + b], ((unsigned long long)s2hi << 24) + s2lo);
            atomicAdd(&table[4 * 64 + b], (unsigned long long)(cnt >> 16));
            atomicAdd(&table[5 * 64 + b], (unsigned long long)((long long)s11hi * (1ll << 24) + (long long)s11lo));
        }
    }
}

template <bool WIDE>
__global__ void __launch_bounds__(kResidThreads) resid_kernel(const float* __restrict__ packed, const float* __restrict__ rgb,
                                                              unsigned long long* __restrict__ acc, int hh, int ww, int groups, int cols,
                                                              float top, float S, float bin_scale) {
    constexpr int V = WIDE ? 4 : 1;
    __shared__ unsigned long long table[kResidWords];
    const int tid = threadIdx.x, lane = tid & 63;
    const int frame = (int)(blockIdx.x / (unsigned)groups), grp = (int)(blockIdx.x % (unsigned)groups);
    for (int i = tid; i < kResidWords; i += kResidThreads) table[i] = 0;
    __syncthreads();

    const int64_t plane = (int64_t)hh * ww;                                    // cells of a plane; WIDE: a multiple of 4, and so is every row's start
    const int64_t items = plane / V;
    const float* pk = packed + (int64_t)frame * 4 * plane;
    const float* out = rgb + (int64_t)frame * 12 * plane;
    const int64_t W = 2 * (int64_t)ww;
    const bool small = plane < (1ll << 31);

    // wave-uniform bounds: every lane of a wave walks the same iterations, in or out of the frame, so that the shuffles and the
    // wave's sums see all 64 lanes
    for (int64_t base = (int64_t)grp * kResidThreads + (tid - lane); base < items; base += (int64_t)groups * kResidThreads) {
        const int64_t item = base + lane;
        const bool in = item < items;
        const int64_t cell = in ? item * V : 0;
        int64_t y;
        int x;
        if (small) {                                                           // uniform
            const unsigned q = (unsigned)cell / (unsigned)ww;
            y = q;
            x = (int)((unsigned)cell - q * (unsigned)ww);
        } else {
            y = cell / ww;
            x = (int)(cell - y * ww);
        }
        const bool more = in && x < ww - V;                                    // the row goes on behind the thread's cells: item + 1 holds them
        Sample s[4][V];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* prow = pk + (k * plane + y * ww + x);
            const float* orow = out + (((cols >> (2 * k)) & 3) * 4 * plane + (2 * y + (k >> 1)) * W + 2 * (int64_t)x + (k & 1));
            if constexpr (WIDE) {
                f32x4 p = {0.0f, 0.0f, 0.0f, 0.0f}, a = p, b = p;
                if (in) {
                    p = *reinterpret_cast<const f32x4*>(prow);
                    a = *reinterpret_cast<const f32x4*>(orow - (k & 1));      // the eight sites 2x .. 2x + 7 of the row; the plane's are every other one
                    b = *reinterpret_cast<const f32x4*>(orow - (k & 1) + 4);
                }
                const int o = k & 1;
                s[k][0] = resid_sample(p[0], o ? a[1] : a[0], top, S, bin_scale);
                s[k][1] = resid_sample(p[1], o ? a[3] : a[2], top, S, bin_scale);
                s[k][2] = resid_sample(p[2], o ? b[1] : b[0], top, S, bin_scale);
                s[k][3] = resid_sample(p[3], o ? b[3] : b[2], top, S, bin_scale);
            } else {
                s[k][0] = resid_sample(in ? prow[0] : 0.0f, in ? orow[0] : 0.0f, top, S, bin_scale);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // rq of cell x + V of this plane: the next lane's first sample; lane 63 forms it from memory
            int nb = __shfl_down(s[k][0].rq, 1);
            if (lane == 63 && more) {
                const float* prow = pk + (k * plane + y * ww + x + V);
                const float* orow = out + (((cols >> (2 * k)) & 3) * 4 * plane + (2 * y + (k >> 1)) * W + 2 * ((int64_t)x + V) + (k & 1));
                nb = resid_sample(prow[0], orow[0], top, S, bin_scale).rq;
            }
            // runs of equal bins, from the back: r[c] = the sums of samples c .. the end of c's run
            Run r[V];
            bool head[V];
#pragma unroll
            for (int c = V - 1; c >= 0; --c) {
                const bool pair = c + 1 < V || more;
                const long long q = s[k][c].rq;
                const long long right = c + 1 < V ? s[k][c + 1 < V ? c + 1 : c].rq : nb;
                Run one{1u, pair ? 1u : 0u, s[k][c].mq, s[k][c].rq, (unsigned long long)(q * q), pair ? q * right : 0ll};
                if (c + 1 < V && s[k][c + 1 < V ? c + 1 : c].j == s[k][c].j) {
                    const Run& t = r[c + 1 < V ? c + 1 : c];
                    one.n += t.n; one.n11 += t.n11; one.mq += t.mq; one.s1 += t.s1; one.s2 += t.s2; one.s11 += t.s11;
                }
                r[c] = one;
                head[c] = c == 0 || s[k][c > 0 ? c - 1 : 0].j != s[k][c].j;
            }
#pragma unroll
            for (int c = 0; c < V; ++c) {
                const bool active = in && head[c];
                if (__any(active)) wave_commit(active, s[k][c].j, r[c], table, lane);      // uniform
            }
        }
    }
    __syncthreads();
    unsigned long long* dst = acc + (int64_t)frame * kResidWords;
    for (int i = tid; i < kResidWords; i += kResidThreads)
        if (table[i]) atomicAdd(&dst[i], table[i]);
}

}  // namespace

bool resid_wide(const float* packed, const float* rgb, int ww) {
    return (ww & 3) == 0 && ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(rgb)) & 15) == 0;
}

int64_t resid_blocks(int n, int hh, int ww, bool wide, int* groups) {
    const int64_t items = (int64_t)hh * ww / (wide ? 4 : 1);                  // hh, ww >= 1
    const int64_t g = std::min<int64_t>((items + kResidThreads - 1) / kResidThreads, kResidGroups);
    if (groups) *groups = (int)g;
    // the tensors' element offsets are 64-bit: 12 n hh ww must stay below 2^63
    if ((int64_t)hh * ww > (1ll << 62) / 12 / std::max(n, 1)) return -1;
    const int64_t blocks = (int64_t)n * g;
    return blocks > 0x7fffffffll ? -1 : blocks;
}

hipError_t launch_resid(const float* packed, const float* rgb, int n, int hh, int ww, int bayer, int bit_depth, rvdd_resid_acc* acc,
                        hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!packed || !rgb || !acc || n < 0 || hh < 1 || ww < 1 || bayer < 0 || bayer > 3 || bit_depth < 1 || bit_depth > 16 ||
        (reinterpret_cast<uintptr_t>(acc) & 7))
        return hipErrorInvalidValue;
    const bool wide = resid_wide(packed, rgb, ww);
    int groups = 0;
    const int64_t blocks = resid_blocks(n, hh, ww, wide, &groups);
    if (blocks < 0) return hipErrorInvalidValue;
    const float top = (float)((1u << bit_depth) - 1u);
    const float S = bit_depth == 16 ? 0.5f : (float)(1u << (15 - bit_depth));
    const float bin_scale = 64.0f / (float)(1u << bit_depth);          // a power of two
    unsigned long long* words = reinterpret_cast<unsigned long long*>(acc);
    const int cols = bayer_cols(bayer);
    if (wide)
        hipLaunchKernelGGL(resid_kernel<true>, dim3((unsigned)blocks), dim3(kResidThreads), 0, s, packed, rgb, words, hh, ww, groups, cols, top, S,
                           bin_scale);
    else
        hipLaunchKernelGGL(resid_kernel<false>, dim3((unsigned)blocks), dim3(kResidThreads), 0, s, packed, rgb, words, hh, ww, groups, cols, top, S,
                           bin_scale);
    return hipGetLastError();
}
