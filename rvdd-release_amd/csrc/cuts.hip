// One integer signature per frame for scene-cut detection (rvdd_frame_sigs; the rule is in include/rvdd.h).  Compiled -ffp-contract=off
// like noise.hip: the clamp, the product and the rounding are each one f32 operation, so that every count and every sum is the integer
// of the NumPy restatement (tests/cuts_ref.py).
//
// One workgroup per (frame, band).  A band's rows are a contiguous run of the gray plane; the workgroup walks it 1024 cells (wide form:
// a lane owns four cells of a row, one 16-byte load; ww % 4 == 0 and a 16-byte aligned pointer) or 256 cells (single floats) at a time,
// four loads in flight per lane.  Every word of the struct has this one owner: the 64 level counts and the 16 column sums of the band are
// written with plain stores at the end, nothing is accumulated in global memory.
//
// Contention.  A flat frame sends every cell of a wave to one level bin, and 64 lanes of an LDS atomic on one address serialise.  So
// every lane counts into LDS words of its OWN: count[bin / 2][lane] holds the lane's counts of two bins as two 16-bit halves,
// csum[column][lane] the lane's sum of q of one column, 32 bits.  The adds are ds_add_u32 without a return value on addresses no other
// lane touches, word index = row * 256 + lane: no two lanes of a wave meet on a bank, whatever the content.  A 16-bit count holds 65535
// cells and a 32-bit sum 2^32 / (4 * 65535) = 16384 cells, so the run is walked in chunks of kChunk iterations (at most 4 * kChunk = 8192
// cells per lane), and behind each chunk the words are folded into registers -- 32-bit counts, 64-bit sums -- by all 256 lanes: lane t
// adds up a quarter of row t / 4, the four quarters meet with two shuffles.  A frame of 1920 x 1080 cells is one chunk per band.
//
// Measured: 0.83 us per 720p frame at n = 16, 16.5 us per 2160p frame at n = 4, a flat frame and a scene alike.  Eight
// loads in flight, or plain read-modify-write of the lane's words with one add per lane and load, change neither figure, which
// points at the loop's own arithmetic (the exact 64-bit column bounds among it) on the four waves a band gets; no counter pass was run.
#include "../../include/rvdd.h"
#include "rvdd_internal.h"

namespace {

constexpr int kSigThreads = 256;
constexpr int kChunk = 2048;          // iterations between two folds
constexpr int kInFlight = 4;          // loads a lane issues before it consumes the first

// the column of cell x: (16 x) / ww without a 64-bit division -- an f32 estimate that is off by one at most, set right against the
// columns' exact bounds (x lies in column b iff b ww <= 16 x < (b + 1) ww)
__device__ __forceinline__ int sig_column(unsigned x, unsigned ww, float r) {
    int b = min((int)((float)x * r), 15);
    const unsigned long long x16 = (unsigned long long)x << 4;
    if (x16 < (unsigned long long)b * ww) --b;
    else if (x16 >= (unsigned long long)(b + 1) * ww) ++b;
    return b;
}

template <bool WIDE>
__global__ void __launch_bounds__(kSigThreads) frame_sig_kernel(const float* __restrict__ gray, rvdd_frame_sig* __restrict__ sig, int hh, int ww,
                                                                float top, float bin_scale) {
    constexpr int V = WIDE ? 4 : 1;
    __shared__ unsigned count[32 * kSigThreads];       // [bin / 2][lane]: two 16-bit counts
    __shared__ unsigned csum[16 * kSigThreads];        // [column][lane]
    const int tid = threadIdx.x;
    const int frame = (int)(blockIdx.x >> 4), by = (int)(blockIdx.x & 15);
    // band by holds the rows y with by hh <= 16 y < (by + 1) hh
    const int64_t y0 = ((int64_t)by * hh + 15) >> 4, y1 = ((int64_t)(by + 1) * hh + 15) >> 4;
    const float* p = gray + ((int64_t)frame * hh + y0) * ww;
    const int64_t cells = (y1 - y0) * ww;              // WIDE: a multiple of 4, and so is every row's start
    const int64_t iters = (cells + kSigThreads * V - 1) / (kSigThreads * V);
    const float r = 16.0f / (float)ww;
    const unsigned uww = (unsigned)ww, stepx = (unsigned)(kSigThreads * V) % uww;
    unsigned x = (unsigned)(tid * V) % uww;            // the column index of the lane's first cell of the iteration
    unsigned htotal = 0;                               // lane t: the count of bin t / 4 (after the shuffles)
    unsigned long long stotal = 0;                     // lane t < 64: the sum of column t / 4

    for (int i = tid; i < 32 * kSigThreads; i += kSigThreads) count[i] = 0;
    for (int i = tid; i < 16 * kSigThreads; i += kSigThreads) csum[i] = 0;
    __syncthreads();

    for (int64_t it0 = 0; it0 < iters; it0 += kChunk) {
        const int64_t it1 = min(it0 + (int64_t)kChunk, iters);
        for (int64_t it = it0; it < it1; it += kInFlight) {
            float g[kInFlight][V];
            bool in[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int64_t at = ((it + u) * kSigThreads + tid) * V;
                in[u] = it + u < it1 && at < cells;
                if constexpr (WIDE) {
                    const f32x4 v = in[u] ? *reinterpret_cast<const f32x4*>(p + at) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    g[u][0] = v[0]; g[u][1] = v[1]; g[u][2] = v[2]; g[u][3] = v[3];
                } else {
                    g[u][0] = in[u] ? p[at] : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                if (in[u]) {
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const float c = fminf(fmaxf(g[u][k], 0.0f), top);
                        const unsigned q = (unsigned)rintf(c * 4.0f);
                        const int j = min((int)(c * bin_scale), 63);
                        const int bx = sig_column(x + k, uww, r);          // WIDE: x + k < ww, the four cells share a row
                        atomicAdd(&count[(j >> 1) * kSigThreads + tid], 1u << ((j & 1) * 16));
                        atomicAdd(&csum[bx * kSigThreads + tid], q);
                    }
                }
                if (it + u < it1) {                                          // uniform: every lane steps, in or out of the run
                    x += stepx;                                              // both below ww <= 2^31 - 1: no wrap of the unsigned sum
                    if (x >= uww) x -= uww;
                }
            }
        }
        __syncthreads();
        // the fold: lane t takes words (t & 3) * 64 .. + 63 of row t / 4, starting t words in so that the lanes of a wave spread over the banks
        {
            const int row = tid >> 2, base = (tid & 3) * 64;
            unsigned h = 0;
#pragma unroll 8
            for (int l = 0; l < 64; ++l) h += (count[(row >> 1) * kSigThreads + base + ((l + tid) & 63)] >> ((row & 1) * 16)) & 0xffffu;
            h += __shfl_xor(h, 1);
            h += __shfl_xor(h, 2);
            htotal += h;
            unsigned long long s = 0;                                        // the first wave: lane t, a quarter of column t / 4
            if (tid < 64)
#pragma unroll 8
                for (int l = 0; l < 64; ++l) s += csum[row * kSigThreads + base + ((l + tid) & 63)];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            stotal += s;
        }
        __syncthreads();
        if (it1 < iters) {
            for (int i = tid; i < 32 * kSigThreads; i += kSigThreads) count[i] = 0;
            for (int i = tid; i < 16 * kSigThreads; i += kSigThreads) csum[i] = 0;
            __syncthreads();
        }
    }
    if ((tid & 3) == 0) sig[frame].hist[by][tid >> 2] = htotal;
    if (tid < 64 && (tid & 3) == 0) sig[frame].sum[by][tid >> 2] = stotal;
}

}  // namespace

bool frame_sig_wide(const float* gray, int ww) { return (ww & 3) == 0 && (reinterpret_cast<uintptr_t>(gray) & 15) == 0; }

hipError_t launch_frame_sigs(const float* gray, int n, int hh, int ww, int bit_depth, rvdd_frame_sig* sig, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!gray || !sig || n < 0 || n > 0x7fffffff / 16 || hh < 16 || ww < 16 || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const float top = (float)((1u << bit_depth) - 1u);
    const float bin_scale = 64.0f / (float)(1u << bit_depth);          // a power of two
    if (frame_sig_wide(gray, ww))
        hipLaunchKernelGGL(frame_sig_kernel<true>, dim3((unsigned)n * 16u), dim3(kSigThreads), 0, s, gray, sig, hh, ww, top, bin_scale);
    else
        hipLaunchKernelGGL(frame_sig_kernel<false>, dim3((unsigned)n * 16u), dim3(kSigThreads), 0, s, gray, sig, hh, ww, top, bin_scale);
    return hipGetLastError();
}
