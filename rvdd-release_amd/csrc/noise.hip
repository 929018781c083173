// Block statistics of packed raw frames for the noise-curve estimate (rvdd_noise_hist; the rule is in include/rvdd.h).  Compiled
// -ffp-contract=off like dpc.hip: every operation below is rounded to f32 on its own, and the sums run in the header's order, so
// that the keys and the sums of means are the integers of the NumPy restatement (tests/noise_ref.py).
//
// A lane owns one 8 x 8 block: eight rows of two 16-byte loads (the wide form: ww % 4 == 0, a 16-byte aligned pointer) or of eight
// single floats, consumed row by row -- the row sum, the six squared second differences, the clip test -- so that nothing but the
// running sums stays live.  Neighbouring lanes own neighbouring blocks of a block row: a wave reads runs of up to 2 KiB of each of
// eight rows.  The kernel writes almost nothing; it is bound by the 16 bytes per raw cell it reads.
//
// Contention.  A flat scene sends every block of a frame to one mean bin and a few dozen variance sub-bins.  A workgroup (256 lanes,
// 256 blocks) therefore combines equal keys in an open-addressing table in LDS (512 slots for at most 256 keys: it never fills),
// the sums of means in 64 LDS words of 64 bits and the three counters in three more, and goes to global memory once per distinct
// key, touched mean bin and non-zero counter -- integer vector atomics, so the totals do not depend on the order of arrival.
#include "../../include/rvdd.h"
#include "dpc_rule.h"      // dn_of

namespace {

constexpr int kNoiseThreads = 256;
constexpr int kNoiseSlots = 512;
constexpr unsigned kNoiseEmpty = 0xffffffffu;

template <bool WIDE>
__global__ void __launch_bounds__(kNoiseThreads) noise_hist_kernel(const float* __restrict__ packed, NoiseAcc* __restrict__ acc, int hh, int ww,
                                                                   int bh, int bw, int64_t total, float top, float bin_scale) {
    __shared__ unsigned keys[kNoiseSlots], cnt[kNoiseSlots];
    __shared__ unsigned long long msum[64];
    __shared__ unsigned counters[3];
    for (int i = threadIdx.x; i < kNoiseSlots; i += kNoiseThreads) {
        keys[i] = kNoiseEmpty;
        cnt[i] = 0;
    }
    if (threadIdx.x < 64) msum[threadIdx.x] = 0;
    if (threadIdx.x < 3) counters[threadIdx.x] = 0;
    __syncthreads();

    const int64_t g = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;       // the block, counted over planes, block rows, blocks of a row
    if (g < total) {
        const int bx = (int)(g % bw);
        const int64_t t = g / bw;
        const int by = (int)(t % bh);
        const int64_t plane = t / bh;                                           // image * 4 + channel
        const float* p = packed + (plane * hh + (int64_t)by * 8) * ww + (int64_t)bx * 8;
        float s = 0.0f, q = 0.0f;
        float margin = top;                                                     // the least of x and top - x over the samples: > 0 iff every one lies in (0, top)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const float* row = p + (int64_t)r * ww;
            float x[8];
            if constexpr (WIDE) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(row), hi = *reinterpret_cast<const f32x4*>(row + 4);
                x[0] = lo[0]; x[1] = lo[1]; x[2] = lo[2]; x[3] = lo[3];
                x[4] = hi[0]; x[5] = hi[1]; x[6] = hi[2]; x[7] = hi[3];
            } else {
#pragma unroll
                for (int c = 0; c < 8; ++c) x[c] = row[c];
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                x[c] = dn_of(x[c], top);
                margin = fminf(fminf(margin, x[c]), top - x[c]);                // top - x is exact enough: it is 0 only where x == top
            }
            float rs = x[0] + x[1];
#pragma unroll
            for (int c = 2; c < 8; ++c) rs = rs + x[c];
            float rq = 0.0f;
#pragma unroll
            for (int c = 1; c < 7; ++c) {
                const float d = x[c] - (x[c - 1] + x[c + 1]) * 0.5f;
                rq = rq + d * d;
            }
            s = r ? s + rs : rs;
            q = r ? q + rq : rq;
        }
        const float m = s * 0.015625f;
        const float v = q * (float)(1.0 / 72.0);
        atomicAdd(&counters[0], 1u);
        if (!(margin > 0.0f)) {
            atomicAdd(&counters[1], 1u);
        } else if (v == 0.0f) {
            atomicAdd(&counters[2], 1u);
        } else {
            const int i = min(max((int)(m * bin_scale), 0), 63);
            const int j = min(max((int)(__float_as_uint(v) >> 19) - ((127 - 6) << 4), 0), 511);
            atomicAdd(&msum[i], (unsigned long long)llrintf(m * 16.0f));
            const unsigned key = (unsigned)(i * 512 + j);
            unsigned slot = (key * 0x9E3779B1u) >> 23;                          // 9 bits
            for (;;) {                                                          // at most 256 keys in 512 slots: a free slot exists
                const unsigned old = atomicCAS(&keys[slot], kNoiseEmpty, key);
                if (old == kNoiseEmpty || old == key) break;
                slot = (slot + 1) & (kNoiseSlots - 1);
            }
            atomicAdd(&cnt[slot], 1u);
        }
    }
    __syncthreads();

    for (int i = threadIdx.x; i < kNoiseSlots; i += kNoiseThreads)
        if (keys[i] != kNoiseEmpty) atomicAdd(&acc->hist[0][0] + keys[i], cnt[i]);        // keys are below 64 * 512 by construction
    if (threadIdx.x < 64 && msum[threadIdx.x]) atomicAdd(&acc->msum[threadIdx.x], msum[threadIdx.x]);
    if (threadIdx.x < 3 && counters[threadIdx.x]) atomicAdd(&acc->counters[threadIdx.x], (unsigned long long)counters[threadIdx.x]);
}

}  // namespace

bool noise_wide(const float* packed, int ww) { return (ww & 3) == 0 && (reinterpret_cast<uintptr_t>(packed) & 15) == 0; }

int64_t noise_groups(int n, int hh, int ww, int64_t* blocks) {
    const int64_t per_plane = (int64_t)(hh / 8) * (ww / 8), planes = (int64_t)n * 4;      // n, hh, ww >= 0: below 2^56 and 2^33
    const int64_t most = 0x7fffffffll * kNoiseThreads;                                     // the blocks of 2^31 - 1 workgroups
    if (per_plane > 0 && planes > most / per_plane) return -1;
    const int64_t total = planes * per_plane;
    if (blocks) *blocks = total;
    return (total + kNoiseThreads - 1) / kNoiseThreads;
}

hipError_t launch_noise_hist(const float* packed, int n, int hh, int ww, int bit_depth, NoiseAcc* acc, hipStream_t s) {
    int64_t total = 0;
    const int64_t groups = noise_groups(n, hh, ww, &total);
    if (groups == 0) return hipSuccess;
    if (groups < 0 || !packed || !acc || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const float top = (float)((1u << bit_depth) - 1u);
    const float bin_scale = 64.0f / (float)(1u << bit_depth);          // a power of two
    if (noise_wide(packed, ww))
        hipLaunchKernelGGL(noise_hist_kernel<true>, dim3((unsigned)groups), dim3(kNoiseThreads), 0, s, packed, acc, hh, ww, hh / 8, ww / 8, total,
                           top, bin_scale);
    else
        hipLaunchKernelGGL(noise_hist_kernel<false>, dim3((unsigned)groups), dim3(kNoiseThreads), 0, s, packed, acc, hh, ww, hh / 8, ww / 8, total,
                           top, bin_scale);
    return hipGetLastError();
}
