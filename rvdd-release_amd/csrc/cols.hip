// Column fixed-pattern noise of packed raw frames: one offset per frame, column parity and plane column estimated (rvdd_cols_estimate),
// pooled over the frames on the host (rvdd_cols_fit, noise_fit.hip) and taken out in place as a static map (rvdd_cols_apply); the stage
// rvdd_set_cols puts behind rvdd_set_dpc in rvdd_video_push.  The rule is in include/rvdd.h, its device form -- the gated key, the
// digit-wise median search, the per-cell step -- in line_noise.h, which rows.hip shares.  Compiled -ffp-contract=off like rows.hip:
// every operation is rounded to f32 on its own, so that offsets, states and the written samples are the bits of the NumPy restatement
// (tests/cols_ref.py).  What is this file's own:
//
// Estimate.  A column's 2 hh samples lie ww floats apart, so a workgroup per column would read 4-byte words at a stride.  Instead a
// workgroup owns a STRIP of CB neighbouring plane columns of one (frame, parity): 64 min(CB, 16) threads, thread t on strip column
// t % CB for good -- its nine column indices (the site and the eight mirrored neighbours) are formed once -- walking the 2 hh rows of
// planes j and j + 2, a wave covering 64 / CB whole row segments of CB floats a step.  The eight neighbours are loaded like the site:
// lanes next to each other read words next to each other, and all but the halo of eight columns a strip are the workgroup's own
// sites, so they come from the vector cache.  The sample's key goes to LDS, column-major: keys[column][2 hh] at a pitch of 2 hh | 1
// words.  The pitch is ODD, so the CB lanes that write one row of the strip fall on CB different banks (ds_write_b32 banks are
// word % 32, CB <= 32), and the 64 lanes that read consecutive keys of one column read consecutive words: neither conflicts.
//
// After ONE barrier a wave owns a column (wave w the columns w, w + waves, ...) and runs the search over the column's keys from LDS:
// one DPP sum per wave and threshold pair, no barrier and no LDS word written in the search at all.
//
// CB is the largest of 32, 16, 8, 4 whose keys fit the 160 KiB of a CU: 4 CB (2 hh | 1) bytes, which gives 32 columns up to 639 rows,
// 16 up to 1279, 8 up to 2559, 4 up to the cap of 4096 rows (kColsMaxHH; a lane then counts 128 keys a round and a wave's count
// stays below 2^16, so that two counts share a register).  With CB < 16 a workgroup is CB waves: a wave per column in the search.
//
// Apply.  A pure stream in place, the offset indexed by column.  A sample whose column has a zero offset keeps the bits it was loaded
// with; a gray cell whose two offsets are zero is not written.
#include "../../include/rvdd.h"
#include "line_noise.h"

namespace {

constexpr int kColsMaxHH = 4096;
constexpr int kColsMaxThreads = 1024;
constexpr int kColsThreads = kLineApplyThreads;                      // the apply kernel's
constexpr size_t kColsLds = 160 * 1024;

// |{key < t[n]}| over one column's nk keys for NT <= 3 thresholds: every lane of the wave arrives, every lane gets the counts.  A lane
// counts the keys lane, lane + 64, ... -- at most 128, so that a wave's count stays below 2^16 and two counts share a register
template <int NT>
__device__ __forceinline__ void cols_count(const unsigned* __restrict__ col, int nk, int lane, const unsigned (&t)[NT], unsigned (&out)[NT]) {
    unsigned lo = 0, hi = 0;
#pragma unroll 4
    for (int q = lane; q < nk; q += 64) line_count_add(col[q], t, lo, hi);
    lo = wave_sum_u32(lo);
    if constexpr (NT > 2) hi = wave_sum_u32(hi);
    line_count_unpack(lo, hi, out);
}

// CB: the strip's columns (a power of two <= 32); blockDim.x = 64 * min(CB, 16); dynamic LDS: CB * pitch words, pitch = 2 hh | 1
__global__ void __launch_bounds__(kColsMaxThreads) cols_estimate_kernel(const float* __restrict__ packed, float* __restrict__ offsets,
                                                                         unsigned char* __restrict__ state, int hh, int ww, int cb_log2,
                                                                         unsigned strips, RowsParams P) {
    extern __shared__ unsigned cols_keys[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, waves = (int)blockDim.x >> 6;
    const int CB = 1 << cb_log2;
    const int nk = 2 * hh, pitch = nk | 1;
    const unsigned strip = blockIdx.x % strips, ij = blockIdx.x / strips;      // ij = frame * 2 + parity
    const int c0 = (int)strip * CB;
    const int64_t hw = (int64_t)hh * ww;
    const float* pl = packed + ((int64_t)(ij >> 1) * 4 + (ij & 1)) * hw;       // plane j of the frame; plane j + 2 lies 2 hw behind

    {   // the keys: this thread's column for good, the rows tid / CB, + threads / CB, ...
        const int sc = tid & (CB - 1), c = c0 + sc;
        if (c < ww) {
            int at[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) at[e] = e == 4 ? c : line_neighbour(c, e - 4, ww);
            unsigned* mine = cols_keys + sc * pitch;
            const int step = (int)blockDim.x >> cb_log2;
            for (int s = tid >> cb_log2; s < nk; s += step) {
                const float* row = s < hh ? pl + (int64_t)s * ww : pl + 2 * hw + (int64_t)(s - hh) * ww;
                float w[9];
#pragma unroll
                for (int e = 0; e < 9; ++e) w[e] = dn_of(row[at[e]], P.top);
                mine[s] = line_key(w, P);
            }
        }
    }
    __syncthreads();

    for (int sc = wave; sc < CB && c0 + sc < ww; sc += waves) {      // uniform in the wave
        const unsigned* col = cols_keys + sc * pitch;
        const int64_t out = (int64_t)ij * ww + c0 + sc;
        const LineMedian med = line_median(
            (unsigned)hh, [&](const auto& t, auto& c) { cols_count(col, nk, lane, t, c); },
            [&](unsigned prefix) {
                unsigned le = 0, above = kLineNoKey;
#pragma unroll 4
                for (int q = lane; q < nk; q += 64) {
                    const unsigned key = col[q];
                    le += key <= prefix ? 1u : 0u;
                    above = min(above, key > prefix ? key : kLineNoKey);
                }
                return LineAbove{wave_sum_u32(le), ~wave_max_u32(~above)};      // the wave's sum and minimum
            });
        if (med.skipped) {
            if (lane == 0) {
                offsets[out] = 0.0f;
                state[out] = 0;
            }
            continue;
        }
        if (lane == 0) {
            offsets[out] = line_midpoint(med);
            state[out] = 1;
        }
    }
}

template <int NC>
__global__ void __launch_bounds__(kColsThreads) cols_apply_kernel(float* __restrict__ packed, float* __restrict__ gray,
                                                                   const float* __restrict__ map, int hh, int ww, unsigned bpf, float top) {
    const unsigned img = blockIdx.x / bpf;
    const int64_t t = (int64_t)(blockIdx.x % bpf) * kColsThreads + threadIdx.x;      // the thread inside its frame
    const int wq = ww / NC;
    if (t >= (int64_t)hh * wq) return;
    const int x = NC * (int)(t % wq), y = (int)(t / wq);
    float o2[2][NC];
    bool any = false;
    if constexpr (NC == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(map + x), b = *reinterpret_cast<const f32x4*>(map + ww + x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o2[0][i] = a[i];
            o2[1][i] = b[i];
        }
    } else {
        o2[0][0] = map[x];
        o2[1][0] = map[ww + x];
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) any = any || o2[0][i] != 0.0f || o2[1][i] != 0.0f;
    if (!any) return;                                                // the cells keep their bits, their gray cells are not written
    const int64_t hw = (int64_t)hh * ww;
    float g[NC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float(&o)[NC] = o2[k & 1];
        float* p = packed + ((int64_t)img * 4 + k) * hw + (int64_t)y * ww + x;
        float c[NC], v[NC];
        line_load_cells<NC>(p, c);
        bool hit = false;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const float d = line_take(c[i], o[i], top, k, g[i]);
            v[i] = o[i] != 0.0f ? norm_dn(d, top) : c[i];            // a column without an offset keeps its bits
            hit = hit || o[i] != 0.0f;
        }
        if (hit) line_store_cells<NC>(p, v);
    }
    if (gray) {
        float* gp = gray + (int64_t)img * hw + (int64_t)y * ww + x;
        if constexpr (NC == 4) {
            bool all = true;
#pragma unroll
            for (int i = 0; i < 4; ++i) all = all && (o2[0][i] != 0.0f || o2[1][i] != 0.0f);
            if (all) {
                line_store_gray<4>(gp, g);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (o2[0][i] != 0.0f || o2[1][i] != 0.0f) gp[i] = g[i] * 0.25f;
            }
        } else {
            line_store_gray<1>(gp, g);
        }
    }
}

}  // namespace

int cols_max_hh() { return kColsMaxHH; }

int cols_strip(int hh) {
    const size_t pitch = (size_t)(2 * hh) | 1;
    for (int cb = 32; cb > 4; cb >>= 1)
        if (4 * pitch * (size_t)cb <= kColsLds) return cb;
    return 4;
}

int64_t cols_estimate_blocks(int n, int hh, int ww) {
    const int cb = cols_strip(hh);
    const int64_t blocks = (int64_t)n * 2 * ((ww + cb - 1) / cb);
    return blocks > 0x7fffffffll ? -1 : blocks;
}

hipError_t launch_cols_estimate(const float* packed, int n, int hh, int ww, int bit_depth, const RowsParams& p, float* offsets, uint8_t* state,
                                hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !offsets || !state || hh < 1 || hh > kColsMaxHH || ww < 5 || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const int64_t blocks = cols_estimate_blocks(n, hh, ww);
    if (blocks < 0) return hipErrorInvalidValue;
    static std::atomic<uint64_t> attr_done{0};
    if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(cols_estimate_kernel), kColsLds, attr_done); e != hipSuccess) return e;
    RowsParams P = p;
    P.top = top_of(bit_depth);
    const int cb = cols_strip(hh);
    const int cb_log2 = cb == 32 ? 5 : cb == 16 ? 4 : cb == 8 ? 3 : 2;
    const size_t lds = 4 * ((size_t)(2 * hh) | 1) * (size_t)cb;
    const unsigned threads = 64u * (unsigned)(cb < 16 ? cb : 16);
    hipLaunchKernelGGL(cols_estimate_kernel, dim3((unsigned)blocks), dim3(threads), lds, s, packed, offsets, state, hh, ww, cb_log2,
                       (unsigned)((ww + cb - 1) / cb), P);
    return hipGetLastError();
}

hipError_t launch_cols_apply(float* packed, float* gray, const float* map, int n, int hh, int ww, int bit_depth, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !map || hh < 1 || ww < 1 || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const bool wide = line_apply_wide(ww, packed, gray, map);
    int64_t bpf = 0;
    const int64_t blocks = line_apply_blocks(n, hh, ww, wide, &bpf);
    if (blocks < 0) return hipErrorInvalidValue;
    const float top = top_of(bit_depth);
    if (wide)
        hipLaunchKernelGGL(cols_apply_kernel<4>, dim3((unsigned)blocks), dim3(kColsThreads), 0, s, packed, gray, map, hh, ww, (unsigned)bpf, top);
    else
        hipLaunchKernelGGL(cols_apply_kernel<1>, dim3((unsigned)blocks), dim3(kColsThreads), 0, s, packed, gray, map, hh, ww, (unsigned)bpf, top);
    return hipGetLastError();
}
