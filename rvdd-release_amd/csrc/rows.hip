// Row noise (banding) of packed raw frames: one offset per frame, row parity and plane row estimated (rvdd_rows_estimate) and taken
// out in place (rvdd_rows_apply); the stage rvdd_set_rows puts behind rvdd_set_dpc in rvdd_video_push.  The rule is in
// include/rvdd.h, its device form -- the gated key, the digit-wise median search, the per-cell step -- in line_noise.h, which
// cols.hip shares.  Compiled -ffp-contract=off like dpc.hip: every operation is rounded to f32 on its own, so that offsets, states,
// counts and the written samples are the bits of the NumPy restatement (tests/rows_ref.py).  What is this file's own:
//
// Estimate.  One workgroup of 256 threads owns one (frame, parity, plane row): the 2 ww samples of planes 2j and 2j + 1, sample s on
// thread s % 256, KPT = ceil(2 ww / 256) <= 32 of them per thread.  Workgroup ((i * 2 + j) * hh + r) reads the rows r - 4 .. r + 4 in
// that order, so that workgroups next to each other read eight of their nine rows twice from L2 and a frame once from memory.  A
// sample's key stays in a register.  A round of the search counts in the thread's own registers (counting by ballots kept a hundred
// scalar pairs alive and spilled them), one DPP sum per wave, lane 0 of each wave leaves its counts in LDS, ONE barrier (the rounds
// alternate between two sets of LDS words), every thread adds the four waves' counts (line_noise.h's line_group_count).  The offset
// is clamped to +-max_dn and the row counted in the frame's accumulator.
//
// Apply.  A pure stream in place.  A row whose two offsets are zero is left after two loads; a plane whose offset is zero is read for
// the gray value and not written.
#include "../../include/rvdd.h"
#include "line_noise.h"

namespace {

constexpr int kRowsThreads = kLineApplyThreads;
constexpr int kRowsWaves = kRowsThreads / 64;
constexpr int kRowsMaxKeys = 32;                                     // keys per thread at most: 2 ww <= 256 * 32

template <int KPT>
__global__ void __launch_bounds__(kRowsThreads) rows_estimate_kernel(const float* __restrict__ packed, float* __restrict__ offsets,
                                                                      unsigned char* __restrict__ state, rvdd_rows_acc* __restrict__ acc,
                                                                      int hh, int ww, RowsParams P) {
    __shared__ unsigned words[2][kRowsWaves][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned row = blockIdx.x;                                 // (frame * 2 + parity) * hh + r
    const int r = (int)(row % (unsigned)hh);
    const unsigned ij = row / (unsigned)hh;
    const int64_t hw = (int64_t)hh * ww;
    const float* pl = packed + ((int64_t)(ij >> 1) * 4 + 2 * (ij & 1)) * hw;      // plane 2j of the frame; plane 2j + 1 lies hw behind
    // the nine rows in ascending dr; uniform
    int64_t at[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) at[e] = (int64_t)(e == 4 ? r : line_neighbour(r, e - 4, hh)) * ww;

    unsigned key[KPT];
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        const int s = tid + q * kRowsThreads;
        unsigned k = kLineNoKey;
        if (s < 2 * ww) {
            const float* col = s < ww ? pl + s : pl + hw + (s - ww);
            float w[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) w[e] = dn_of(col[at[e]], P.top);
            k = line_key(w, P);
        }
        key[q] = k;
    }

    int phase = 0;
    const LineMedian med = line_median(
        (unsigned)ww,
        [&](const auto& t, auto& c) {
            line_group_count<kRowsWaves>(key, t, words[phase], lane, wave, c);      // four waves of at most 2048 each
            phase ^= 1;
        },
        [&](unsigned prefix) { return line_group_above<kRowsWaves>(key, prefix, words[phase], lane, wave); });
    if (med.skipped) {                                               // uniform
        if (tid == 0) {
            offsets[row] = 0.0f;
            state[row] = 0;
            if (acc) atomicAdd(&acc[ij >> 1].skipped, 1u);
        }
        return;
    }
    if (tid == 0) {
        const float o = line_midpoint(med);
        const float oc = fminf(fmaxf(o, -P.max_dn), P.max_dn);
        const bool clamped = oc != o;
        offsets[row] = oc;
        state[row] = clamped ? 2 : 1;
        if (acc) {
            rvdd_rows_acc* a = acc + (ij >> 1);
            atomicAdd(&a->applied, 1u);
            if (clamped) atomicAdd(&a->clamped, 1u);
            const long long q = (long long)(int)rintf(oc * 16.0f);
            if (q) atomicAdd(reinterpret_cast<unsigned long long*>(&a->sum_q2), (unsigned long long)(q * q));
        }
    }
}

template <int NC>
__global__ void __launch_bounds__(kRowsThreads) rows_apply_kernel(float* __restrict__ packed, float* __restrict__ gray,
                                                                   const float* __restrict__ offsets, int hh, int ww, unsigned bpf, float top) {
    const unsigned img = blockIdx.x / bpf;
    const int64_t t = (int64_t)(blockIdx.x % bpf) * kRowsThreads + threadIdx.x;      // the thread inside its frame
    const int wq = ww / NC;
    if (t >= (int64_t)hh * wq) return;
    const int x = NC * (int)(t % wq), y = (int)(t / wq);
    const float o2[2] = {offsets[((int64_t)img * 2) * hh + y], offsets[((int64_t)img * 2 + 1) * hh + y]};
    if (o2[0] == 0.0f && o2[1] == 0.0f) return;                      // the row keeps its bits, its gray row is not written
    const int64_t hw = (int64_t)hh * ww;
    float g[NC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float o = o2[k >> 1];
        float* p = packed + ((int64_t)img * 4 + k) * hw + (int64_t)y * ww + x;
        float c[NC], v[NC];
        line_load_cells<NC>(p, c);
#pragma unroll
        for (int i = 0; i < NC; ++i) v[i] = norm_dn(line_take(c[i], o, top, k, g[i]), top);
        if (o != 0.0f) line_store_cells<NC>(p, v);
    }
    if (gray) line_store_gray<NC>(gray + (int64_t)img * hw + (int64_t)y * ww + x, g);
}

template <int KPT>
void rows_estimate_go(unsigned blocks, hipStream_t s, const float* packed, float* offsets, uint8_t* state, rvdd_rows_acc* acc, int hh, int ww,
                      const RowsParams& P) {
    hipLaunchKernelGGL(rows_estimate_kernel<KPT>, dim3(blocks), dim3(kRowsThreads), 0, s, packed, offsets, state, acc, hh, ww, P);
}

}  // namespace

int rows_max_ww() { return kRowsThreads * kRowsMaxKeys / 2; }

int64_t rows_estimate_blocks(int n, int hh) {
    const int64_t blocks = (int64_t)n * 2 * hh;
    return blocks > 0x7fffffffll ? -1 : blocks;
}

hipError_t launch_rows_estimate(const float* packed, int n, int hh, int ww, int bit_depth, const RowsParams& p, float* offsets, uint8_t* state,
                                rvdd_rows_acc* acc, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !offsets || !state || hh < 5 || ww < 1 || ww > rows_max_ww() || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const int64_t blocks = rows_estimate_blocks(n, hh);
    if (blocks < 0) return hipErrorInvalidValue;
    RowsParams P = p;
    P.top = top_of(bit_depth);
    const int need = (2 * ww + kRowsThreads - 1) / kRowsThreads;     // keys per thread
    const unsigned b = (unsigned)blocks;
    if (need <= 1) rows_estimate_go<1>(b, s, packed, offsets, state, acc, hh, ww, P);
    else if (need <= 2) rows_estimate_go<2>(b, s, packed, offsets, state, acc, hh, ww, P);
    else if (need <= 4) rows_estimate_go<4>(b, s, packed, offsets, state, acc, hh, ww, P);
    else if (need <= 6) rows_estimate_go<6>(b, s, packed, offsets, state, acc, hh, ww, P);
    else if (need <= 8) rows_estimate_go<8>(b, s, packed, offsets, state, acc, hh, ww, P);
    else if (need <= 16) rows_estimate_go<16>(b, s, packed, offsets, state, acc, hh, ww, P);
    else rows_estimate_go<kRowsMaxKeys>(b, s, packed, offsets, state, acc, hh, ww, P);
    return hipGetLastError();
}

hipError_t launch_rows_apply(float* packed, float* gray, const float* offsets, int n, int hh, int ww, int bit_depth, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !offsets || hh < 1 || ww < 1 || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const bool wide = line_apply_wide(ww, packed, gray);
    int64_t bpf = 0;
    const int64_t blocks = line_apply_blocks(n, hh, ww, wide, &bpf);
    if (blocks < 0) return hipErrorInvalidValue;
    const float top = top_of(bit_depth);
    if (wide)
        hipLaunchKernelGGL(rows_apply_kernel<4>, dim3((unsigned)blocks), dim3(kRowsThreads), 0, s, packed, gray, offsets, hh, ww, (unsigned)bpf, top);
    else
        hipLaunchKernelGGL(rows_apply_kernel<1>, dim3((unsigned)blocks), dim3(kRowsThreads), 0, s, packed, gray, offsets, hh, ww, (unsigned)bpf, top);
    return hipGetLastError();
}
