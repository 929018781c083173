// Dynamic defective-pixel correction of packed raw frames (rvdd_dpc; the stage rvdd_set_dpc puts between ingest and the slot ring of
// rvdd_video_push).  Compiled -ffp-contract=off like ingest.hip: every operation below is rounded to f32 on its own, so that the
// decisions and the written values are the bits of the NumPy restatement (tests/dpc_ref.py).
//
// Inside one channel plane of the packed layout the +-1 neighbours are the same-colour +-2 neighbours of the mosaic, so the rule
// knows neither the Bayer pattern nor the container.  Per sample: the 3x3 neighbourhood of its own plane in DN, indices outside the
// plane mirrored about the site (-1 -> +1, n -> n - 2), lo / hi / the median m of the eight neighbours, var = max(a m - b, floor);
// hot: c - hi = d > 0 and d d > k_hot^2 var, dead: lo - c = d > 0 and d d > k_dead^2 var (no square root).  A flagged sample becomes
// norm_dn(m); every other one is copied with its bits.  The gray plane of a cell with a flag is re-formed from the four DN values
// (m where flagged), the others are not touched.
//
// A thread owns the four planes of NC cells of a cell row: per plane a window of 3 rows x (NC + 2) columns in registers.  The wide
// form (NC = 4: ww % 4 == 0, 16-B aligned pointers) loads each row of the window as one 16-B vector and two single floats -- the 64
// lanes of a wave read 1 KiB runs of three rows of each plane, two of them from the cache once the row above has been through -- and
// stores one 16-B vector per plane; the one-cell form (NC = 1) serves every other shape.  Both run the same arithmetic per sample:
// same bits.  No LDS: a workgroup is ONE wave, so the reduction of the flag counts inside the wave is the workgroup's, and lane 0
// adds them to the frame's two counters with one atomic each (none where the count is zero).  A workgroup lies inside one frame.
#include "dpc_rule.h"

namespace {

template <int NC>
__global__ void __launch_bounds__(64) dpc_kernel(const float* __restrict__ pin, float* __restrict__ pout, float* __restrict__ gray,
                                                 unsigned* __restrict__ counts, int hh, int ww, unsigned bpf, DpcParams P) {
    const unsigned img = blockIdx.x / bpf;
    const int64_t t = (int64_t)(blockIdx.x % bpf) * 64 + threadIdx.x;       // the thread inside its frame
    const int wq = ww / NC;
    const int64_t hw = (int64_t)hh * ww;
    unsigned found = 0;                                  // hot samples | dead samples << 16 of this thread (at most 16 each)
    if (t < (int64_t)hh * wq) {
        const int x = NC * (int)(t % wq), y = (int)(t / wq);
        const int yr[3] = {mirror_below(y), y, mirror_above(y + 1, hh)};
        const int xl = mirror_below(x), xr = mirror_above(x + NC, ww);      // the columns left and right of the thread's cells
        float g[NC];                                     // the cell's gray: its DN per plane (the median where flagged) summed in plane order
        unsigned any = 0;                                // bit i: cell i has a flag in some plane
#pragma unroll 1
        for (int k = 0; k < 4; ++k) {                    // one plane at a time keeps the window's 3 x (NC + 2) values the only large live set
            const float* plane = pin + ((int64_t)img * 4 + k) * hw;
            float raw[NC], w[3][NC + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                float c[NC];
                dpc_window_row<NC>(plane + (int64_t)yr[r] * ww, x, xl, xr, P.top, w[r], c);
#pragma unroll
                for (int i = 0; i < NC; ++i)
                    if (r == 1) raw[i] = c[i];
            }
            float o[NC];
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                float s[8];
                const float m = dpc_neighbours<NC>(w, i, s), c = w[1][i + 1];
                const float var = fmaxf(P.a * m - P.b, P.floor);
                const float dh = c - s[7], dl = s[0] - c;
                const bool hot = P.k_hot > 0.0f && dh > 0.0f && dh * dh > P.k2_hot * var;
                const bool dead = P.k_dead > 0.0f && dl > 0.0f && dl * dl > P.k2_dead * var;
                found += (hot ? 1u : 0u) + (dead ? 0x10000u : 0u);
                any |= hot || dead ? 1u << i : 0u;
                const float dk = hot || dead ? m : c;
                g[i] = k ? g[i] + dk : dk;
                o[i] = hot || dead ? norm_dn(m, P.top) : raw[i];
            }
            float* dst = pout + ((int64_t)img * 4 + k) * hw + (int64_t)y * ww + x;
            if constexpr (NC == 4) {
                const f32x4 v = {o[0], o[1], o[2], o[3]};
                *reinterpret_cast<f32x4*>(dst) = v;
            } else {
                dst[0] = o[0];
            }
        }
        if (gray) {
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if ((any >> i) & 1) gray[(int64_t)img * hw + (int64_t)y * ww + x + i] = g[i] * 0.25f;
        }
    }
    if (!counts) return;
#pragma unroll
    for (int o = 32; o; o >>= 1) found += __shfl_xor(found, o);
    if (threadIdx.x == 0) {
        if (found & 0xffffu) atomicAdd(counts + 2 * (size_t)img, found & 0xffffu);
        if (found >> 16) atomicAdd(counts + 2 * (size_t)img + 1, found >> 16);
    }
}

}  // namespace

bool dpc_wide(const float* pin, const float* pout, const float* gray, int ww) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(pin) | reinterpret_cast<uintptr_t>(pout) | reinterpret_cast<uintptr_t>(gray);
    return (ww & 3) == 0 && (al & 15) == 0;
}

int64_t dpc_blocks(int n, int hh, int ww, bool wide, int64_t* per_frame) {
    const int64_t per = (int64_t)hh * (wide ? ww >> 2 : ww);      // threads per frame
    const int64_t bpf = (per + 63) / 64;
    if (per_frame) *per_frame = bpf;
    if (bpf > 0x7fffffffll || (bpf > 0 && n > 0x7fffffffll / bpf)) return -1;
    return n * bpf;
}

hipError_t launch_dpc(const float* pin, float* pout, float* gray, int n, int hh, int ww, int bit_depth, const DpcParams& p, unsigned* counts,
                      hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!pin || !pout || hh < 2 || ww < 2 || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    const bool wide = dpc_wide(pin, pout, gray, ww);
    int64_t bpf = 0;
    const int64_t blocks = dpc_blocks(n, hh, ww, wide, &bpf);
    if (blocks < 0) return hipErrorInvalidValue;
    DpcParams P = p;
    P.top = (float)((1u << bit_depth) - 1u);
    if (wide)
        hipLaunchKernelGGL(dpc_kernel<4>, dim3((unsigned)blocks), dim3(64), 0, s, pin, pout, gray, counts, hh, ww, (unsigned)bpf, P);
    else
        hipLaunchKernelGGL(dpc_kernel<1>, dim3((unsigned)blocks), dim3(64), 0, s, pin, pout, gray, counts, hh, ww, (unsigned)bpf, P);
    return hipGetLastError();
}
