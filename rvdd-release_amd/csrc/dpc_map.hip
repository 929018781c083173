// The static defect map (rvdd_dpc_detect, rvdd_dpc_map_apply; the stage rvdd_set_dpc_map puts behind the ingest of rvdd_video_push).
// Compiled -ffp-contract=off like dpc.hip: every operation below is rounded to f32 on its own, so that the counts and the written
// values are the bits of the NumPy restatement (tests/dpc_map_ref.py).  dn_of, norm_dn, the mirroring, the window and the sorted eight
// neighbours are dpc_rule.h's, the text dpc.hip uses.
//
// Detection: rvdd_dpc's rule per sample, with the largest / smallest neighbour replaced by the (tolerate + 1)-th largest / smallest, so
// the whole order of the eight is needed: all 19 exchanges of the sorting network.  A thread owns NC sites of one row of ONE plane
// across all n frames of the call -- the window of dpc_rule.h, the wide form (NC = 4) with 16-byte loads -- counts its sites' hot and
// dead frames in registers and folds them into `hits` once, with a plain load, add and store: nobody else touches those words, and
// launches are stream-ordered, so the totals do not depend on how the frames are split over calls.  No atomics, no LDS.
//
// Correction: one thread per (frame, defective cell), the only writer of that cell's four planes and of its gray value.  It reads
// good sites only (mask bit clear) and writes defective ones only: in place without a race, and a second application finds the same
// good values.  The order statistics of the q good values of a ring come from rank counting over the ring padded with +inf -- fully
// unrolled, no register array is indexed with a runtime value, nothing goes to scratch.
#include "dpc_rule.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned fold_hits(unsigned old, unsigned hot, unsigned dead) {      // both halves saturate at 65535
    const unsigned lo = min((old & 0xffffu) + min(hot, 0xffffu), 0xffffu), hi = min((old >> 16) + min(dead, 0xffffu), 0xffffu);
    return lo | hi << 16;
}

template <int NC>
__global__ void __launch_bounds__(64) dpc_detect_kernel(const float* __restrict__ pin, unsigned* __restrict__ hits, int n, int hh, int ww,
                                                        int tol, DpcParams P) {
    const int wq = ww / NC;
    const int64_t per = (int64_t)hh * wq, hw = (int64_t)hh * ww;      // threads per plane, sites per plane
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= 4 * per) return;
    const int k = (int)(t / per);
    const int64_t r = t % per;
    const int x = NC * (int)(r % wq), y = (int)(r / wq);
    const int yr[3] = {mirror_below(y), y, mirror_above(y + 1, hh)};
    const int xl = mirror_below(x), xr = mirror_above(x + NC, ww);      // the columns left and right of the thread's sites
    unsigned hot[NC], dead[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) hot[i] = dead[i] = 0;
#pragma unroll 1
    for (int f = 0; f < n; ++f) {
        const float* plane = pin + ((int64_t)f * 4 + k) * hw;
        float w[3][NC + 2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float c[NC];
            dpc_window_row<NC>(plane + (int64_t)yr[q] * ww, x, xl, xr, P.top, w[q], c);
        }
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            float s[8];
            const float m = dpc_neighbours<NC>(w, i, s), c = w[1][i + 1];
            const float var = fmaxf(P.a * m - P.b, P.floor);
            const float hi = tol == 0 ? s[7] : tol == 1 ? s[6] : tol == 2 ? s[5] : s[4];      // s[7 - tol], tol wave-uniform
            const float lo = tol == 0 ? s[0] : tol == 1 ? s[1] : tol == 2 ? s[2] : s[3];      // s[tol]
            const float dh = c - hi, dl = lo - c;
            hot[i] += P.k_hot > 0.0f && dh > 0.0f && dh * dh > P.k2_hot * var ? 1u : 0u;       // dpc_kernel's two tests, hi / lo for s[7] / s[0]
            dead[i] += P.k_dead > 0.0f && dl > 0.0f && dl * dl > P.k2_dead * var ? 1u : 0u;
        }
    }
    unsigned* dst = hits + (int64_t)k * hw + (int64_t)y * ww + x;
    if constexpr (NC == 4) {
        u32x4 v = *reinterpret_cast<const u32x4*>(dst);
        v[0] = fold_hits(v[0], hot[0], dead[0]);
        v[1] = fold_hits(v[1], hot[1], dead[1]);
        v[2] = fold_hits(v[2], hot[2], dead[2]);
        v[3] = fold_hits(v[3], hot[3], dead[3]);
        *reinterpret_cast<u32x4*>(dst) = v;
    } else {
        dst[0] = fold_hits(dst[0], hot[0], dead[0]);
    }
}

__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }      // about the plane's edge

// (s[(q - 1) / 2] + s[q / 2]) * 0.5 of the q >= 1 finite values among v[0 .. N), the other slots being +inf: rank_i = the number of
// j with v_j < v_i, or v_j == v_i and j < i -- a permutation of 0 .. N-1 in which the finite values hold the ranks below q
template <int N>
__device__ __forceinline__ float middle_of(const float (&v)[N], int q) {
    const int r1 = (q - 1) >> 1, r2 = q >> 1;
    float a = 0.0f, b = 0.0f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j != i) rank += (v[j] < v[i] || (j < i && v[j] == v[i])) ? 1 : 0;
        a = rank == r1 ? v[i] : a;
        b = rank == r2 ? v[i] : b;
    }
    return (a + b) * 0.5f;
}

__global__ void __launch_bounds__(64) dpc_map_apply_kernel(float* __restrict__ packed, float* __restrict__ gray,
                                                           const uint8_t* __restrict__ mask, const int* __restrict__ cells, int64_t ncells,
                                                           int n, int hh, int ww, float top) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= (int64_t)n * ncells) return;
    const int64_t f = t / ncells, hw = (int64_t)hh * ww;
    const int cell = cells[t % ncells];
    const int y = cell / ww, x = cell % ww;
    const unsigned bits = mask[cell];
    const float inf = __builtin_inff();
    int ys[5], xs[5];
#pragma unroll
    for (int d = 0; d < 5; ++d) {
        ys[d] = reflect(y + d - 2, hh);
        xs[d] = reflect(x + d - 2, ww);
    }
    // ring 1's mask bytes serve all four planes: one round trip of eight loads in front of the planes' own loads (hh * ww < 2^31)
    int at1[8];
    unsigned m1[8];
    {
        int i = 0;
#pragma unroll
        for (int dy = 1; dy <= 3; ++dy)
#pragma unroll
            for (int dx = 1; dx <= 3; ++dx) {
                if (dy == 2 && dx == 2) continue;
                at1[i] = ys[dy] * ww + xs[dx];
                m1[i] = mask[at1[i]];
                ++i;
            }
    }
    float g = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {            // unrolled: the loads of the four planes are in flight together
        float* plane = packed + (f * 4 + k) * hw;
        float* own = plane + (int64_t)y * ww + x;
        float d;
        if ((bits >> k) & 1u) {
            float v1[8];
            int q = 0, i = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const bool good = !((m1[j] >> k) & 1u);
                v1[j] = good ? dn_of(plane[at1[j]], top) : inf;
                q += good ? 1 : 0;
            }
            if (q) {
                d = middle_of<8>(v1, q);
                *own = norm_dn(d, top);
            } else {
                float v2[16];
                i = 0;
#pragma unroll
                for (int dy = 0; dy < 5; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 5; ++dx) {
                        if (dy > 0 && dy < 4 && dx > 0 && dx < 4) continue;
                        const int64_t at = (int64_t)ys[dy] * ww + xs[dx];
                        const bool good = !((mask[at] >> k) & 1u);
                        v2[i++] = good ? dn_of(plane[at], top) : inf;
                        q += good ? 1 : 0;
                    }
                if (q) {
                    d = middle_of<16>(v2, q);
                    *own = norm_dn(d, top);
                } else {
                    d = dn_of(*own, top);         // unfixable: the sample keeps its bits
                }
            }
        } else {
            d = dn_of(*own, top);
        }
        g = k ? g + d : d;
    }
    if (gray) gray[f * hw + cell] = g * 0.25f;
}

}  // namespace

bool dpc_detect_wide(const float* packed, const unsigned* hits, int ww) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(hits);
    return (ww & 3) == 0 && (al & 15) == 0;
}

int64_t dpc_detect_blocks(int hh, int ww, bool wide) {
    const int64_t per = (int64_t)hh * (wide ? ww >> 2 : ww);      // threads per plane, below 2^62: 4 * per threads in blocks of 64
    const int64_t blocks = (per + 15) / 16;
    return blocks > 0x7fffffffll ? -1 : blocks;
}

hipError_t launch_dpc_detect(const float* packed, int n, int hh, int ww, int bit_depth, const DpcParams& p, int tolerate, unsigned* hits,
                             hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!packed || !hits || hh < 2 || ww < 2 || bit_depth < 1 || bit_depth > 16 || tolerate < 0 || tolerate > 3) return hipErrorInvalidValue;
    const bool wide = dpc_detect_wide(packed, hits, ww);
    const int64_t blocks = dpc_detect_blocks(hh, ww, wide);
    if (blocks < 0) return hipErrorInvalidValue;
    DpcParams P = p;
    P.top = (float)((1u << bit_depth) - 1u);
    if (wide)
        hipLaunchKernelGGL(dpc_detect_kernel<4>, dim3((unsigned)blocks), dim3(64), 0, s, packed, hits, n, hh, ww, tolerate, P);
    else
        hipLaunchKernelGGL(dpc_detect_kernel<1>, dim3((unsigned)blocks), dim3(64), 0, s, packed, hits, n, hh, ww, tolerate, P);
    return hipGetLastError();
}

int64_t dpc_map_blocks(int n, int64_t ncells) {
    if (n <= 0 || ncells <= 0) return 0;
    if (ncells > (0x7fffffffll * 64) / n) return -1;
    return ((int64_t)n * ncells + 63) / 64;
}

hipError_t launch_dpc_map_apply(float* packed, float* gray, int n, int hh, int ww, int bit_depth, const uint8_t* mask, const int* cells,
                                int64_t ncells, hipStream_t s) {
    const int64_t blocks = dpc_map_blocks(n, ncells);
    if (blocks == 0) return hipSuccess;
    if (blocks < 0 || !packed || !mask || !cells || hh < 3 || ww < 3 || bit_depth < 1 || bit_depth > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dpc_map_apply_kernel, dim3((unsigned)blocks), dim3(64), 0, s, packed, gray, mask, cells, ncells, n, hh, ww,
                       (float)((1u << bit_depth) - 1u));
    return hipGetLastError();
}
