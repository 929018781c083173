// Device code of the defective-pixel rule shared by dpc.hip (rvdd_dpc: flag and replace) and dpc_map.hip (rvdd_dpc_detect: count the
// flags per site), and the DN <-> packed conversion that ingest.hip and noise.hip use as well: the edge mirroring, a row of the
// window of a thread's sites, the sorted eight neighbours and their median.  The two threshold tests on top of these stay written out
// in each kernel: no shared form of them compiled to the instructions both kernels had.  Every includer is compiled
// -ffp-contract=off: each operation below is rounded to f32 on its own.  The pieces are free of loops on purpose -- a loop in here is
// unrolled before it is inlined, which reorders the kernels' instructions.  File-local in every translation unit that includes it.
#pragma once
#include "rvdd_internal.h"

namespace {

// dn = ((v + 1) * 0.5) * top, and back: packed = 2 * (dn / maxv) - 1, the division correctly rounded, then the product, then the difference
__device__ __forceinline__ float dn_of(float v, float top) { return ((v + 1.0f) * 0.5f) * top; }
__device__ __forceinline__ float norm_dn(float dn, float maxv) { return 2.0f * __fdiv_rn(dn, maxv) - 1.0f; }

__device__ __forceinline__ void cex(float& a, float& b) {
    const float lo = fminf(a, b), hi = fmaxf(a, b);
    a = lo;
    b = hi;
}

// eight values in any order -> ascending: the 19 compare-exchanges of the optimal 8-input sorting network (exchanges whose results
// the caller does not read fall away in the compiler)
__device__ __forceinline__ void sort8(float v[8]) {
    cex(v[0], v[2]); cex(v[1], v[3]); cex(v[4], v[6]); cex(v[5], v[7]);
    cex(v[0], v[4]); cex(v[1], v[5]); cex(v[2], v[6]); cex(v[3], v[7]);
    cex(v[0], v[1]); cex(v[2], v[3]); cex(v[4], v[5]); cex(v[6], v[7]);
    cex(v[2], v[4]); cex(v[3], v[5]);
    cex(v[1], v[4]); cex(v[3], v[6]);
    cex(v[1], v[2]); cex(v[3], v[4]); cex(v[5], v[6]);
}

// An index one outside a plane of n, mirrored about the site it belongs to: -1 -> +1, n -> n - 2 (i is the site's index - 1, or + 1 and on)
__device__ __forceinline__ int mirror_below(int i) { return i > 0 ? i - 1 : 1; }
__device__ __forceinline__ int mirror_above(int i, int n) { return i < n ? i : n - 2; }

// One row of the window of NC neighbouring sites x .. x + NC - 1: c the sites as stored, w the NC + 2 values from column xl to column xr
// in DN.  NC == 4 (ww % 4 == 0, 16-byte aligned plane) loads the sites as one 16-byte vector.  The caller loops over the three rows;
// no loop in here, so that every kernel unrolls its own loops itself.
template <int NC>
__device__ __forceinline__ void dpc_window_row(const float* row, int x, int xl, int xr, float top, float (&w)[NC + 2], float (&c)[NC]) {
    static_assert(NC == 1 || NC == 4, "one site or four");
    if constexpr (NC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + x);
        c[0] = v[0]; c[1] = v[1]; c[2] = v[2]; c[3] = v[3];
    } else {
        c[0] = row[x];
    }
    w[0] = dn_of(row[xl], top);
    w[NC + 1] = dn_of(row[xr], top);
    w[1] = dn_of(c[0], top);
    if constexpr (NC == 4) {
        w[2] = dn_of(c[1], top); w[3] = dn_of(c[2], top); w[4] = dn_of(c[3], top);
    }
}

// site i of the window: its eight neighbours ascending in s, and their median
template <int NC>
__device__ __forceinline__ float dpc_neighbours(const float (&w)[3][NC + 2], int i, float (&s)[8]) {
    s[0] = w[0][i]; s[1] = w[0][i + 1]; s[2] = w[0][i + 2]; s[3] = w[1][i];
    s[4] = w[1][i + 2]; s[5] = w[2][i]; s[6] = w[2][i + 1]; s[7] = w[2][i + 2];
    sort8(s);
    return (s[3] + s[4]) * 0.5f;
}

}  // namespace
