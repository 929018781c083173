// The rule rows.hip (a line = a plane row) and cols.hip (a line = a plane column) share, once: the two files differ in where a line's
// samples lie and which threads hold them, not in what is computed.  Every includer is compiled -ffp-contract=off: each operation
// below is rounded to f32 on its own (the NumPy restatement is tests/line_ref.py).  File-local in both translation units, and free of
// loops over samples like dpc_rule.h: every kernel unrolls its own.
//
// Estimate.  A sample's d = x - median of its eight neighbours ACROSS the lines (line_neighbour: mirrored about the site, then about
// the plane's edge), gated by the noise curve at that median (line_key).  A used d is held as a 32-bit key that sorts as d does
// (sign bit flipped, negative values inverted); a sample outside the gate, or past the line's end, holds kLineNoKey -- no used d has
// that key (it is a NaN's), and no threshold below exceeds it.
//
// The median of a line's cnt used d (line_median) is exact and takes the same steps whatever the values: a frame of quantised DN is
// full of equal d, so nothing depends on how many keys are equal (no histogram, no LDS atomics).  The key of rank k = (cnt - 1) / 2
// is the largest P with |{key < P}| <= k; P is built from the top, two bits a round: the three thresholds prefix | (1, 2, 3) << b
// are counted at once -- one compare and one add per key and threshold, two 16-bit counts to a register (line_count_add /
// line_count_unpack; the caller keeps a wave's count below 2^16) -- and the digit is the number of thresholds with a count <= k.
// 16 rounds.  The key of rank cnt / 2 (cnt even) is the same key where |{key <= P}| >= k + 2, else the least key above P: one more
// round, a count and a minimum.  The offset is the midpoint of the two (line_midpoint).  A line with no used sample,
// or with fewer than half of its samples used, is skipped.  How the counts of a line's keys are gathered -- registers or LDS, one
// wave or four -- is the caller's: line_median takes it as two callables; line_group_count / line_group_above are the workgroup-wide
// form with the keys in registers, which rows.hip and green.hip share.
//
// Apply.  A thread owns the four planes of NC cells of a cell row (NC = 4: ww % 4 == 0 and 16-byte aligned tensors, 16-byte loads and
// stores; NC = 1 otherwise; the same arithmetic per sample, the same bits): line_load_cells / line_store_cells, and per cell
// line_take: the DN less the offset, added to the gray sum; norm_dn packs it again.  Which cells are skipped is each kernel's own.
#pragma once
#include "dpc_rule.h"      // dn_of, norm_dn, sort8

namespace {

constexpr unsigned kLineNoKey = 0xffffffffu;

inline float top_of(int bit_depth) { return (float)((1u << bit_depth) - 1u); }

// the index of the neighbour d lines from line i in a plane of n: mirrored about the site where i + d lies outside; in a plane of
// fewer than nine lines i - d may lie outside as well, and is then reflected about the plane's edge (-q -> q, n - 1 + q -> n - 1 - q)
__device__ __forceinline__ int line_neighbour(int i, int d, int n) {
    int q = i + d;
    if (q < 0 || q >= n) q = i - d;
    if (q < 0) q = -q;
    if (q >= n) q = 2 * (n - 1) - q;
    return q;
}

__device__ __forceinline__ unsigned line_key_of(float d) {
    const unsigned u = __float_as_uint(d);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float line_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// the gate: a site of x DN whose neighbours' middle is m -> the key of d = x - m, or kLineNoKey where d lies outside k_gate standard
// deviations of the noise curve at m (green.hip takes its four diagonal neighbours through here as well)
__device__ __forceinline__ unsigned line_gate(float x, float m, const RowsParams& P) {
    const float d = x - m;
    const float var = fmaxf(P.a * m - P.b, P.floor);
    return d * d <= P.k2 * var ? line_key_of(d) : kLineNoKey;
}

// nine DN across the lines in ascending distance, the site in the middle -> the key of the site's d, or kLineNoKey outside the gate
__device__ __forceinline__ unsigned line_key(const float (&w)[9], const RowsParams& P) {
    float v[8] = {w[0], w[1], w[2], w[3], w[5], w[6], w[7], w[8]};
    sort8(v);
    return line_gate(w[4], (v[3] + v[4]) * 0.5f, P);
}

// one key against NT <= 3 thresholds: |{key < t[0]}| in the low half of lo, t[1]'s in its high half, t[2]'s in hi
template <int NT>
__device__ __forceinline__ void line_count_add(unsigned key, const unsigned (&t)[NT], unsigned& lo, unsigned& hi) {
    static_assert(NT >= 1 && NT <= 3, "two counts below 2^16 in one register");
    lo += key < t[0] ? 1u : 0u;
    if constexpr (NT > 1) lo += key < t[1] ? 0x10000u : 0u;
    if constexpr (NT > 2) hi += key < t[2] ? 1u : 0u;
}

// lo and hi summed over all of a line's keys -> the NT counts
template <int NT>
__device__ __forceinline__ void line_count_unpack(unsigned lo, unsigned hi, unsigned (&out)[NT]) {
    out[0] = NT > 1 ? lo & 0xffffu : lo;
    if constexpr (NT > 1) out[1] = lo >> 16;
    if constexpr (NT > 2) out[2] = hi;
}

// |{key < t[n]}| over a workgroup of WAVES waves for NT <= 3 thresholds: every thread of the workgroup arrives, every thread gets the
// counts.  A thread counts its own KPT keys -- the caller keeps a wave's count below 2^16, so that two counts share a register --, the
// wave adds them up (DPP), lane 0 leaves them in LDS.  `words`: this round's LDS words [wave][2]; the caller alternates between two
// sets, which makes one barrier a round enough
template <int WAVES, int KPT, int NT>
__device__ __forceinline__ void line_group_count(const unsigned (&key)[KPT], const unsigned (&t)[NT], unsigned (*words)[2], int lane, int wave,
                                                 unsigned (&out)[NT]) {
    static_assert(KPT <= 32, "two counts below 2^16 in one register");
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int q = 0; q < KPT; ++q) line_count_add(key[q], t, lo, hi);
    lo = wave_sum_u32(lo);
    if constexpr (NT > 2) hi = wave_sum_u32(hi);
    if (lane == 0) {
        words[wave][0] = lo;
        if constexpr (NT > 2) words[wave][1] = hi;
    }
    __syncthreads();
    lo = hi = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        lo += words[w][0];
        if constexpr (NT > 2) hi += words[w][1];
    }
    line_count_unpack(lo, hi, out);
}

struct LineMedian {
    bool skipped;                // no used sample, or fewer than `half`
    unsigned prefix, upper;      // the keys of rank (cnt - 1) / 2 and cnt / 2
};
struct LineAbove {
    unsigned le, above;          // |{key <= P}| and the least key > P
};

// The search over one line's keys.  count(t, c): c[i] = |{key < t[i]}| for the 1 or 3 thresholds t; above(P) -> LineAbove.  Both run
// on every thread that searches the line and give each of them the line's totals
template <class Count, class Above>
__device__ __forceinline__ LineMedian line_median(unsigned half, Count count, Above above) {
    unsigned cnt;
    {
        const unsigned t[1] = {kLineNoKey};
        unsigned c[1];
        count(t, c);
        cnt = c[0];
    }
    if (cnt == 0 || cnt < half) return {true, 0, 0};                 // 2 cnt >= 2 half is not met
    const unsigned k = (cnt - 1) >> 1;
    unsigned prefix = 0;
#pragma unroll 1
    for (int b = 30; b >= 0; b -= 2) {
        const unsigned t[3] = {prefix | (1u << b), prefix | (2u << b), prefix | (3u << b)};
        unsigned c[3];
        count(t, c);
        const unsigned digit = (c[0] <= k ? 1u : 0u) + (c[1] <= k ? 1u : 0u) + (c[2] <= k ? 1u : 0u);      // the counts ascend
        prefix |= digit << b;
    }
    unsigned upper = prefix;
    if (!(cnt & 1)) {
        const LineAbove a = above(prefix);
        if (a.le < k + 2) upper = a.above;                           // rank k + 1 lies above the key of rank k
    }
    return {false, prefix, upper};
}

// |{key <= P}| and the least key > P over the workgroup's keys, gathered as line_group_count gathers its counts
template <int WAVES, int KPT>
__device__ __forceinline__ LineAbove line_group_above(const unsigned (&key)[KPT], unsigned prefix, unsigned (*words)[2], int lane, int wave) {
    unsigned le = 0, above = kLineNoKey;
#pragma unroll
    for (int q = 0; q < KPT; ++q) {
        le += key[q] <= prefix ? 1u : 0u;
        above = min(above, key[q] > prefix ? key[q] : kLineNoKey);
    }
    le = wave_sum_u32(le);
    above = ~wave_max_u32(~above);                                   // the wave's minimum
    if (lane == 0) {
        words[wave][0] = le;
        words[wave][1] = above;
    }
    __syncthreads();
    le = 0;
    above = kLineNoKey;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        le += words[w][0];
        above = min(above, words[w][1]);
    }
    return LineAbove{le, above};
}

__device__ __forceinline__ float line_midpoint(const LineMedian& m) { return (line_unkey(m.prefix) + line_unkey(m.upper)) * 0.5f; }

template <int NC>
__device__ __forceinline__ void line_load_cells(const float* p, float (&c)[NC]) {
    static_assert(NC == 1 || NC == 4, "one cell or four");
    if constexpr (NC == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(p);
        c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; c[3] = q[3];
    } else {
        c[0] = p[0];
    }
}

template <int NC>
__device__ __forceinline__ void line_store_cells(float* p, const float (&v)[NC]) {
    if constexpr (NC == 4) {
        const f32x4 q = {v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p) = q;
    } else {
        p[0] = v[0];
    }
}

// the gray cells of NC sites: a quarter of the four planes' sums g
template <int NC>
__device__ __forceinline__ void line_store_gray(float* p, const float (&g)[NC]) {
    if constexpr (NC == 4) {
        const f32x4 q = {g[0] * 0.25f, g[1] * 0.25f, g[2] * 0.25f, g[3] * 0.25f};
        *reinterpret_cast<f32x4*>(p) = q;
    } else {
        p[0] = g[0] * 0.25f;
    }
}

// cell c (packed) of plane k in DN less the offset o; it joins the gray sum g (plane 0 starts it).  The caller packs it again
// (norm_dn) where it writes the cell: cols.hip does so under its condition, which keeps the division out of the cells it leaves
__device__ __forceinline__ float line_take(float c, float o, float top, int k, float& g) {
    const float d = dn_of(c, top) - o;
    g = k ? g + d : d;
    return d;
}

}  // namespace
