// Device code of the Hamilton-Adams demosaic shared by demosaic.hip (the stand-alone kernels) and netin.hip (the demosaic
// inside the network input): the replicate-padded CFA, the green stencil (algo1), the 3x3 ring and red / blue from it (algo2),
// and the dispatch of a kernel template on the Bayer phase.  File-local in every translation unit that includes it.
#pragma once
#include "rvdd_internal.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float signf(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// CFA of a packed frame (util/Hamilton_Adam_demo.py:226-234), replicate
// padded: coordinates are clamped BEFORE the lookup.  Channel k of the packed
// frame is CFA position (k >> 1, k & 1) whatever the Bayer pattern; the pattern
// only decides which colour sits there.  With the phase PH = (py << 1) | px
// (bayer_phase: GBRG 0, BGGR 1, RGGB 2, GRBG 3) the colour site of full-
// resolution pixel (y, x) is the GBRG site of (y ^ py, x ^ px), i.e. its
// memory site XOR PH.  Memory addressing keeps (y & 1, x & 1); the demosaic's
// arithmetic is the same for every pattern, only the site selection moves.
// PH is a template parameter: the GBRG instantiations are the kernels as they
// were before the pattern existed.
struct Cfa {
    const float* raw;  // [4][h][w] of one frame
    int h, w, H, W;
    __device__ __forceinline__ float at(int y, int x) const {
        y = clampi(y, 0, H - 1);
        x = clampi(x, 0, W - 1);
        return raw[((size_t)(((y & 1) << 1) | (x & 1)) * h + (y >> 1)) * w + (x >> 1)];
    }
    // sparse colour plane `site` (GBRG sites: 0 = Gb, 1 = B, 2 = R, 3 = Gr), replicate padded
    template <int PH>
    __device__ __forceinline__ float plane(int y, int x, int site) const {
        y = clampi(y, 0, H - 1);
        x = clampi(x, 0, W - 1);
        const int s = ((y & 1) << 1) | (x & 1);
        return (s ^ PH) == site ? raw[((size_t)s * h + (y >> 1)) * w + (x >> 1)] : 0.f;
    }
};

// algo1 (util/Hamilton_Adam_demo.py:123-142)
// (`at`: the replicate-padded CFA as a function of the coordinates -- the frame in memory, or a copy of a tile of it in LDS)
template <int PH, class At>
__device__ __forceinline__ float ha_green_from(At at, int y, int x) {
    const float cc = at(y, x);
    float gval;
    if (((y ^ x ^ (PH >> 1) ^ PH) & 1) == 0) {      // y ^ x ^ py ^ px even: GBRG / GRBG's green diagonal, RGGB / BGGR's other one
        gval = cc;  // measured green
    } else {
        const float l1 = at(y, x - 1), r1 = at(y, x + 1), l2 = at(y, x - 2), r2 = at(y, x + 2);
        const float u1 = at(y - 1, x), d1 = at(y + 1, x), u2 = at(y - 2, x), d2 = at(y + 2, x);
        const float Kh = 0.5f * l1 + 0.5f * r1;
        const float Kv = 0.5f * u1 + 0.5f * d1;
        const float Dh = (l2 + (-2.f) * cc) + r2;
        const float Dv = (u2 + (-2.f) * cc) + d2;
        const float Fh = l1 + (-1.f) * r1;
        const float Fv = u1 + (-1.f) * d1;
        const float rawh = Kh - Dh / 4.f;
        const float rawv = Kv - Dv / 4.f;
        const float CLh = fabsf(Fh) + fabsf(Dh);
        const float CLv = fabsf(Fv) + fabsf(Dv);
        const float sg = signf(CLh - CLv);
        gval = (1.f + sg) * rawv / 2.f + (1.f - sg) * rawh / 2.f;
    }
    return gval;
}
template <int PH>
__device__ __forceinline__ float ha_green_at(const Cfa& c, int y, int x) {
    return ha_green_from<PH>([&](int yy, int xx) { return c.at(yy, xx); }, y, x);
}

// The 3x3 neighbourhood of a pixel in the green plane and in the CFA (replicate padded: coordinates clamped before the lookup),
// loaded UNCONDITIONALLY and together: algo2 below picks among them by the pixel's CFA site, and a load inside one of its four
// site branches was a memory round trip of its own (the branches diverge inside a wave: every path ran, each with its loads and
// its s_waitcnt vmcnt(0) -- 25 dependent round trips per pixel in netin_kernel, profiles/r06g_netin_load_batches.txt).
struct Ring {
    float g[3][3], r[3][3];
    int site[3][3];      // colour site of the (clamped) neighbour (GBRG numbering: the memory site XOR PH)
};
template <int PH>
__device__ __forceinline__ void load_ring(const Cfa& c, const float* __restrict__ gp, int H, int W, int y, int x, Ring& q) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int yy = clampi(y + dy - 1, 0, H - 1), xx = clampi(x + dx - 1, 0, W - 1);
            const int st = ((yy & 1) << 1) | (xx & 1);
            q.site[dy][dx] = st ^ PH;
            q.g[dy][dx] = gp[(size_t)yy * W + xx];
            q.r[dy][dx] = c.raw[((size_t)st * c.h + (yy >> 1)) * c.w + (xx >> 1)];
        }
}

// algo2 (util/Hamilton_Adam_demo.py:145-172) for red (k = 0) and blue (k = 1) at the ring's centre pixel (y, x)
template <int PH>
__device__ __forceinline__ void ha_red_blue(const Ring& q, int y, int x, float (&rb)[2]) {
    auto G = [&](int dy, int dx) { return q.g[dy + 1][dx + 1]; };
    // sparse colour plane `own` at a neighbour (Cfa::plane): the sample where the neighbour's site is `own`, zero elsewhere
    auto P = [&](int dy, int dx, int own) { return q.site[dy + 1][dx + 1] == own ? q.r[dy + 1][dx + 1] : 0.f; };
    const float g0 = q.g[1][1];
    const int site = (((y & 1) << 1) | (x & 1)) ^ PH;   // colour site: 0 Gb 1 B 2 R 3 Gr (GBRG: (e,e) (e,o) (o,e) (o,o))
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int own = k == 0 ? 2 : 1;          // the channel's own CFA site (R / B)
        const int hsite = k == 0 ? 3 : 0;        // sites with horizontal neighbours of the channel
        const int vsite = k == 0 ? 0 : 3;        // sites with vertical neighbours
        float v;
        if (site == own) {
            v = q.r[1][1];
        } else if (site == hsite) {
            const float Kh = 0.5f * P(0, -1, own) + 0.5f * P(0, 1, own);
            const float gD = (0.25f * G(0, -1) + (-0.5f) * g0) + 0.25f * G(0, 1);
            v = Kh - gD;
        } else if (site == vsite) {
            const float Kv = 0.5f * P(-1, 0, own) + 0.5f * P(1, 0, own);
            const float gD = (0.25f * G(-1, 0) + (-0.5f) * g0) + 0.25f * G(1, 0);
            v = Kv - gD;
        } else {  // mask_ochan site (B sites for red, R sites for blue): diagonal, hard selection
            const float a = P(-1, -1, own), d = P(1, 1, own);
            const float bq = P(-1, 1, own), cq = P(1, -1, own);
            const float Kp = 0.5f * a + 0.5f * d;
            const float Kn = 0.5f * bq + 0.5f * cq;
            const float Fp = (-1.f) * a + d;
            const float Fn = (-1.f) * bq + cq;
            const float gDp = (G(-1, -1) + (-2.f) * g0) + G(1, 1);
            const float gDn = (G(-1, 1) + (-2.f) * g0) + G(1, -1);
            const float Cp = Kp - gDp / 4.f;
            const float Cn = Kn - gDn / 4.f;
            const float CLp = fabsf(Fp) + fabsf(gDp);
            const float CLn = fabsf(Fn) + fabsf(gDn);
            const float sl = signf(CLp - CLn);
            v = (1.f + sl) * Cn / 2.f + (1.f - sl) * Cp / 2.f;
        }
        rb[k] = v;
    }
}

// enum rvdd_bayer -> the phase PH of the kernels' instantiations: (py << 1) | px, the row and column offset of the pattern
// from GBRG (GBRG (0,0), GRBG (1,1), RGGB (1,0), BGGR (0,1)); -1 for a value that is no pattern
constexpr int bayer_phase(int bayer) { return bayer == 0 ? 0 : bayer == 1 ? 3 : bayer == 2 ? 2 : bayer == 3 ? 1 : -1; }

// the instantiation of kernel template K for the phase of `bayer` (a hipError_t when it is no pattern)
#define RVDD_BAYER_DISPATCH(bayer, K, ...)                                           \
    switch (bayer_phase(bayer)) {                                                    \
    case 0: hipLaunchKernelGGL(K<0>, __VA_ARGS__); break;                            \
    case 1: hipLaunchKernelGGL(K<1>, __VA_ARGS__); break;                            \
    case 2: hipLaunchKernelGGL(K<2>, __VA_ARGS__); break;                            \
    case 3: hipLaunchKernelGGL(K<3>, __VA_ARGS__); break;                            \
    default: return hipErrorInvalidValue;                                            \
    }

}  // namespace
