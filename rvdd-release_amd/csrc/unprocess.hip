// Raw datasets from sRGB video (reference: dataset/generate_raw_from_RGB.py:45-127, :168-189): one fused pointwise kernel
// from sRGB uint8 [n,H,W,3] to the linear camera image (f32 and uint16), its mosaic (the ground truth in the raw domain) and
// the noisy mosaic -- all HWC, the layout the reference writes -- and a second kernel that writes the two random planes alone.
//
// Compiled -ffp-contract=off: the reference evaluates the chain one f32 operation at a time (numpy, then torch, then numpy),
// and so do the draws below, which is what makes the fused path the bits of the path with supplied planes.
//
// Per pixel and channel:
//   v   = ((float)u8 + dither) / 266                 correctly rounded division (div_c, as srgb.hip)
//   v   = clamp(v, 0, 1)
//   t   = 0.5 - sin(asin(1 - 2 v) / 3)               inverse smoothstep
//   p   = pow(max(t, 1e-8), 2.2)                     gamma expansion
//   cam[k] = (p[0] * M[k][0] + p[1] * M[k][1]) + p[2] * M[k][2]          the CRVD rgb2cam matrix (:101)
//   y   = clamp(cam[k] * g[k], 0, 1)                 g: the inverted gains, three f32 values formed on the host
//   lin = y * 3855 + 240                             12 bits, black level 240
//   lin = A * (lin - 245) / 2060 + B                 percentile matching to CRVD: (A, B) = (3344, 266) / (3807, 268)
// lin_u16 = clip(rint(lin), 0, 4095); gt_raw = the mosaic of lin in the pattern (CFA position k = (k >> 1, k & 1) of a 2x2 cell,
// the packing of rvdd_ingest_raw's RVDD_RAW_PACKED_HWC); noisy = m + sqrt(max(ka * m - kb, 0)) * z.
//
// The draws are counter-based (Philox4x32-10), so a result depends on (seed, frame, element) alone -- not on the launch geometry,
// the wide or narrow form, or how frames are batched into calls.  key = (low, high) word of seed; counter = (element, stream,
// low, high word of the frame index).
//   stream 0, element = pixel y * W + x: dither of channel c = (w_c >> 8) * 2^-24 - 0.5          (exact in f32; w_3 unused)
//   stream 1, element = cell  y * (W/2) + x: u = ((w_0 >> 8) + 1) * 2^-24, v = (w_1 >> 8) * 2^-24, r = sqrt(-2 ln u),
//             (z_0, z_1) = (r cos 2 pi v, r sin 2 pi v); (z_2, z_3) the same from (w_2, w_3); z_k belongs to CFA position k.
// u >= 2^-24, so |z| <= sqrt(48 ln 2) = 5.77: the normal's tail ends at 5.77 sigma (probability 8e-9 per sample beyond it).
//
// unprocess_kernel<NC>: a thread owns NC neighbouring 2x2 cells of a cell row.  NC = 1 uses scalar accesses and takes any
// shape; NC = 2 (the wide form: W/2 % 4 == 0 and aligned pointers) reads a row's four pixels as three dwords (and three 16-byte
// vectors of dither) and writes three 16-byte vectors of lin_f32, three 8-byte vectors of lin_u16 and one 16-byte vector per
// cell of gt_raw / noisy.  Same bits either way.  VALU-bound: three asin, sin and pow per pixel, five Philox blocks per cell.
#include "rvdd_internal.h"

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

struct Words {
    uint32_t w[4];
};

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Words{{c0, c1, c2, c3}};
}

struct Draw {
    uint32_t k0, k1;        // seed
    uint32_t f0, f1;        // frame index
};

// the dither of pixel `pix` of the frame: three channels
__device__ __forceinline__ void draw_dither(const Draw& d, uint32_t pix, float o[3]) {
    const Words w = philox4x32_10(pix, 0u, d.f0, d.f1, d.k0, d.k1);
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (float)(w.w[c] >> 8) * 0x1p-24f - 0.5f;
}

// the four normals of cell `cell` of the frame, one per CFA position
__device__ __forceinline__ void draw_normal(const Draw& d, uint32_t cell, float z[4]) {
    const Words w = philox4x32_10(cell, 1u, d.f0, d.f1, d.k0, d.k1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float u = (float)((w.w[2 * i] >> 8) + 1u) * 0x1p-24f;
        const float v = (float)(w.w[2 * i + 1] >> 8) * 0x1p-24f;
        const float r = sqrtf(-2.0f * logf(u));
        float sn, cs;
        sincospif(2.0f * v, &sn, &cs);
        z[2 * i] = r * cs;
        z[2 * i + 1] = r * sn;
    }
}

// x / c, correctly rounded, for a divisor known at compile time (srgb.hip div_c: Markstein's sequence)
__device__ __forceinline__ float div_c(float x, float c, float rc) {
    const float q = x * rc;
    const float r = __builtin_fmaf(-c, q, x);
    return __builtin_fmaf(r, rc, q);
}
#define DIVC(x, c) div_c((x), (c), (float)(1.0 / (double)(c)))

struct UnprocessArgs {
    const uint8_t* srgb;
    const float* dither;    // [n,H,W,3] or NULL: drawn here
    const float* normal;    // [n,hh,ww,4] or NULL: drawn here
    float* lin_f32;
    uint16_t* lin_u16;
    float* gt_raw;
    float* noisy;
    int n, hh, ww;          // cells
    int cols;               // RGB plane of CFA position k, two bits each
    float g[3];
    float A, B, ka, kb;
    uint32_t k0, k1;
    int64_t frame0;
};

// one pixel: sRGB code values + dither -> linear camera values in DN
__device__ __forceinline__ void pixel(const UnprocessArgs& a, const float u8[3], const float d[3], float lin[3]) {
    float p[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = DIVC(u8[c] + d[c], 266.0f);
        v = fminf(fmaxf(v, 0.0f), 1.0f);
        const float t = 0.5f - sinf(DIVC(asinf(1.0f - 2.0f * v), 3.0f));
        p[c] = powf(fmaxf(t, 1e-8f), 2.2f);
    }
    const float cam[3] = {(p[0] * 0.95640505f + p[1] * 0.17353177f) + p[2] * -0.13219438f,
                          (p[0] * 0.14135948f + p[1] * 0.80402001f) + p[2] * 0.07771696f,
                          (p[0] * 0.05432832f + p[1] * 0.29852577f) + p[2] * 0.67210576f};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float y = fminf(fmaxf(cam[k] * a.g[k], 0.0f), 1.0f);
        const float l = y * 3855.0f + 240.0f;
        lin[k] = DIVC(a.A * (l - 245.0f), 2060.0f) + a.B;
    }
}

__device__ __forceinline__ unsigned to_u16(float v) { return (unsigned)fminf(fmaxf(rintf(v), 0.0f), 4095.0f); }

template <int NC>
__global__ void __launch_bounds__(256) unprocess_kernel(UnprocessArgs a) {
    const int wq = a.ww / NC;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)a.n * a.hh * wq) return;
    const int x = NC * (int)(t % wq);                 // first cell of the thread
    const int64_t row = t / wq;                       // img * hh + y
    const int y = (int)(row % a.hh);
    const int64_t img = row / a.hh;
    const int64_t W = 2 * (int64_t)a.ww;
    const uint64_t frame = (uint64_t)(a.frame0 + img);
    const Draw dr{a.k0, a.k1, (uint32_t)frame, (uint32_t)(frame >> 32)};
    constexpr int NP = 2 * NC;                        // pixels of a row
    float m[NC][4];                                   // the mosaic: CFA position k of each cell
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int64_t pix = (2 * (int64_t)y + r) * W + 2 * x;             // first pixel of the run, inside the frame
        const int64_t e = ((img * 2 * a.hh) * W + pix) * 3;               // its first element in the [n,H,W,3] arrays
        float u8[NP][3], d[NP][3], lin[NP][3];
        if constexpr (NC == 2) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(a.srgb + e);
            const uint32_t w3[3] = {s[0], s[1], s[2]};
#pragma unroll
            for (int i = 0; i < 12; ++i) u8[i / 3][i % 3] = (float)((w3[i >> 2] >> (8 * (i & 3))) & 255u);
        } else {
#pragma unroll
            for (int i = 0; i < 3 * NP; ++i) u8[i / 3][i % 3] = (float)a.srgb[e + i];
        }
        if (a.dither) {
            if constexpr (NC == 2) {
                const f32x4* s = reinterpret_cast<const f32x4*>(a.dither + e);
                const f32x4 v3[3] = {s[0], s[1], s[2]};
#pragma unroll
                for (int i = 0; i < 12; ++i) d[i / 3][i % 3] = v3[i >> 2][i & 3];
            } else {
#pragma unroll
                for (int i = 0; i < 3 * NP; ++i) d[i / 3][i % 3] = a.dither[e + i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < NP; ++i) draw_dither(dr, (uint32_t)(pix + i), d[i]);
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) pixel(a, u8[i], d[i], lin[i]);
        if (a.lin_f32) {
            if constexpr (NC == 2) {
                f32x4* o = reinterpret_cast<f32x4*>(a.lin_f32 + e);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = lin[(4 * q + j) / 3][(4 * q + j) % 3];
                    o[q] = v;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3 * NP; ++i) a.lin_f32[e + i] = lin[i / 3][i % 3];
            }
        }
        if (a.lin_u16) {
            if constexpr (NC == 2) {
                u32x2* o = reinterpret_cast<u32x2*>(a.lin_u16 + e);
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    unsigned h[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) h[j] = to_u16(lin[(4 * q + j) / 3][(4 * q + j) % 3]);
                    u32x2 v;
                    v[0] = h[0] | (h[1] << 16);
                    v[1] = h[2] | (h[3] << 16);
                    o[q] = v;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 3 * NP; ++i) a.lin_u16[e + i] = (uint16_t)to_u16(lin[i / 3][i % 3]);
            }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int k = 2 * r + (i & 1);
            const int col = (a.cols >> (2 * k)) & 3;
            m[i >> 1][k] = col == 0 ? lin[i][0] : col == 1 ? lin[i][1] : lin[i][2];
        }
    }
    if (!a.gt_raw && !a.noisy) return;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int64_t cell = (int64_t)y * a.ww + x + i;
        const int64_t o = (img * a.hh * a.ww + cell) * 4;
        if (a.gt_raw) {
            if constexpr (NC == 2) {
                f32x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = m[i][k];
                *reinterpret_cast<f32x4*>(a.gt_raw + o) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) a.gt_raw[o + k] = m[i][k];
            }
        }
        if (a.noisy) {
            float z[4];
            if (a.normal) {
                if constexpr (NC == 2) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(a.normal + o);
#pragma unroll
                    for (int k = 0; k < 4; ++k) z[k] = v[k];
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) z[k] = a.normal[o + k];
                }
            } else {
                draw_normal(dr, (uint32_t)cell, z);
            }
            float nz[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) nz[k] = m[i][k] + sqrtf(fmaxf(a.ka * m[i][k] - a.kb, 0.0f)) * z[k];
            if constexpr (NC == 2) {
                f32x4 v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = nz[k];
                *reinterpret_cast<f32x4*>(a.noisy + o) = v;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) a.noisy[o + k] = nz[k];
            }
        }
    }
}

// the two planes alone: one thread per cell, the same draws as the fused kernel makes
__global__ void __launch_bounds__(256) unprocess_draws_kernel(float* __restrict__ dither, float* __restrict__ normal, int n, int hh, int ww,
                                                              uint32_t k0, uint32_t k1, int64_t frame0) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * hh * ww) return;
    const int x = (int)(t % ww);
    const int64_t row = t / ww;
    const int y = (int)(row % hh);
    const int64_t img = row / hh;
    const int64_t W = 2 * (int64_t)ww;
    const uint64_t frame = (uint64_t)(frame0 + img);
    const Draw dr{k0, k1, (uint32_t)frame, (uint32_t)(frame >> 32)};
    if (dither) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t pix = (2 * (int64_t)y + (k >> 1)) * W + 2 * x + (k & 1);
            float d[3];
            draw_dither(dr, (uint32_t)pix, d);
            float* o = dither + ((img * 2 * hh) * W + pix) * 3;
            o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
        }
    }
    if (normal) {
        const int64_t cell = (int64_t)y * ww + x;
        float z[4];
        draw_normal(dr, (uint32_t)cell, z);
        float* o = normal + (img * hh * ww + cell) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = z[k];
    }
}

}  // namespace

hipError_t launch_unprocess(const uint8_t* srgb, int n, int hh, int ww, const float g[3], int iso, int bayer, const float* dither,
                            const float* normal, uint64_t seed, int64_t frame0, float* lin_f32, uint16_t* lin_u16, float* gt_raw, float* noisy,
                            hipStream_t s) {
    if (n <= 0 || (!lin_f32 && !lin_u16 && !gt_raw && !noisy)) return hipSuccess;
    if (bayer < 0 || bayer > 3 || (iso != 3200 && iso != 12800)) return hipErrorInvalidValue;
    UnprocessArgs a{};
    a.srgb = srgb; a.dither = dither; a.normal = normal;
    a.lin_f32 = lin_f32; a.lin_u16 = lin_u16; a.gt_raw = gt_raw; a.noisy = noisy;
    a.n = n; a.hh = hh; a.ww = ww;
    a.cols = bayer_cols(bayer);
    for (int k = 0; k < 3; ++k) a.g[k] = g[k];
    a.A = iso == 3200 ? 3344.0f : 3807.0f;
    a.B = iso == 3200 ? 266.0f : 268.0f;
    a.ka = iso == 3200 ? 8.0034f : 28.3015f;
    a.kb = iso == 3200 ? 2043.51144f : 6307.62081f;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
    a.frame0 = frame0;
    const uintptr_t al16 = reinterpret_cast<uintptr_t>(dither) | reinterpret_cast<uintptr_t>(normal) | reinterpret_cast<uintptr_t>(lin_f32) |
                           reinterpret_cast<uintptr_t>(gt_raw) | reinterpret_cast<uintptr_t>(noisy);
    const bool wide = (ww & 3) == 0 && (al16 & 15) == 0 && (reinterpret_cast<uintptr_t>(lin_u16) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(srgb) & 3) == 0;
    const int64_t work = (int64_t)n * hh * (wide ? ww >> 1 : ww);
    const int64_t blocks = (work + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (wide)
        hipLaunchKernelGGL(unprocess_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(unprocess_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_unprocess_draws(uint64_t seed, int64_t frame0, int n, int hh, int ww, float* dither, float* normal, hipStream_t s) {
    if (n <= 0 || (!dither && !normal)) return hipSuccess;
    const int64_t blocks = ((int64_t)n * hh * ww + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(unprocess_draws_kernel, dim3((unsigned)blocks), dim3(256), 0, s, dither, normal, n, hh, ww, (uint32_t)seed,
                       (uint32_t)(seed >> 32), frame0);
    return hipGetLastError();
}
