// Sensor frames -> the inputs of a frame-step (packed raw in [-1, 1]) and of TV-L1 (gray plane in DN), the same gray plane of
// an output frame's re-mosaic (rvdd_gray_of_rgb), the way back -- an output frame as sensor frames (rvdd_egress) --, both
// directions on frames of bit-packed 10 / 12 / 14-bit samples (rvdd_ingest_bits, rvdd_egress_bits), and the
// small copy kernels rvdd_video_push composes its flow batch and its substituted frames with.  Compiled -ffp-contract=off: every operation below is rounded
// to f32 on its own, which is what makes the outputs the bits of the reference's loader (library.py load_image + the
// dataset's transform) and of library._gray on integer-valued frames.
//
// ingest_raw_kernel is a pure streaming kernel (2 B read, 4 B + 1 B written per CFA site for a u16 mosaic).  The fast form
// gives a thread FOUR neighbouring 2x2 cells of one cell row: for a mosaic it reads 16 B (u16) / 2 x 16 B (f32) from each of
// the two sensor rows, for the packed HWC layout 2 x 16 B (u16) / 4 x 16 B (f32) of one row, and writes one 16-B vector per
// packed channel and one for the gray plane -- so the 64 lanes of a wave read 1 KiB runs of each sensor row and write 1 KiB
// runs of each output plane.  It needs ww % 4 == 0 and 16-B aligned pointers; any other shape takes the one-cell form.
#include "dpc_rule.h"      // dn_of, norm_dn

namespace {

typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

// one 2x2 cell: c[k] = CFA position (k >> 1, k & 1) in DN
template <typename T, int LAYOUT>
__device__ __forceinline__ void load_cell(const T* __restrict__ f, int64_t img, int y, int x, int hh, int ww, float c[4]) {
    if constexpr (LAYOUT == 0) {
        const T* r0 = f + (img * 2 * hh + 2 * (int64_t)y) * (2 * (int64_t)ww) + 2 * x;
        const T* r1 = r0 + 2 * (int64_t)ww;
        c[0] = (float)r0[0]; c[1] = (float)r0[1]; c[2] = (float)r1[0]; c[3] = (float)r1[1];
    } else {
        const T* p = f + ((img * hh + y) * (int64_t)ww + x) * 4;
        c[0] = (float)p[0]; c[1] = (float)p[1]; c[2] = (float)p[2]; c[3] = (float)p[3];
    }
}

// four cells x .. x+3 of a cell row (x % 4 == 0, ww % 4 == 0, 16-B aligned base): c[i][k]
template <typename T, int LAYOUT>
__device__ __forceinline__ void load_cells4(const T* __restrict__ f, int64_t img, int y, int x, int hh, int ww, float c[4][4]) {
    if constexpr (LAYOUT == 0) {
        const T* r0 = f + (img * 2 * hh + 2 * (int64_t)y) * (2 * (int64_t)ww) + 2 * x;
        const T* r1 = r0 + 2 * (int64_t)ww;
        if constexpr (sizeof(T) == 2) {
            const u16x8 a = *reinterpret_cast<const u16x8*>(r0), b = *reinterpret_cast<const u16x8*>(r1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c[i][0] = (float)a[2 * i]; c[i][1] = (float)a[2 * i + 1];
                c[i][2] = (float)b[2 * i]; c[i][3] = (float)b[2 * i + 1];
            }
        } else {
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(r0), a1 = *reinterpret_cast<const f32x4*>(r0 + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(r1), b1 = *reinterpret_cast<const f32x4*>(r1 + 4);
            c[0][0] = a0[0]; c[0][1] = a0[1]; c[1][0] = a0[2]; c[1][1] = a0[3];
            c[2][0] = a1[0]; c[2][1] = a1[1]; c[3][0] = a1[2]; c[3][1] = a1[3];
            c[0][2] = b0[0]; c[0][3] = b0[1]; c[1][2] = b0[2]; c[1][3] = b0[3];
            c[2][2] = b1[0]; c[2][3] = b1[1]; c[3][2] = b1[2]; c[3][3] = b1[3];
        }
    } else {
        const T* p = f + ((img * hh + y) * (int64_t)ww + x) * 4;
        if constexpr (sizeof(T) == 2) {
            const u16x8 a = *reinterpret_cast<const u16x8*>(p), b = *reinterpret_cast<const u16x8*>(p + 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                c[0][k] = (float)a[k]; c[1][k] = (float)a[4 + k];
                c[2][k] = (float)b[k]; c[3][k] = (float)b[4 + k];
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(p + 4 * i);
                c[i][0] = v[0]; c[i][1] = v[1]; c[i][2] = v[2]; c[i][3] = v[3];
            }
        }
    }
}

// library._gray of a 4-channel frame: the f32 sum in channel order, left to right, times 0.25
__device__ __forceinline__ float gray_dn(const float c[4]) { return (((c[0] + c[1]) + c[2]) + c[3]) * 0.25f; }

template <typename T, int LAYOUT, bool VEC>
__global__ void __launch_bounds__(256) ingest_raw_kernel(const T* __restrict__ frames, float* __restrict__ packed, float* __restrict__ gray,
                                                         int n, int hh, int ww, float maxv) {
    const int64_t hw = (int64_t)hh * ww;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (VEC) {
        const int wq = ww >> 2;
        if (t >= (int64_t)n * hh * wq) return;
        const int xq = (int)(t % wq);
        const int64_t row = t / wq;              // img * hh + y
        const int y = (int)(row % hh);
        const int64_t img = row / hh;
        float c[4][4];
        load_cells4<T, LAYOUT>(frames, img, y, 4 * xq, hh, ww, c);
        const int64_t o = (int64_t)y * ww + 4 * xq;
        if (packed) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = norm_dn(c[i][k], maxv);
                *reinterpret_cast<f32x4*>(packed + (img * 4 + k) * hw + o) = v;
            }
        }
        if (gray) {
            f32x4 g;
#pragma unroll
            for (int i = 0; i < 4; ++i) g[i] = gray_dn(c[i]);
            *reinterpret_cast<f32x4*>(gray + img * hw + o) = g;
        }
    } else {
        if (t >= (int64_t)n * hw) return;
        const int x = (int)(t % ww);
        const int64_t row = t / ww;
        const int y = (int)(row % hh);
        const int64_t img = row / hh;
        float c[4];
        load_cell<T, LAYOUT>(frames, img, y, x, hh, ww, c);
        const int64_t o = (int64_t)y * ww + x;
        if (packed) {
#pragma unroll
            for (int k = 0; k < 4; ++k) packed[(img * 4 + k) * hw + o] = norm_dn(c[k], maxv);
        }
        if (gray) gray[img * hw + o] = gray_dn(c);
    }
}

template <typename T, int LAYOUT>
hipError_t launch_ingest_t(const T* frames, int n, int hh, int ww, float maxv, float* packed, float* gray, hipStream_t s) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(gray);
    const bool vec = (ww & 3) == 0 && (al & 15) == 0;
    const int64_t work = vec ? (int64_t)n * hh * (ww >> 2) : (int64_t)n * hh * ww;
    const int64_t blocks = (work + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (vec)
        hipLaunchKernelGGL((ingest_raw_kernel<T, LAYOUT, true>), dim3((unsigned)blocks), dim3(256), 0, s, frames, packed, gray, n, hh, ww, maxv);
    else
        hipLaunchKernelGGL((ingest_raw_kernel<T, LAYOUT, false>), dim3((unsigned)blocks), dim3(256), 0, s, frames, packed, gray, n, hh, ww, maxv);
    return hipGetLastError();
}

// ---- rvdd_gray_of_rgb: the gray plane (DN) of an RGB frame's re-mosaic ---------------------------------------------------
// HamiltonAdam(pattern).remosaick picks, at CFA position k = (k >> 1, k & 1) of a 2x2 cell, the colour the pattern has there;
// `cols` carries those four plane indices, two bits each.  Per cell: dn_k = ((v_k + 1) * 0.5) * top, then ingest's gray_dn.
// Of the six plane-rows of a pair of pixel rows four are read (one colour per position), half of each used.  The wide form
// gives a thread four neighbouring cells of a cell row: 2 x 16 B from each of the four plane-rows, one 16-B store.

template <bool VEC>
__global__ void __launch_bounds__(256) gray_of_rgb_kernel(const float* __restrict__ rgb, float* __restrict__ gray, int n, int hh, int ww,
                                                          int cols, float top) {
    const int64_t W = 2 * (int64_t)ww, HW = 2 * (int64_t)hh * W;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    constexpr int NC = VEC ? 4 : 1;                  // cells per thread
    const int wq = ww / NC;
    if (t >= (int64_t)n * hh * wq) return;
    const int x = NC * (int)(t % wq);
    const int64_t row = t / wq;                      // img * hh + y
    const int y = (int)(row % hh);
    const int64_t img = row / hh;
    float c[NC][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* p = rgb + (img * 3 + ((cols >> (2 * k)) & 3)) * HW + (2 * (int64_t)y + (k >> 1)) * W + 2 * x + (k & 1);
        if constexpr (VEC) {
            const float* a = p - (k & 1);            // the 16-B aligned run of eight pixels; position k takes its even / odd ones
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(a), v1 = *reinterpret_cast<const f32x4*>(a + 4);
            c[0][k] = dn_of(v0[k & 1], top); c[1][k] = dn_of(v0[2 + (k & 1)], top);
            c[2][k] = dn_of(v1[k & 1], top); c[3][k] = dn_of(v1[2 + (k & 1)], top);
        } else {
            c[0][k] = dn_of(p[0], top);
        }
    }
    float* g = gray + img * hh * ww + (int64_t)y * ww + x;
    if constexpr (VEC) {
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = gray_dn(c[i]);
        *reinterpret_cast<f32x4*>(g) = v;
    } else {
        g[0] = gray_dn(c[0]);
    }
}

// ---- rvdd_egress: a denoised frame in the containers a sensor pipeline reads ----------------------------------------------
// The inverse direction of ingest: dn = dn_of(v), written as it is (f32) or rounded half-to-even and clamped to 0 .. top (u16;
// the comparisons send NaN and -inf to 0, +inf to top), as interleaved RGB [n][H][W][3] (LAYOUT 0), as the re-mosaic in one
// plane [n][H][W] (1) or packed [n][H/2][W/2][4] (2).  Pure streaming: 12 B read per pixel for RGB, 4 B used (8 B fetched: the
// other half of every 16-B vector is another colour's site) for the mosaic layouts.  The wide form makes every access 16 B:
// RGB gives a thread 8 (u16) / 4 (f32) consecutive pixels of an image -- the planes and the interleaved output are both flat
// in the pixel index, so rows do not matter -- and its store is 3 x 16 B; the mosaic layouts give it four cells of a cell row,
// loaded as gray_of_rgb_kernel<true> loads them, and store one (u16) / two (f32) vectors per sensor row, twice that per packed
// run.  Both forms compute every sample with the same operations: same bits.
template <typename T>
__device__ __forceinline__ T out_of(float dn, float top) {
    if constexpr (sizeof(T) == 4) {
        return dn;
    } else {
        float r = rintf(dn);
        r = r > 0.0f ? r : 0.0f;
        r = r < top ? r : top;
        return (unsigned short)r;
    }
}

// N consecutive outputs as N * sizeof(T) / 16 vectors of 16 B (dst 16-B aligned)
template <typename T, int N>
__device__ __forceinline__ void store_run(T* __restrict__ dst, const float (&dn)[N], float top) {
    constexpr int PER = 16 / sizeof(T);
    typedef T vec_t __attribute__((ext_vector_type(PER)));
#pragma unroll
    for (int j = 0; j < N / PER; ++j) {
        vec_t v;
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] = out_of<T>(dn[j * PER + i], top);
        *reinterpret_cast<vec_t*>(dst + j * PER) = v;
    }
}

template <int LAYOUT, typename T, bool WIDE>
__global__ void __launch_bounds__(256) egress_kernel(const float* __restrict__ rgb, T* __restrict__ out, int n, int H, int W, int cols,
                                                     float top) {
    const int64_t HW = (int64_t)H * W;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (LAYOUT == 0) {
        constexpr int P = WIDE ? 16 / (int)sizeof(T) : 1;      // pixels per thread
        const int64_t q = HW / P;
        if (t >= (int64_t)n * q) return;
        const int64_t img = t / q, p = (t % q) * P;
        float dn[3 * P];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* src = rgb + (img * 3 + c) * HW + p;
            if constexpr (WIDE) {
#pragma unroll
                for (int j = 0; j < P / 4; ++j) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(src + 4 * j);
#pragma unroll
                    for (int i = 0; i < 4; ++i) dn[(4 * j + i) * 3 + c] = dn_of(v[i], top);
                }
            } else {
                dn[c] = dn_of(src[0], top);
            }
        }
        T* dst = out + (img * HW + p) * 3;
        if constexpr (WIDE) {
            store_run<T, 3 * P>(dst, dn, top);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = out_of<T>(dn[c], top);
        }
    } else {
        constexpr int NC = WIDE ? 4 : 1;                 // cells per thread
        const int hh = H >> 1, ww = W >> 1, wq = ww / NC;
        if (t >= (int64_t)n * hh * wq) return;
        const int x = NC * (int)(t % wq);
        const int64_t row = t / wq;                      // img * hh + y
        const int y = (int)(row % hh);
        const int64_t img = row / hh;
        float c[NC][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float* p = rgb + (img * 3 + ((cols >> (2 * k)) & 3)) * HW + (2 * (int64_t)y + (k >> 1)) * W + 2 * x + (k & 1);
            if constexpr (WIDE) {
                const float* a = p - (k & 1);            // the 16-B aligned run of eight pixels; position k takes its even / odd ones
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(a), v1 = *reinterpret_cast<const f32x4*>(a + 4);
                c[0][k] = dn_of(v0[k & 1], top); c[1][k] = dn_of(v0[2 + (k & 1)], top);
                c[2][k] = dn_of(v1[k & 1], top); c[3][k] = dn_of(v1[2 + (k & 1)], top);
            } else {
                c[0][k] = dn_of(p[0], top);
            }
        }
        if constexpr (LAYOUT == 1) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                float run[2 * NC];                       // sensor row 2y + r, sites 2x .. 2x + 2 NC - 1
#pragma unroll
                for (int i = 0; i < NC; ++i) { run[2 * i] = c[i][2 * r]; run[2 * i + 1] = c[i][2 * r + 1]; }
                T* dst = out + (img * H + 2 * (int64_t)y + r) * W + 2 * x;
                if constexpr (WIDE) {
                    store_run<T, 2 * NC>(dst, run, top);
                } else {
                    dst[0] = out_of<T>(run[0], top); dst[1] = out_of<T>(run[1], top);
                }
            }
        } else {
            float run[4 * NC];
#pragma unroll
            for (int i = 0; i < NC; ++i)
#pragma unroll
                for (int k = 0; k < 4; ++k) run[4 * i + k] = c[i][k];
            T* dst = out + ((img * hh + y) * (int64_t)ww + x) * 4;
            if constexpr (WIDE) {
                store_run<T, 4 * NC>(dst, run, top);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) dst[k] = out_of<T>(run[k], top);
            }
        }
    }
}

template <int LAYOUT, typename T>
hipError_t launch_egress_t(const float* rgb, int n, int H, int W, int cols, float top, T* out, bool wide, int64_t blocks, hipStream_t s) {
    if (wide)
        hipLaunchKernelGGL((egress_kernel<LAYOUT, T, true>), dim3((unsigned)blocks), dim3(256), 0, s, rgb, out, n, H, W, cols, top);
    else
        hipLaunchKernelGGL((egress_kernel<LAYOUT, T, false>), dim3((unsigned)blocks), dim3(256), 0, s, rgb, out, n, H, W, cols, top);
    return hipGetLastError();
}

template <int LAYOUT>
hipError_t launch_egress_l(const float* rgb, int n, int H, int W, int cols, float top, int dtype, void* out, bool wide, int64_t blocks,
                           hipStream_t s) {
    return dtype == 0 ? launch_egress_t<LAYOUT>(rgb, n, H, W, cols, top, static_cast<unsigned short*>(out), wide, blocks, s)
                      : launch_egress_t<LAYOUT>(rgb, n, H, W, cols, top, static_cast<float*>(out), wide, blocks, s);
}

// ---- rvdd_ingest_bits / rvdd_egress_bits: the same two directions on frames of packed 10 / 12 / 14-bit samples ----------------
// ORDER 0 (RVDD_BITS_MIPI, CSI-2 RAW10 / RAW12 / RAW14): groups of G = 4 (2 at 12 bits) pixels, G bytes of the samples' upper
// eight bits, then G (b - 8) / 8 bytes of their lower bits, pixel 0's lowest.  ORDER 1 (RVDD_BITS_MSB, TIFF FillOrder 1): the
// samples b bits each, most significant bit first, as one bit string per row.  In both, 4 pixels are b / 2 whole bytes (5 / 6 / 7)
// and 16 pixels 2 b bytes (20 / 24 / 28), a whole number of dwords.
// A thread takes NC cells of a cell row: from each of the two sensor rows it holds the NC * 2 * b / 8 bytes of its 2 NC pixels as
// a WINDOW of dwords in registers, byte i at bits 8 (i & 3) of word i >> 2 -- the little-endian image of the bytes.  The
// general form (NC = 2) moves the window byte by byte and touches no byte at or beyond row_bytes (an odd ww ends a row inside
// the last window: the missing samples are not written on the way in and are zero -- the pad bits -- on the way out); the fast
// form (NC = 8, ww % 8 == 0, rows on dword boundaries) moves it as 5 / 6 / 7 dwords, so a wave reads or writes one run of 1280 /
// 1536 / 1792 bytes per sensor row.  Between window and samples both forms run the same code with every index a constant after
// unrolling (registers only: no LDS, no scratch); the per-sample arithmetic is ingest_raw_kernel's and egress_kernel's own.
template <int NW>
__device__ __forceinline__ unsigned window_byte(const unsigned (&w)[NW], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// sample j of the window, j = 0 .. NS - 1
template <int BITS, int ORDER, int NS, int NW>
__device__ __forceinline__ void unpack_window(const unsigned (&w)[NW], unsigned (&s)[NS]) {
    constexpr int LOW = BITS - 8;
    if constexpr (ORDER == 0) {
        constexpr int G = BITS == 12 ? 2 : 4, GB = G * BITS / 8;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int base = (j / G) * GB, k = j % G;
            const int q = 8 * (base + G) + k * LOW;      // where the sample's lower bits start, counted in the little-endian window
            unsigned lo = w[q >> 5] >> (q & 31);
            if ((q & 31) + LOW > 32) lo |= w[(q >> 5) + 1] << (32 - (q & 31));
            s[j] = (window_byte(w, base + k) << LOW) | (lo & ((1u << LOW) - 1u));
        }
    } else {
        unsigned m[NW];                                  // the same bytes as big-endian words: bit q of the row's string is bit 31 - (q & 31)
#pragma unroll
        for (int i = 0; i < NW; ++i) m[i] = __builtin_bswap32(w[i]);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int q = j * BITS, sh = q & 31;
            unsigned v = m[q >> 5] << sh;
            if (sh + BITS > 32) v |= m[(q >> 5) + 1] >> (32 - sh);
            s[j] = v >> (32 - BITS);
        }
    }
}

// the window of NS samples (each < 2^BITS); every bit no sample owns is zero
template <int BITS, int ORDER, int NS, int NW>
__device__ __forceinline__ void pack_window(const unsigned (&s)[NS], unsigned (&w)[NW]) {
    constexpr int LOW = BITS - 8;
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = 0u;
    if constexpr (ORDER == 0) {
        constexpr int G = BITS == 12 ? 2 : 4, GB = G * BITS / 8;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int base = (j / G) * GB, k = j % G;
            const int q = 8 * (base + G) + k * LOW;
            const unsigned lo = s[j] & ((1u << LOW) - 1u);
            w[(base + k) >> 2] |= (s[j] >> LOW) << (8 * ((base + k) & 3));
            w[q >> 5] |= lo << (q & 31);
            if ((q & 31) + LOW > 32) w[(q >> 5) + 1] |= lo >> (32 - (q & 31));
        }
    } else {
        unsigned m[NW];
#pragma unroll
        for (int i = 0; i < NW; ++i) m[i] = 0u;
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const int q = j * BITS, sh = q & 31;
            if (sh + BITS <= 32) {
                m[q >> 5] |= s[j] << (32 - sh - BITS);
            } else {
                m[q >> 5] |= s[j] >> (sh + BITS - 32);
                m[(q >> 5) + 1] |= s[j] << (64 - sh - BITS);
            }
        }
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = __builtin_bswap32(m[i]);
    }
}

template <int BITS, bool FAST>
struct BitsWindow {
    static constexpr int NC = FAST ? 8 : 2;              // cells per thread
    static constexpr int NS = 2 * NC;                    // samples of one sensor row
    static constexpr int NB = NS * BITS / 8;             // their bytes
    static constexpr int NW = (NB + 3) / 4;              // the window's dwords
};

template <int BITS, int ORDER, bool FAST>
__global__ void __launch_bounds__(256) ingest_bits_kernel(const uint8_t* __restrict__ frames, float* __restrict__ packed,
                                                          float* __restrict__ gray, int n, int hh, int ww, int64_t row_bytes, float maxv) {
    typedef BitsWindow<BITS, FAST> Wn;
    constexpr int NC = Wn::NC, NS = Wn::NS, NB = Wn::NB, NW = Wn::NW;
    const int64_t hw = (int64_t)hh * ww;
    const int wq = (ww + NC - 1) / NC;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * hh * wq) return;
    const int xq = (int)(t % wq);
    const int64_t row = t / wq;                          // img * hh + y
    const int y = (int)(row % hh);
    const int64_t img = row / hh;
    const int64_t at = (int64_t)xq * NB;                 // the window's first byte in its row
    const uint8_t* r0 = frames + (img * 2 * hh + 2 * (int64_t)y) * row_bytes + at;
    const int left = (int)(row_bytes - at < NB ? row_bytes - at : NB);      // the window's bytes that lie in the row
    unsigned s[2][NS];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint8_t* p = r0 + r * row_bytes;
        unsigned w[NW];
        if constexpr (FAST) {
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = reinterpret_cast<const unsigned*>(p)[i];
        } else {
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = 0u;
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (i < left) w[i >> 2] |= (unsigned)p[i] << (8 * (i & 3));
        }
        unpack_window<BITS, ORDER>(w, s[r]);
    }
    float c[NC][4];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        c[i][0] = (float)s[0][2 * i]; c[i][1] = (float)s[0][2 * i + 1];
        c[i][2] = (float)s[1][2 * i]; c[i][3] = (float)s[1][2 * i + 1];
    }
    const int x = NC * xq;
    const int64_t o = (int64_t)y * ww + x;
    if constexpr (FAST) {
        if (packed) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int j = 0; j < NC / 4; ++j) {
                    f32x4 v;
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = norm_dn(c[4 * j + i][k], maxv);
                    *reinterpret_cast<f32x4*>(packed + (img * 4 + k) * hw + o + 4 * j) = v;
                }
        }
        if (gray) {
#pragma unroll
            for (int j = 0; j < NC / 4; ++j) {
                f32x4 g;
#pragma unroll
                for (int i = 0; i < 4; ++i) g[i] = gray_dn(c[4 * j + i]);
                *reinterpret_cast<f32x4*>(gray + img * hw + o + 4 * j) = g;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            if (x + i >= ww) break;                      // an odd ww: the row ends inside this window
            if (packed) {
#pragma unroll
                for (int k = 0; k < 4; ++k) packed[(img * 4 + k) * hw + o + i] = norm_dn(c[i][k], maxv);
            }
            if (gray) gray[img * hw + o + i] = gray_dn(c[i]);
        }
    }
}

template <int BITS, int ORDER, bool FAST>
__global__ void __launch_bounds__(256) egress_bits_kernel(const float* __restrict__ rgb, uint8_t* __restrict__ out, int n, int H, int W,
                                                          int64_t row_bytes, int cols, float top) {
    typedef BitsWindow<BITS, FAST> Wn;
    constexpr int NC = Wn::NC, NS = Wn::NS, NB = Wn::NB, NW = Wn::NW;
    const int64_t HW = (int64_t)H * W;
    const int hh = H >> 1, ww = W >> 1, wq = (ww + NC - 1) / NC;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * hh * wq) return;
    const int xq = (int)(t % wq);
    const int x = NC * xq;
    const int64_t row = t / wq;                          // img * hh + y
    const int y = (int)(row % hh);
    const int64_t img = row / hh;
    unsigned s[2][NS];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* p = rgb + (img * 3 + ((cols >> (2 * k)) & 3)) * HW + (2 * (int64_t)y + (k >> 1)) * W + 2 * x + (k & 1);
        if constexpr (FAST) {
            const float* a = p - (k & 1);                // the 16-B aligned run of sixteen pixels; position k takes its even / odd ones
#pragma unroll
            for (int j = 0; j < NC / 2; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(a + 4 * j);
                s[k >> 1][4 * j + (k & 1)] = out_of<unsigned short>(dn_of(v[k & 1], top), top);
                s[k >> 1][4 * j + 2 + (k & 1)] = out_of<unsigned short>(dn_of(v[2 + (k & 1)], top), top);
            }
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i) s[k >> 1][2 * i + (k & 1)] = x + i < ww ? out_of<unsigned short>(dn_of(p[2 * i], top), top) : 0u;
        }
    }
    const int64_t at = (int64_t)xq * NB;
    uint8_t* r0 = out + (img * H + 2 * (int64_t)y) * row_bytes + at;
    const int left = (int)(row_bytes - at < NB ? row_bytes - at : NB);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint8_t* p = r0 + r * row_bytes;
        unsigned w[NW];
        pack_window<BITS, ORDER>(s[r], w);
        if constexpr (FAST) {
#pragma unroll
            for (int i = 0; i < NW; ++i) reinterpret_cast<unsigned*>(p)[i] = w[i];
        } else {
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (i < left) p[i] = (uint8_t)window_byte(w, i);
        }
    }
}

// one launch of kernel K<BITS, ORDER, FAST> chosen by the run-time (bit_depth, order, fast); bit_depth is 10, 12 or 14
#define BITS_DISPATCH(K, bits, order, fast, ...)                                                      \
    do {                                                                                              \
        if (bits == 10) BITS_DISPATCH_O(K, 10, order, fast, __VA_ARGS__);                             \
        else if (bits == 12) BITS_DISPATCH_O(K, 12, order, fast, __VA_ARGS__);                        \
        else BITS_DISPATCH_O(K, 14, order, fast, __VA_ARGS__);                                        \
    } while (0)
#define BITS_DISPATCH_O(K, B, order, fast, ...)                                                       \
    do {                                                                                              \
        if (order == 0) BITS_DISPATCH_F(K, B, 0, fast, __VA_ARGS__);                                  \
        else BITS_DISPATCH_F(K, B, 1, fast, __VA_ARGS__);                                             \
    } while (0)
#define BITS_DISPATCH_F(K, B, O, fast, ...)                                                           \
    do {                                                                                              \
        if (fast) hipLaunchKernelGGL((K<B, O, true>), dim3((unsigned)blocks), dim3(256), 0, s, __VA_ARGS__);  \
        else hipLaunchKernelGGL((K<B, O, false>), dim3((unsigned)blocks), dim3(256), 0, s, __VA_ARGS__);      \
    } while (0)

// ---- rvdd_video_push: the flow batch's operands and results, and the substituted frames of the ring ------------------------
// One byte per entry, handed to the kernel by value (B <= 64 slots, two directions)
struct SlotList {
    unsigned char slot[64];
};
struct PairList {
    unsigned char e[128];
};

// (V = f32x4 where a plane is a whole number of 16-B vectors, float otherwise; hw4 / hw2_4 count V's)
// I0[q] / I1[q], q < npairs: pair q is (centre, previous) of slot b for the entry b, (centre, next) for the entry 64 | b; with
// `all` -- every slot has every pair, no list -- pair q is slot q % B, direction q / B.
// gray_c / gray_p / gray_n: the [B][hw] planes of the ring positions that hold the centre, previous and next frames.
// dgray [B][hw]: the gray planes of the slots' previous OUTPUTS; slot b's pair towards the previous frame is matched against
// it where bit b of from_den is set (option "stream_flow_from_denoised"), against gray_p elsewhere.
template <typename V>
__global__ void __launch_bounds__(256) stream_gather_kernel(const float* __restrict__ gray_c, const float* __restrict__ gray_p,
                                                            const float* __restrict__ gray_n, const float* __restrict__ dgray,
                                                            float* __restrict__ I0, float* __restrict__ I1, PairList pl, int B, int all,
                                                            uint64_t from_den, int64_t hw4) {
    const int q = blockIdx.y;
    const int b = all ? q % B : pl.e[q] & 63;
    const int dir = all ? q / B : pl.e[q] >> 6;
    const V* c = reinterpret_cast<const V*>(gray_c) + (int64_t)b * hw4;
    const float* other = dir ? gray_n : ((from_den >> b) & 1) ? dgray : gray_p;
    const V* o = reinterpret_cast<const V*>(other) + (int64_t)b * hw4;
    V* d0 = reinterpret_cast<V*>(I0) + (int64_t)q * hw4;
    V* d1 = reinterpret_cast<V*>(I1) + (int64_t)q * hw4;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw4; i += (int64_t)gridDim.x * blockDim.x) {
        d0[i] = c[i];
        d1[i] = o[i];
    }
}

// flows [ndir][B][2][hw] of a step from the batch's u [npairs][2][hw]: the flow of a (slot, direction) that has a pair, zero
// for the others.  rank.e[dir * B + b] = position of that pair in the batch, 255 = none.
template <typename V>
__global__ void __launch_bounds__(256) stream_scatter_kernel(const float* __restrict__ u, float* __restrict__ flows, PairList rank,
                                                             int64_t hw2_4) {
    const int r = rank.e[blockIdx.y];
    V* d = reinterpret_cast<V*>(flows) + (int64_t)blockIdx.y * hw2_4;
    const V* src = r == 255 ? nullptr : reinterpret_cast<const V*>(u) + (int64_t)r * hw2_4;
    const V zero = {};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw2_4; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = src ? src[i] : zero;
}

// option "stream_all_frames": the packed frame of every listed slot from one ring position to its neighbour -- ring_prev / ring_pos
// [B][4][hw] are the positions before this push's and this push's; bit b of to_pos set: previous -> this push's (a tail: the last
// frame stands in for the missing next one), clear: this push's -> previous (a FIRST: frame 0 stands in for the missing previous
// one).  A packed frame is hw vectors of 16 B on a 16-B boundary whatever hw is.
__global__ void __launch_bounds__(256) stream_dup_kernel(float* __restrict__ ring_prev, float* __restrict__ ring_pos, SlotList sl,
                                                         uint64_t to_pos, int64_t hw) {
    const int b = sl.slot[blockIdx.y];
    const bool fwd = (to_pos >> b) & 1;
    const f32x4* src = reinterpret_cast<const f32x4*>(fwd ? ring_prev : ring_pos) + (int64_t)b * hw;
    f32x4* dst = reinterpret_cast<f32x4*>(fwd ? ring_pos : ring_prev) + (int64_t)b * hw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x) dst[i] = src[i];
}

}  // namespace

hipError_t launch_ingest_raw(const void* frames, int dtype, int layout, int n, int hh, int ww, int bit_depth, float* packed, float* gray,
                             hipStream_t s) {
    if (n <= 0 || (!packed && !gray)) return hipSuccess;
    const float maxv = (float)((1u << bit_depth) - 1u);
    if (dtype == 0) {
        const unsigned short* f = static_cast<const unsigned short*>(frames);
        return layout == 0 ? launch_ingest_t<unsigned short, 0>(f, n, hh, ww, maxv, packed, gray, s)
                           : launch_ingest_t<unsigned short, 1>(f, n, hh, ww, maxv, packed, gray, s);
    }
    const float* f = static_cast<const float*>(frames);
    return layout == 0 ? launch_ingest_t<float, 0>(f, n, hh, ww, maxv, packed, gray, s) : launch_ingest_t<float, 1>(f, n, hh, ww, maxv, packed, gray, s);
}

hipError_t launch_gray_of_rgb(const float* rgb, int n, int hh, int ww, int bayer, int bit_depth, float* gray, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (bayer < 0 || bayer > 3) return hipErrorInvalidValue;
    const int cols = bayer_cols(bayer);
    const float top = (float)((1u << bit_depth) - 1u);
    const uintptr_t al = reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(gray);
    const bool vec = (ww & 3) == 0 && (al & 15) == 0;
    const int64_t work = vec ? (int64_t)n * hh * (ww >> 2) : (int64_t)n * hh * ww;
    const int64_t blocks = (work + 255) / 256;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (vec)
        hipLaunchKernelGGL(gray_of_rgb_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, rgb, gray, n, hh, ww, cols, top);
    else
        hipLaunchKernelGGL(gray_of_rgb_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, rgb, gray, n, hh, ww, cols, top);
    return hipGetLastError();
}

int64_t egress_blocks(const float* rgb, int n, int H, int W, int layout, int dtype, const void* out, bool* wide) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(out);
    const int64_t hw = (int64_t)H * W;
    int64_t per;                                         // threads per image
    if (layout == 0) {
        const int P = dtype == 0 ? 8 : 4;
        *wide = hw % P == 0 && (al & 15) == 0;
        per = *wide ? hw / P : hw;
    } else {
        *wide = ((W >> 1) & 3) == 0 && (al & 15) == 0;
        per = (int64_t)(H >> 1) * (*wide ? W >> 3 : W >> 1);
    }
    constexpr int64_t most = 0x7fffffffll * 256;         // threads of the largest grid
    if (per > most || n > most / per) return -1;
    return (n * per + 255) / 256;
}

hipError_t launch_egress(const float* rgb, int n, int H, int W, int layout, int dtype, int bit_depth, int bayer, void* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (layout < 0 || layout > 2 || dtype < 0 || dtype > 1 || H < 1 || W < 1) return hipErrorInvalidValue;
    if (layout != 0 && (bayer < 0 || bayer > 3 || ((H | W) & 1))) return hipErrorInvalidValue;
    bool wide;
    const int64_t blocks = egress_blocks(rgb, n, H, W, layout, dtype, out, &wide);
    if (blocks < 0) return hipErrorInvalidValue;
    const int cols = layout == 0 ? 0 : bayer_cols(bayer);
    const float top = (float)((1u << bit_depth) - 1u);
    return layout == 0   ? launch_egress_l<0>(rgb, n, H, W, cols, top, dtype, out, wide, blocks, s)
           : layout == 1 ? launch_egress_l<1>(rgb, n, H, W, cols, top, dtype, out, wide, blocks, s)
                         : launch_egress_l<2>(rgb, n, H, W, cols, top, dtype, out, wide, blocks, s);
}

int64_t bits_blocks(int n, int hh, int ww, bool fast) {
    const int64_t per = (int64_t)hh * (fast ? ww >> 3 : (ww + 1) >> 1);      // threads per image
    constexpr int64_t most = 0x7fffffffll * 256;
    if (per > most || (per > 0 && n > most / per)) return -1;
    return (n * per + 255) / 256;
}

bool ingest_bits_fast(const uint8_t* frames, int ww, const float* packed, const float* gray) {
    const uintptr_t al = reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(gray);
    return (ww & 7) == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (al & 15) == 0;
}

bool egress_bits_fast(const float* rgb, int W, const uint8_t* out) {
    return (W & 15) == 0 && (reinterpret_cast<uintptr_t>(rgb) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
}

hipError_t launch_ingest_bits(const uint8_t* frames, int order, int n, int hh, int ww, int bit_depth, float* packed, float* gray, hipStream_t s) {
    if (n <= 0 || (!packed && !gray)) return hipSuccess;
    if (order < 0 || order > 1 || (bit_depth != 10 && bit_depth != 12 && bit_depth != 14) || hh < 1 || ww < 1) return hipErrorInvalidValue;
    if (order == 0 && bit_depth != 12 && (ww & 1)) return hipErrorInvalidValue;
    const bool fast = ingest_bits_fast(frames, ww, packed, gray);
    const int64_t blocks = bits_blocks(n, hh, ww, fast);
    if (blocks < 0) return hipErrorInvalidValue;
    const int64_t row_bytes = bits_row_bytes(ww, bit_depth);
    const float maxv = (float)((1u << bit_depth) - 1u);
    BITS_DISPATCH(ingest_bits_kernel, bit_depth, order, fast, frames, packed, gray, n, hh, ww, row_bytes, maxv);
    return hipGetLastError();
}

hipError_t launch_egress_bits(const float* rgb, int n, int H, int W, int order, int bit_depth, int bayer, uint8_t* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (order < 0 || order > 1 || (bit_depth != 10 && bit_depth != 12 && bit_depth != 14) || H < 2 || W < 2 || ((H | W) & 1) || bayer < 0 || bayer > 3)
        return hipErrorInvalidValue;
    if (order == 0 && bit_depth != 12 && (W & 3)) return hipErrorInvalidValue;
    const bool fast = egress_bits_fast(rgb, W, out);
    const int64_t blocks = bits_blocks(n, H >> 1, W >> 1, fast);
    if (blocks < 0) return hipErrorInvalidValue;
    const int64_t row_bytes = bits_row_bytes(W >> 1, bit_depth);
    const int cols = bayer_cols(bayer);
    const float top = (float)((1u << bit_depth) - 1u);
    BITS_DISPATCH(egress_bits_kernel, bit_depth, order, fast, rgb, out, n, H, W, row_bytes, cols, top);
    return hipGetLastError();
}

// planes of the handle's own buffers (hipMalloc alignment); pairs: slot | direction << 6 of every pair in batch order (ignored
// when every slot has every pair)
hipError_t launch_stream_gather(const float* gray_c, const float* gray_p, const float* gray_n, const float* dgray, uint64_t from_den,
                                float* I0, float* I1, const uint8_t* pairs, int npairs, int B, int64_t hw, hipStream_t s) {
    PairList pl{};
    const int all = npairs == B * (gray_n ? 2 : 1);
    if (B > 64 || npairs < 1 || npairs > B * (gray_n ? 2 : 1) || (from_den && !dgray)) return hipErrorInvalidValue;      // one bit per slot
    if (!all)
        for (int q = 0; q < npairs; ++q) {
            if ((pairs[q] & 63) >= B || (pairs[q] >> 6) > (gray_n ? 1 : 0)) return hipErrorInvalidValue;
            pl.e[q] = pairs[q];
        }
    const bool vec = (hw & 3) == 0;
    const int64_t hw4 = vec ? hw / 4 : hw;
    const int gx = (int)((hw4 + 255) / 256 < 256 ? (hw4 + 255) / 256 : 256);
    if (vec)
        hipLaunchKernelGGL(stream_gather_kernel<f32x4>, dim3(gx, npairs), dim3(256), 0, s, gray_c, gray_p, gray_n, dgray, I0, I1, pl, B, all,
                           from_den, hw4);
    else
        hipLaunchKernelGGL(stream_gather_kernel<float>, dim3(gx, npairs), dim3(256), 0, s, gray_c, gray_p, gray_n, dgray, I0, I1, pl, B, all,
                           from_den, hw4);
    return hipGetLastError();
}

hipError_t launch_stream_scatter(const float* u, float* flows, const uint8_t* pairs, int npairs, int ndir, int B, int64_t hw, hipStream_t s) {
    if (B > 64 || ndir < 1 || ndir > 2 || npairs < 0 || npairs > ndir * B) return hipErrorInvalidValue;
    PairList rank;
    for (int i = 0; i < 128; ++i) rank.e[i] = 255;
    for (int q = 0; q < npairs; ++q) {
        if ((pairs[q] & 63) >= B || (pairs[q] >> 6) >= ndir) return hipErrorInvalidValue;
        rank.e[(pairs[q] >> 6) * B + (pairs[q] & 63)] = (unsigned char)q;
    }
    const bool vec = (hw & 1) == 0;
    const int64_t n4 = vec ? 2 * hw / 4 : 2 * hw;
    const int gx = (int)((n4 + 255) / 256 < 256 ? (n4 + 255) / 256 : 256);
    if (vec)
        hipLaunchKernelGGL(stream_scatter_kernel<f32x4>, dim3(gx, ndir * B), dim3(256), 0, s, u, flows, rank, n4);
    else
        hipLaunchKernelGGL(stream_scatter_kernel<float>, dim3(gx, ndir * B), dim3(256), 0, s, u, flows, rank, n4);
    return hipGetLastError();
}

hipError_t launch_stream_dup(float* ring_prev, float* ring_pos, const int* slots, int nslots, uint64_t to_pos, int B, int64_t hw, hipStream_t s) {
    if (nslots <= 0) return hipSuccess;
    if (B > 64 || nslots > B) return hipErrorInvalidValue;
    SlotList sl{};
    for (int q = 0; q < nslots; ++q) {
        if (slots[q] < 0 || slots[q] >= B) return hipErrorInvalidValue;
        sl.slot[q] = (unsigned char)slots[q];
    }
    const int gx = (int)((hw + 255) / 256 < 256 ? (hw + 255) / 256 : 256);
    hipLaunchKernelGGL(stream_dup_kernel, dim3(gx, nslots), dim3(256), 0, s, ring_prev, ring_pos, sl, to_pos, hw);
    return hipGetLastError();
}
