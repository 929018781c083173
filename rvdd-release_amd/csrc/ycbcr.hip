// Display images as frames of a Y'CbCr 4:2:0 video (rvdd_ycbcr; include/rvdd.h states the rule): BT.709, limited range, chroma the
// box average of each 2 x 2 quad, 8 or 10 bits, one Y4M frame body per image -- Y [H][W], Cb and Cr [H/2][W/2].
//
// Compiled with -ffp-contract=off like its neighbours; the one floating-point operation per value is the product in `quant`, and
// everything behind it is integer: the NumPy restatement (tests/ycbcr_ref.py) gives the same bits.
//
// A memory stream: 12 B read and 1.5 (8 bits) or 3 (10 bits) B written per pixel.  The byte-wide Y samples are what can go wrong: a
// thread that stored its own pixel's sample would issue one byte per lane.  The wide form gives a thread a strip of two rows by
// kStrip = 8 pixels: six 16-B loads of the HWC floats per row (a lane's 96 B are contiguous, and the lanes of a wave cover 6 KiB of
// a row without a gap), ONE store of 8 B (8 bits) or 16 B (10 bits) of Y per row -- consecutive lanes write consecutive words: a wave
// stores 512 B / 1 KiB of a row at once -- and the strip's four Cb and four Cr samples as one dword (8 bits) or two (10 bits) each.
// A strip of 4 would halve those stores to one dword of Y and two bytes of chroma, below the dword the form is for; 16 would hold
// 96 floats per lane for nothing a wave's 512 B does not already have.  It needs W % 8 == 0 and both pointers 16-B aligned: H W
// is then a multiple of 16 samples and an image's 3 H W / 2 samples a multiple of 24, so at 8 bits an image starts on 8 B, its Cb and
// Cr planes on 4 B, at 10 bits on 16 B and 8 B -- every store (8 / 4 B, 16 / 8 B) is aligned to its own size, not to more.  The
// narrow form, for every other even shape: one quad per thread, scalar loads and stores.  Both compute every sample with the same
// integer expressions: same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rvdd_internal.h"

namespace {

constexpr int kStrip = 8;                         // pixels of a row a thread of the wide form owns
constexpr int kThreads = 256;
constexpr uint32_t kHalfK = 65535u * 8192u;       // K / 2, K = 65535 * 16384

// one display value -> 0 .. 65535: the clamp sends NaN and everything <= 0 to 0, +inf to 255; then one product, rounded half to even
__device__ __forceinline__ int quant(float d) {
    d = d > 0.0f ? d : 0.0f;
    d = d < 255.0f ? d : 255.0f;
    return (int)rintf(d * 257.0f);
}

// Y = 16 m + floor((L * 219 m + K / 2) / K).  K = 65535 * 2^14, and floor(floor(a / 2^14) / 65535) = floor(a / K) for a >= 0: the 64-bit
// numerator (up to 9.4e11) shifted is below 2^26, and the division by the constant is a 32-bit multiply-high.
template <int D>
__device__ __forceinline__ unsigned luma(int r, int g, int b) {
    constexpr unsigned m = 1u << (D - 8);
    const unsigned L = 3483u * (unsigned)r + 11718u * (unsigned)g + 1183u * (unsigned)b;      // <= K < 2^30
    const unsigned t = (unsigned)(((uint64_t)L * (219u * m) + kHalfK) >> 14);
    return 16u * m + t / 65535u;
}

// 128 m + floor((c * 224 m + 2 K) / (4 K)) for the signed c of a quad's sums (|c| <= 8192 * 4 * 65535 < 2^31): 512 * 4 K added to the
// numerator makes it positive (the quotient is at least -448), the floor of a positive number is the shift and the unsigned division --
// 4 K = 65535 * 2^16 -- and 512 comes off the quotient.
template <int D>
__device__ __forceinline__ unsigned chroma(int64_t c) {
    constexpr int m = 1 << (D - 8);
    constexpr int64_t K = 65535ll * 16384ll;
    const uint64_t num = (uint64_t)(c * (224 * m) + 2 * K + 512 * 4 * K);
    const unsigned t = (unsigned)(num >> 16);                                                   // < 2^26
    return (unsigned)(128 * m - 512 + (int)(t / 65535u));
}
template <int D>
__device__ __forceinline__ void chroma_pair(const int (&s)[3], unsigned& cb, unsigned& cr) {
    cb = chroma<D>(-1877ll * s[0] - 6315ll * s[1] + 8192ll * s[2]);
    cr = chroma<D>(8192ll * s[0] - 7441ll * s[1] - 751ll * s[2]);
}

// N samples (N * sizeof(T) = 4, 8 or 16 bytes) as ONE store of that size, the first sample in the lowest bits; dst aligned to it
template <typename T, int N>
__device__ __forceinline__ void store_samples(T* __restrict__ dst, const unsigned (&v)[N]) {
    constexpr int PER = 4 / (int)sizeof(T), WORDS = N / PER;      // samples per dword, dwords
    static_assert(N % PER == 0 && (WORDS == 1 || WORDS == 2 || WORDS == 4), "whole dwords, one store");
    unsigned x[WORDS];
#pragma unroll
    for (int j = 0; j < WORDS; ++j) {
        x[j] = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) x[j] |= v[j * PER + i] << (8 * (int)sizeof(T) * i);
    }
    if constexpr (WORDS == 1) {
        *reinterpret_cast<unsigned*>(dst) = x[0];
    } else {
        typedef unsigned words_t __attribute__((ext_vector_type(WORDS)));
        words_t w;
#pragma unroll
        for (int j = 0; j < WORDS; ++j) w[j] = x[j];
        *reinterpret_cast<words_t*>(dst) = w;
    }
}

// T = uint8_t (D = 8) or uint16_t (D = 10).  total = n * (H / 2) * (W / P) threads' worth of strips, P = kStrip (WIDE) or 2.
template <int D, bool WIDE>
__global__ void __launch_bounds__(kThreads) ycbcr_kernel(const float* __restrict__ disp, void* __restrict__ frames, int64_t total, int H, int W) {
    typedef typename std::conditional<D == 8, uint8_t, uint16_t>::type T;
    constexpr int P = WIDE ? kStrip : 2;
    const int hh = H >> 1, wq = W / P;
    const int64_t HW = (int64_t)H * W;
    T* const out = static_cast<T*>(frames);
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        const int x = P * (int)(i % wq);
        const int64_t row = i / wq;                      // img * hh + y
        const int y = (int)(row % hh);
        const int64_t img = row / hh;
        const float* src = disp + ((img * H + 2 * (int64_t)y) * W + x) * 3;
        T* const fr = out + img * (HW + (HW >> 1));
        int s[P / 2][3] = {};                            // the quads' sums
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            float v[3 * P];
            const float* p = src + (int64_t)r * W * 3;
            if constexpr (WIDE) {
#pragma unroll
                for (int j = 0; j < 3 * P / 4; ++j) {
                    const f32x4 q = reinterpret_cast<const f32x4*>(p)[j];
                    v[4 * j] = q[0]; v[4 * j + 1] = q[1]; v[4 * j + 2] = q[2]; v[4 * j + 3] = q[3];
                }
            } else {
#pragma unroll
                for (int j = 0; j < 3 * P; ++j) v[j] = p[j];
            }
            unsigned yy[P];
#pragma unroll
            for (int k = 0; k < P; ++k) {
                const int qr = quant(v[3 * k]), qg = quant(v[3 * k + 1]), qb = quant(v[3 * k + 2]);
                yy[k] = luma<D>(qr, qg, qb);
                s[k >> 1][0] += qr; s[k >> 1][1] += qg; s[k >> 1][2] += qb;
            }
            T* dst = fr + (2 * (int64_t)y + r) * W + x;
            if constexpr (WIDE) {
                store_samples<T, P>(dst, yy);
            } else {
                dst[0] = (T)yy[0]; dst[1] = (T)yy[1];
            }
        }
        unsigned cb[P / 2], cr[P / 2];
#pragma unroll
        for (int k = 0; k < P / 2; ++k) chroma_pair<D>(s[k], cb[k], cr[k]);
        T* const pb = fr + HW + (int64_t)y * (W >> 1) + (x >> 1);
        T* const pr = pb + (HW >> 2);
        if constexpr (WIDE) {
            store_samples<T, P / 2>(pb, cb);
            store_samples<T, P / 2>(pr, cr);
        } else {
            pb[0] = (T)cb[0];
            pr[0] = (T)cr[0];
        }
    }
}

template <int D>
hipError_t launch_d(const float* disp, void* frames, int64_t total, int H, int W, bool wide, int64_t blocks, hipStream_t s) {
    if (wide)
        hipLaunchKernelGGL((ycbcr_kernel<D, true>), dim3((unsigned)blocks), dim3(kThreads), 0, s, disp, frames, total, H, W);
    else
        hipLaunchKernelGGL((ycbcr_kernel<D, false>), dim3((unsigned)blocks), dim3(kThreads), 0, s, disp, frames, total, H, W);
    return hipGetLastError();
}

// threads of a launch over n images of H x W (even, >= 2); -1 = they leave 63 bits
int64_t ycbcr_threads(int n, int H, int W, bool wide) {
    const int64_t per = (int64_t)(H >> 1) * (W / (wide ? kStrip : 2));      // < 2^60
    if (n > 0 && per > INT64_MAX / n) return -1;
    return n * per;
}

}  // namespace

bool ycbcr_wide(const float* disp, int W, const void* frames) {
    return W % kStrip == 0 && ((reinterpret_cast<uintptr_t>(disp) | reinterpret_cast<uintptr_t>(frames)) & 15) == 0;
}

int64_t ycbcr_blocks(int n, int H, int W, bool wide) {
    const int64_t total = ycbcr_threads(n, H, W, wide);
    if (total < 0 || total > 0x7fffffffll * kThreads) return -1;
    return (total + kThreads - 1) / kThreads;
}

hipError_t launch_ycbcr(const float* disp, int n, int H, int W, int depth, void* frames, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (H < 2 || W < 2 || ((H | W) & 1) || (depth != 8 && depth != 10)) return hipErrorInvalidValue;
    const bool wide = ycbcr_wide(disp, W, frames);
    const int64_t blocks = ycbcr_blocks(n, H, W, wide);
    if (blocks < 0) return hipErrorInvalidValue;
    const int64_t total = ycbcr_threads(n, H, W, wide);
    return depth == 8 ? launch_d<8>(disp, frames, total, H, W, wide, blocks, s) : launch_d<10>(disp, frames, total, H, W, wide, blocks, s);
}
