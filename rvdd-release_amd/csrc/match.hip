// Footage matched to the checkpoint's noise curve (rvdd_match_raw, rvdd_unmatch_rgb; the stage rvdd_set_match puts around the step of
// rvdd_video_push).  An affine noise curve var(m) = a m - b maps onto any other by an affine map of the samples: on samples in
// [-1,1] that is v' = scale * v + offset on the way in and v = (v' - offset) * (1 / scale) on the way out (include/rvdd.h has the
// derivation, rvdd_match_coeffs the numbers).  Compiled -ffp-contract=off like dpc.hip: the product and the sum are each rounded to
// f32 on their own, so that the written values are the bits of the NumPy restatement (tests/match_ref.py).
//
// Both directions are plain streams over a dense tensor: a thread owns one sample, or in the wide form (both pointers 16-byte
// aligned, the element count a multiple of 4) four neighbouring ones as one 16-byte load and one 16-byte store.  The arithmetic per
// sample is the same: same bits.  A thread reads its samples before it writes them and touches no others, so in place is fine; the
// pointers are not declared restrict for that reason.
#include "rvdd_internal.h"

namespace {

// UN = false: (p * v) + q with p = scale, q = offset;  UN = true: (v - q) * p with p = (float)(1 / scale), q = offset
template <bool UN>
__device__ __forceinline__ float match_one(float v, float p, float q) {
    if constexpr (UN) return (v - q) * p;
    return (p * v) + q;
}

template <bool UN, int NC>
__global__ void __launch_bounds__(256) match_kernel(const float* in, float* out, int64_t items, float p, float q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    if constexpr (NC == 4) {
        f32x4 v = reinterpret_cast<const f32x4*>(in)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = match_one<UN>(v[k], p, q);
        reinterpret_cast<f32x4*>(out)[i] = v;
    } else {
        out[i] = match_one<UN>(in[i], p, q);
    }
}

}  // namespace

bool match_wide(const float* in, const float* out, int64_t count) {
    return (count & 3) == 0 && ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
}

int64_t match_blocks(int64_t count, bool wide) {
    const int64_t blocks = ((wide ? count >> 2 : count) + 255) / 256;
    return blocks > 0x7fffffffll ? -1 : blocks;
}

hipError_t launch_match(const float* in, float* out, int64_t count, float scale, float offset, bool inverse, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (!in || !out) return hipErrorInvalidValue;
    const bool wide = match_wide(in, out, count);
    const int64_t blocks = match_blocks(count, wide);
    if (blocks < 0) return hipErrorInvalidValue;
    const int64_t items = wide ? count >> 2 : count;
    const float p = inverse ? (float)(1.0 / (double)scale) : scale;
    const dim3 grid((unsigned)blocks), block(256);
    if (inverse) {
        if (wide) hipLaunchKernelGGL((match_kernel<true, 4>), grid, block, 0, s, in, out, items, p, offset);
        else hipLaunchKernelGGL((match_kernel<true, 1>), grid, block, 0, s, in, out, items, p, offset);
    } else {
        if (wide) hipLaunchKernelGGL((match_kernel<false, 4>), grid, block, 0, s, in, out, items, p, offset);
        else hipLaunchKernelGGL((match_kernel<false, 1>), grid, block, 0, s, in, out, items, p, offset);
    }
    return hipGetLastError();
}
