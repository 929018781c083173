// The recurrent state of single sequences of a batch (previous output, features, amax words): zeroed by the latch of a
// partial reset (rvdd_reset_slots), moved between slots (rvdd_move_slots).  Pure store and copy bandwidth; compiled with
// -ffp-contract=off like the file these kernels came from (they hold no floating-point arithmetic).
#include "rvdd_internal.h"

namespace {

// The latch of a partial reset (rvdd_reset_slots): the recurrent features and every set of amax words of the sequences in
// `mask` are zeroed, as the memsets of a first step zero them for the whole batch.  Grid (blocks, popcount(mask)): block row y
// serves the y-th set bit, so one launch covers any set of slots without a mask on the device.  Pure store bandwidth (177 MB of
// features per 720p sequence): 16-B stores, grid-stride.  `feat` (nullable): [B][feat4] float4; `words` (nullable):
// [nsets][B][kAmaxSeqWords].
__global__ __launch_bounds__(256) void latch_zero_kernel(unsigned long long mask, f32x4* __restrict__ feat, int64_t feat4,
                                                         unsigned* __restrict__ words, int nsets, int B) {
    unsigned long long m = mask;
    for (unsigned k = 0; k < blockIdx.y; ++k) m &= m - 1;
    const int b = __builtin_ctzll(m);
    const int64_t me = (int64_t)blockIdx.x * 256 + threadIdx.x, all = (int64_t)gridDim.x * 256;
    if (feat) {
        f32x4* p = feat + (size_t)b * feat4;
        for (int64_t i = me; i < feat4; i += all) p[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (words) {
        constexpr int kQ = kAmaxSeqWords / 4;
        for (int64_t i = me; i < (int64_t)nsets * kQ; i += all) {
            const int set = (int)(i / kQ), j = (int)(i - (int64_t)set * kQ);
            reinterpret_cast<uint4*>(words + ((size_t)set * B + b) * kAmaxSeqWords)[j] = uint4{0u, 0u, 0u, 0u};
        }
    }
}

// rvdd_move_slots: the whole recurrent state of sequence from[k] replaces that of sequence to[k].  Grid (blocks, count): block
// row y serves pair y, whose two slots are bytes of the kernel arguments (eight pairs per 64-bit word) -- nothing is staged on
// the device and the launch is ordered in its stream like any other.  Pure copy bandwidth (208 B per pixel read and written:
// 16 of the previous output, 192 of the features): 16-B loads and stores, grid-stride.  The pairs are disjoint (checked by
// the caller), so no block reads what another one writes.  `feat` and `words` nullable as in latch_zero_kernel.
struct MovePairs {
    unsigned long long from[kMaxMovePairs / 8], to[kMaxMovePairs / 8];
};
__device__ __forceinline__ int move_pair_slot(unsigned long long w0, unsigned long long w1, unsigned long long w2, unsigned long long w3,
                                              unsigned k) {
    const unsigned long long w = k < 8 ? w0 : (k < 16 ? w1 : (k < 24 ? w2 : w3));
    return (int)((w >> (8 * (k & 7u))) & 0xffull);
}
__global__ __launch_bounds__(256) void move_slots_kernel(MovePairs pr, f32x4* __restrict__ den, int64_t den4, f32x4* __restrict__ feat,
                                                         int64_t feat4, unsigned* __restrict__ words, int nsets, int B) {
    const int src = move_pair_slot(pr.from[0], pr.from[1], pr.from[2], pr.from[3], blockIdx.y);
    const int dst = move_pair_slot(pr.to[0], pr.to[1], pr.to[2], pr.to[3], blockIdx.y);
    const int64_t me = (int64_t)blockIdx.x * 256 + threadIdx.x, all = (int64_t)gridDim.x * 256;
    if (feat) {
        const f32x4* __restrict__ p = feat + (size_t)src * feat4;
        f32x4* __restrict__ q = feat + (size_t)dst * feat4;
#pragma unroll 4
        for (int64_t i = me; i < feat4; i += all) q[i] = p[i];
    }
    {
        const f32x4* __restrict__ p = den + (size_t)src * den4;
        f32x4* __restrict__ q = den + (size_t)dst * den4;
        for (int64_t i = me; i < den4; i += all) q[i] = p[i];
    }
    if (words) {
        constexpr int kQ = kAmaxSeqWords / 4;
        for (int64_t i = me; i < (int64_t)nsets * kQ; i += all) {
            const int set = (int)(i / kQ), j = (int)(i - (int64_t)set * kQ);
            reinterpret_cast<uint4*>(words + ((size_t)set * B + dst) * kAmaxSeqWords)[j] =
                reinterpret_cast<const uint4*>(words + ((size_t)set * B + src) * kAmaxSeqWords)[j];
        }
    }
}

}  // namespace

hipError_t launch_latch_zero(unsigned long long mask, float* feat, int64_t feat_per_seq, unsigned* words, int nsets, int B, hipStream_t s) {
    const int nseq = __builtin_popcountll(mask);
    if (!nseq || (!feat && !words)) return hipSuccess;
    if (B > 64 || (B < 64 && (mask >> B)) || (feat_per_seq & 3)) return hipErrorInvalidValue;
    const int64_t feat4 = feat ? feat_per_seq / 4 : 0, words4 = words ? (int64_t)nsets * (kAmaxSeqWords / 4) : 0;
    const int64_t work = feat4 > words4 ? feat4 : words4;
    int64_t nblk = (work + 256 * 4 - 1) / (256 * 4);        // four 16-B stores per thread, at most 1024 blocks per sequence
    nblk = nblk < 1 ? 1 : (nblk > 1024 ? 1024 : nblk);
    hipLaunchKernelGGL(latch_zero_kernel, dim3((unsigned)nblk, nseq), dim3(256), 0, s, mask, reinterpret_cast<f32x4*>(feat), feat4,
                       words, nsets, B);
    return hipGetLastError();
}

hipError_t launch_move_slots(const int* from, const int* to, int count, float* den, int64_t den_per_seq, float* feat, int64_t feat_per_seq,
                             unsigned* words, int nsets, int B, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (count > kMaxMovePairs || B > 64 || !den || (den_per_seq & 3) || (feat_per_seq & 3)) return hipErrorInvalidValue;
    MovePairs pr{};
    for (int k = 0; k < count; ++k) {
        if (from[k] < 0 || from[k] >= B || to[k] < 0 || to[k] >= B) return hipErrorInvalidValue;
        pr.from[k / 8] |= (unsigned long long)from[k] << (8 * (k % 8));
        pr.to[k / 8] |= (unsigned long long)to[k] << (8 * (k % 8));
    }
    const int64_t den4 = den_per_seq / 4, feat4 = feat ? feat_per_seq / 4 : 0;
    const int64_t work = feat4 > den4 ? feat4 : den4;
    int64_t nblk = (work + 256 * 4 - 1) / (256 * 4);        // four 16-B copies per thread, at most 1024 blocks per pair
    nblk = nblk < 1 ? 1 : (nblk > 1024 ? 1024 : nblk);
    hipLaunchKernelGGL(move_slots_kernel, dim3((unsigned)nblk, count), dim3(256), 0, s, pr, reinterpret_cast<f32x4*>(den), den4,
                       reinterpret_cast<f32x4*>(feat), feat4, words, nsets, B);
    return hipGetLastError();
}
