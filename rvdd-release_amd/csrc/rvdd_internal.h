// Internal declarations shared by the HIP translation units of librvdd_hip.so.
// Activation maps live in HBM as NHWC fp32 with C = 48 (192 B per pixel, three
// 64-B lines); the network input is NHWC with C padded to 16; 3-channel
// frames that are gathered by the bicubic warp are NHWC with C padded to 4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kF = 48;        // feature channels everywhere (filters=48)
constexpr int kNetInC = 16;   // padded channel count of the network input map

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: `done` (one per kernel
// instantiation) remembers the devices of this process that already have it, one bit per device ordinal.
inline hipError_t allow_dynamic_lds(const void* kern, size_t bytes, std::atomic<uint64_t>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const uint64_t bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return e;
}
// compute units of the current device (queried once per device ordinal)
inline int current_device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    int v = cache[dev & 63].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    cache[dev & 63].store(cus, std::memory_order_relaxed);
    return cus;
}
inline unsigned nblocks(size_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }      // blocks of bs threads for n of them

// ---------------------------------------------------------------- conv3x3 --
// EPI_RELU_OUT3 (Winograd kernel only): ReLU, store the 48-channel map AND apply the final 1x1 conv 48->3
enum ConvEpi { EPI_NONE = 0, EPI_RELU = 1, EPI_POOL = 2, EPI_RELU_ADD2 = 3, EPI_RELU_OUT3 = 4 };

struct ConvArgs {
    const float* in;      // NHWC [B][H][W][CIN]
    const float* w;       // arranged [9][CIN/16][3][64 lanes][4] (see arrange_conv3x3 / arrange_wino3x3 in net_convunet.hip)
    const float* bias;    // [48]   (ignored when acc_in != nullptr)
    const float* acc_in;  // NHWC48 [B][H][W] partial sums to start from, or nullptr
    const float* res1;    // EPI_RELU_ADD2: out = relu(conv) + res1 + res2
    const float* res2;
    float* out;           // NHWC48 [B][Hout][Wout]
    int B, H, W;          // conv domain (input size = conv output size)
    int Hout, Wout;       // size of the map `out` points to
    int oy, ox;           // placement of the conv output inside it (zero_pad_features)
    int ups;              // Winograd kernel, 48 -> 48, ReLU only: `in` is [B][H/2][W/2][48] and the conv input is its
                          // bilinear x2 upsample (align_corners=False), interpolated in the patch load
    int tiles_x, tiles_y, ntiles;
    // EPI_RELU_OUT3: PostConvs[1] (networks/unet.py:713-720) fused into PostConvs[0]'s epilogue
    const float* w3;      // [3][48]
    const float* b3;      // [3]
    float* out3_nchw;     // [B][3][H][W]
    float* out3_nhwc4;    // [B][H][W][4] copy for the next frame's warp, or nullptr
    float wscale;         // conv3x3h.hip: 2^-s, the filters having been scaled by 2^s before the f16 split
    // conv3x3h.hip, block floating point per map and sequence (see amax_shift below): amax_in[b][kAmaxSeqWords] = words whose
    // maximum is the bits of max |x| over sequence b of the input map (null: no scaling), amax_out[b][kAmaxSeqWords] receives
    // the same for the map this launch writes (null: nobody reads that map as a split operand)
    const unsigned* amax_in;
    unsigned* amax_out;
};

// ---- block floating point for the split-f16 operands --------------------------------------------------------------------
// An f16 half saturates at 65504 and loses its low bits below 2^-14; an f32 activation has neither limit.  Every map that
// a split-f16 kernel reads therefore carries, per sequence, kAmaxLines words (one per 128-byte line) whose maximum is the
// bits of max |x| over the map, written by the kernel that produced the map (atomic max on the integer bits, which order
// like the non-negative floats they are).  The reader multiplies by the power of two that puts that maximum into
// [2^3, 2^4) before it splits -- the range the trained nets' activations have by themselves -- and scales the sums back in
// its epilogue; both exact.  A zero / non-finite / absurdly small maximum (< 2^-95) means "no scaling".
// Atomics are the cost to watch here (measured, profiles/r04_amax_atomics.txt): the waves of a persistent kernel finish
// together, and one atomic per wave on one word per sequence (2048 on 8 addresses) serialised for 13 us at the tail of every
// conv launch; one per wave of the streaming kernels (10^5 per launch) cost 4 % of a frame-step even spread over 64 words of
// two cache lines.  So: a workgroup reduces through LDS first (amax_commit_block), and the workgroups of a launch spread
// over kAmaxLines separate lines per sequence.
constexpr int kAmaxTargetExp = 3;
constexpr int kAmaxLines = 16;          // words per sequence, each at the start of its own 128-byte line
constexpr int kAmaxLineWords = 32;
constexpr int kAmaxSeqWords = kAmaxLines * kAmaxLineWords;
// The shift for a map whose max |x| has these bits.  A maximum inside [2^-6, 2^12) -- every map of the trained nets on frames
// in the reference's [-1, 1] -- needs none: the f16 halves are as far from overflow (x16 at least) and as precise relative to
// the map's maximum (2^-19 at worst) as they need to be, the reader then skips the multiplication (it is not free: the chunk
// loop of conv3x3h_kernel has no spare vector-issue slot, 18 v_pk_mul_f32 per tile cost 1.5 % of a layer) and in-domain
// frames keep the bits they had before the scaling existed.  Outside the window: the shift that puts the maximum into [8, 16).
__host__ __device__ inline int amax_shift(unsigned bits) {
    const int e = (int)((bits >> 23) & 0xffu);
    if (e < 32 || e == 255) return 0;                      // zero, absurdly small, inf / nan: leave alone
    if (e >= 127 - 6 && e < 127 + 12) return 0;
    return kAmaxTargetExp - (e - 127);
}
__host__ __device__ inline float pow2f(int k) {          // 2^k, |k| <= 126
    const unsigned u = (unsigned)(127 + k) << 23;
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
#ifdef __HIPCC__
// v (+ | max) the same variable of the lane whose index differs in bit 0 / 1 (a quad neighbour: DPP quad_perm) or in bit 4 / 5
// (v_permlane16_swap / v_permlane32_swap): what `v + __shfl_xor(v, MASK)` / `fmaxf(v, __shfl_xor(v, MASK))` give, bit for bit
// (addition and maximum commute) -- without the LDS round trip of the ds_bpermute_b32 hipcc lowers __shfl_xor to.  Every lane active.
template <int MASK>
__device__ __forceinline__ void lane_xor_pair(float v, float& a, float& b) {
    static_assert(MASK == 1 || MASK == 2 || MASK == 16 || MASK == 32, "quad neighbours and row pairs only");
    const int u = __builtin_bit_cast(int, v);
    if constexpr (MASK == 1) {
        a = v;
        b = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, u, 0xB1, 0xf, 0xf, true));      // quad_perm:[1,0,3,2]
    } else if constexpr (MASK == 2) {
        a = v;
        b = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, u, 0x4E, 0xf, 0xf, true));      // quad_perm:[2,3,0,1]
    } else if constexpr (MASK == 16) {
        // {own, partner} or {partner, own}.  (Elements into scalars first: __builtin_bit_cast of r[1] itself reads r[0].)
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);
        const unsigned r0 = r[0], r1 = r[1];
        a = __builtin_bit_cast(float, r0);
        b = __builtin_bit_cast(float, r1);
    } else {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)u, (unsigned)u, false, false);
        const unsigned r0 = r[0], r1 = r[1];
        a = __builtin_bit_cast(float, r0);
        b = __builtin_bit_cast(float, r1);
    }
}
template <int MASK>
__device__ __forceinline__ float lane_xor_add(float v) {
    float a, b;
    lane_xor_pair<MASK>(v, a, b);
    return a + b;
}
template <int MASK>
__device__ __forceinline__ float lane_xor_max(float v) {
    float a, b;
    lane_xor_pair<MASK>(v, a, b);
    return fmaxf(a, b);
}
// max over the 64 lanes of a wave of an unsigned value (DPP; every lane must be active): the result, wave-uniform
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));      // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));      // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));      // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));      // row_shr:8
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));      // row_bcast:15 into rows 1, 3
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));      // row_bcast:31 into rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// the sum of v over the 64 lanes of a wave (DPP; every lane must be active): wave-uniform
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);      // row_shr:1
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);      // row_shr:2
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);      // row_shr:4
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);      // row_shr:8
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true);      // row_bcast:15 into rows 1, 3
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true);      // row_bcast:31 into rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// the reader's side: lane l < kAmaxLines holds word l of its sequence (other lanes 0) -> the maximum, wave-uniform
__device__ __forceinline__ unsigned amax_lines_max(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 15);
}
// One WORKGROUP's contribution to the amax words of sequence b (the same b in every thread): m >= 0 per lane; `red` = one
// LDS word per wave; `spread` = any number that differs between the workgroups that finish together.  Contains a
// __syncthreads(): every thread of the workgroup must arrive.  One atomic per workgroup, nothing returned, nobody waits.
__device__ __forceinline__ void amax_commit_block(unsigned* words, int b, unsigned spread, float m, unsigned* red) {
    const unsigned mx = wave_max_u32(__float_as_uint(m));
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = red[0];
        for (int i = 1; i < nw; ++i) t = max(t, red[i]);
        if (t) atomicMax(words + (size_t)b * kAmaxSeqWords + (spread % kAmaxLines) * kAmaxLineWords, t);
    }
}
__device__ __forceinline__ float absmax4(float m, f32x4 v) {      // max(m, |v[0]| .. |v[3]|): a lane's running maximum over 16-B loads
    return fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
}
// Does sequence b start a video on this step?  `mask`: ~0 = every sequence (a first step, any B); otherwise bit b (B <= 64:
// rvdd_reset_slots) of the launch's own sequences.
__device__ __forceinline__ bool seq_latched(unsigned long long mask, int b) {
    return mask == ~0ull || (b < 64 && ((mask >> b) & 1ull));
}
#endif

// cin = 16 or 48.  Returns hipGetLastError().  variant 1, 2: A/B forms of the plain 48 -> 48 ReLU layer (rvdd_debug_conv_bench only)
hipError_t launch_conv3x3(const ConvArgs& a, int cin, int epi, hipStream_t s, int variant = 0);
size_t conv3x3_weight_floats(int cin);
// Winograd F(2x2,3x3) variant for 48 -> 48 layers; a.w = bank arranged by arrange_wino3x3 (net_convunet.hip)
hipError_t launch_wino3x3(const ConvArgs& a, int cin, int epi, hipStream_t s);   // cin: 48, or 16 = the zero-padded network input
size_t wino3x3_weight_floats();
// the same layers on the F16 matrix pipe with split f32 operands (conv3x3h.hip); a.w = the split bank arranged by
// arrange_conv3x3h (net_convunet.hip), a.wscale its scale; cin 48 (every epilogue, with or without a.acc_in, with a.ups for
// UpConv's fused upsample) or 16 (the zero-padded network input): every 3x3 conv of the convunet by default
// cout_split = false: no launch takes the output-channel split of small launches (conv3x3h.hip MT = 1; option "cout_split" 0)
hipError_t launch_conv3x3h(const ConvArgs& a, int cin, int epi, hipStream_t s, bool cout_split = true);
size_t conv3x3h_weight_bytes(int cin);
// preprocessing_layer composed with the first source of EncoderConvs[0][0]: one 5x5 conv of the 16-channel network input
// (conv3x3h.hip HGeo KS = 5; net_convunet.hip compose_pre_enc0); the fix of its border ring is launch_pre_border_fix
hipError_t launch_conv5x5h_c16(const ConvArgs& a, hipStream_t s);
// ... over the first 8 channels only (at most 8 real channels, i.e. no future frame): 25 groups in 7 chunks instead of 50 in 13
hipError_t launch_conv5x5h_c8(const ConvArgs& a, hipStream_t s);
size_t conv5x5h_weight_bytes(int cin);      // cin = 8 or 16: the channels multiplied
void conv3x3h_set_groups(int g);   // stand-alone harness (-DRVDD_CONV_GROUPS2): 2 = two groups of four waves with an 8x16 tile each

// ---- prologue.hip -- the composed first layer's border fix and zero-source pass, amax words of maps handed in
// the border ring of launch_conv5x5h_*'s output: part -= sum over the 3x3 taps d whose pixel q = p + d - 1 lies OUTSIDE the
// image of W2[d] (b1 + sum over taps e inside the image of W1[e] x(q + e - 1))
hipError_t launch_pre_border_fix(const float* netin, const float* w1, const float* b1, const float* w2, float* part, int B, int H, int W,
                                 hipStream_t s);
// What the second pass of a two-source conv (ACC_IN, EPI_RELU) leaves when its source map is all +0: out = relu(part + 0), and
// the amax words of `out` (nullable) per sequence; n = floats per sequence (a multiple of 4), part / out 16-B aligned
hipError_t launch_relu_part(const float* part, float* out, int B, int64_t n, unsigned* words, hipStream_t s);
// amax words of a dense NHWC map [B][HW][C] (the maps no split kernel's producer wrote: caller-supplied inputs and states)
hipError_t launch_amax_reduce(const float* map, int B, int64_t hw_c, unsigned* words, hipStream_t s, int up = 0);

// ---- demosaic.hip -- Hamilton-Adams demosaic of packed raw frames and its inverse, the re-mosaic
// raw [n][4][h][w] -> green plane scratch [n][2h][2w] -> RGB written at out[b*bstride + (y*W+x)*pstride + c*cstride].  raw_bstride: floats
// between the raw frames of consecutive sequences (0 = dense, 4hw): the caller's raw frames may be channel slices of a wider
// [B][4k][h][w] tensor.  `bayer` (every launcher that demosaics or re-mosaics): enum rvdd_bayer of the packed raw frames (channel k =
// CFA position (k >> 1, k & 1) of each 2x2 cell, whatever the pattern); hipErrorInvalidValue for any other value.
hipError_t launch_demosaic(const float* raw, float* green_scratch, float* out, int n, int h, int w,
                           int64_t bstride, int pstride, int cstride, hipStream_t s, int64_t raw_bstride, int bayer);
// its first half alone, for launch_netin: the green plane [n][2h][2w] (n, h, w >= 1; rbs = the raw frames' stride, never 0)
hipError_t launch_ha_green(const float* raw, float* green, int n, int h, int w, int64_t rbs, hipStream_t s, int bayer);
// HamiltonAdam(pattern).remosaick of an NHWC4 frame: the packed planes of the pattern (the inverse of its packing)
hipError_t launch_remosaick4(const float* rgb4, float* raw, int B, int H, int W, hipStream_t s, int bayer);

// ---- warp.hip -- bicubic backward warps with the raw-resolution flow (x2 bilinear upsample, align_corners=True, times 2, fused)
// src NHWC4 -> dst[(b*H*W + p)*dpstride + c], c<3.
hipError_t launch_warp3(const float* src4, const float* flow_raw, float* dst, int dpstride, int B, int H, int W, hipStream_t s);
// src NHWC48 -> dst NHWC48.  pairs = true: the gather shares loads within pairs of pixels only, never within 2 x 2 quads
// (option "warp48_pairs" 1; same bits)
hipError_t launch_warp48(const float* src, const float* flow_raw, float* dst, int B, int H, int W, hipStream_t s, int64_t flow_bstride = 0,
                         bool pairs = false);
// the same, and a 48 -> 48 projection of every warped pixel: dst = W warp(src) + bias; frag / inv_e = the projection as a
// NextProj's split-f16 fragments and scale (net_convnext.hip), applied per pixel in block floating point (warp48_proj_kernel)
hipError_t launch_warp48_proj(const float* src, const float* flow_raw, float* dst, int B, int H, int W, const float* frag,
                              int inv_e, const float* bias, hipStream_t s, int64_t flow_bstride = 0);
// generic NCHW warp with a full-resolution flow (util.flow_utils.warp), and that flow from the raw-resolution one (times mul)
hipError_t launch_warp_nchw(const float* x, const float* flow, float* y, int n, int c, int H, int W, hipStream_t s);
hipError_t launch_upsample_flow(const float* t, float* out, int nc, int h, int w, float mul, hipStream_t s);

// ---- netin.hip -- the network input of a frame-step and the bound of its maximum
// The NHWC16 network input of a step in one pass: warp3 of prev4 | demosaic of raw_cur | warp3 of next4 (or zeros when next4 == nullptr);
// flows nullptr = --no_warp.  [B][4][h][w] raw, [B][2][h][w] flows, dense inside a sequence, with raw_bstride / flow_bstride floats
// from one sequence to the next (0 = dense); green_scratch [B][2h][2w].  proj_w16 set (ConvNeXtUnet): the 16-channel map is not
// written; `proj_out` NHWC48 receives its 1x1 projection proj_w16 / proj_b (launch_proj1x1's (16, 0) arrangement) instead (netin_proj_kernel)
hipError_t launch_netin(const float* raw_cur, float* green_scratch, const float* prev4, const float* flow_prev, const float* next4,
                        const float* flow_next, float* netin, int B, int h, int w, hipStream_t s, int64_t raw_bstride,
                        int64_t flow_bstride, const float* proj_w16, const float* proj_b, float* proj_out, int bayer);
// amax words of that network input (block floating point of the split-f16 convs, below): an upper bound from the packed raw
// frames it is made of (up to three, each nullable) and from `prev_words`, words that bound the previous output (nullable)
// (zero_a / zero_b, nullable: word ranges the kernel also clears -- the next step's amax words, step.hip)
hipError_t launch_netin_bound(const float* raw_a, const float* raw_b, const float* raw_c, int B, int h, int w, int64_t raw_bstride,
                              const unsigned* prev_words, unsigned* words, hipStream_t s, unsigned* zero_a = nullptr, size_t zero_na = 0,
                              unsigned* zero_b = nullptr, size_t zero_nb = 0, unsigned long long latch = ~0ull);
// the three pre-stage kernels of a small frame-step without a future frame in one launch, same bits (enabled: option "small_prestage")
bool netin_small_applies(int B, int h, int w, bool future, bool enabled = true);
// ... at most 1024 tiles of 16x16.  Above that the same kernel forms the network input alone (words, zero_a, zero_b null: the
// bound and the clearing stay with launch_netin_bound) -- no green plane in memory; any size without a future frame
bool netin_tiled_applies(int h, int w, bool future, bool enabled = true);
// (raw_prev: the first step of a video, whose bound also covers the previous raw frame -- prev_words is null then)
hipError_t launch_netin_small(const float* raw_cur, const float* raw_prev, const float* prev4, const float* flow_prev, float* netin, int B,
                              int h, int w, int64_t raw_bstride, int64_t flow_bstride, const unsigned* prev_words, unsigned* words,
                              hipStream_t s, unsigned* zero_a, size_t zero_na, unsigned* zero_b, size_t zero_nb,
                              unsigned long long latch, int bayer);

// ---- maps.hip -- the map primitives of the nets and the loss reduction
// bilinear x2 of a NHWC48 map [B][h][w] into [B][Hout][Wout] at offset (oy,ox); pixels outside the 2h x 2w window are zero.
// align_corners selects nn.Upsample(align_corners=...) semantics.
hipError_t launch_upsample2x(const float* in, float* out, int B, int h, int w, int Hout, int Wout, int oy, int ox, bool align_corners, hipStream_t s);
hipError_t launch_maxpool2(const float* in, float* out, int B, int H, int W, hipStream_t s);
hipError_t launch_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, int Cpad, hipStream_t s);
hipError_t launch_nhwc_to_nchw(const float* in, float* out, int B, int C, int H, int W, int Cpad, hipStream_t s);
// final 1x1 conv 48->3: feat NHWC48 -> out NCHW [B][3][H][W] (+ NHWC4 copy for the next warp)
hipError_t launch_conv1x1_out(const float* feat, const float* w3x48, const float* b3, float* out_nchw,
                              float* out_nhwc4, int B, int H, int W, hipStream_t s);
// {sum|d|, sum d^2} as doubles -> host math, for `nslices` dense slices of n elements: partial[nslices][2*nblk] doubles scratch,
// result2[nslices][2]; each slice's two sums are bit for bit what a launch of that slice alone gives
hipError_t launch_loss_reduce_batch(const float* a, const float* b, int nslices, int64_t n, double* partial, int nblk,
                                    double* result2, hipStream_t s);

// ---- state.hip -- the recurrent state of single sequences of a batch: reset and moved
// rvdd_reset_slots' latch: zero the features (feat_per_seq floats per sequence) and the amax words of every set (nsets, layout
// [nsets][B][kAmaxSeqWords]) of the sequences in `mask` (B <= 64); either pointer nullable
hipError_t launch_latch_zero(unsigned long long mask, float* feat, int64_t feat_per_seq, unsigned* words, int nsets, int B, hipStream_t s);
// rvdd_move_slots: the recurrent state of sequence from[k] replaces that of sequence to[k], k < count <= kMaxMovePairs, in ONE
// launch: the previous output (den, NHWC4), the features (feat, feat_per_seq floats per sequence, nullable) and the amax words
// of every set (nullable, layout as above).  The pairs travel as kernel arguments, one byte per slot (B <= 64); they must be
// disjoint (no slot twice across from and to): the caller checks that, it is what makes one launch race-free
constexpr int kMaxMovePairs = 32;
hipError_t launch_move_slots(const int* from, const int* to, int count, float* den, int64_t den_per_seq, float* feat, int64_t feat_per_seq,
                             unsigned* words, int nsets, int B, hipStream_t s);

// -------------------------------------------------------------- ConvNeXt ---
struct NextBlockW {          // device pointers, one ConvBlock (networks/new_unet.py:74-103)
    const float* proj_w;     // [CinP][48] (k-major) or nullptr
    const float* proj_b;     // [48]
    const float* dw_w;       // [49][48]  (tap-major)
    const float* dw_b;       // [48]
    const float* ln_w;       // [48]
    const float* ln_b;       // [48]
    const float* fc1_w;      // arranged for MFMA, see net_convnext.hip
    const float* fc1_b;      // [192]
    const float* fc2_w;
    const float* fc2_b;      // [48]
    const float* ls;         // [48]
    // the fused kernel's split-f16 MLP (convnext.hip SPLIT): filter fragments of 2^s fc1 / 2^s' fc2 as f16 hi, lo halves
    // (arranged in net_convnext.hip), the scales and their inverses; fc1_h null = the f32-MFMA form
    const float* fc1_h;
    const float* fc2_h;
    float fc1_scale, fc1_inv, fc2_scale, fc2_inv;
    float gelu_c[7][2];      // gelu_phi4_scaled's constants for s = fc1_inv: C_i s^(6-i), cap / s -- each TWICE: as scalar pairs
                             // they are packed-f32 operands as they stand (hipcc 7.2 folds a splat of ONE kernel-argument scalar
                             // into the pair that starts at it, i.e. (c_i, c_i+1): wrong numbers, found the hard way)
    int pipe;                // 1 = convblock_pipe_kernel (front / back waves pipelined over tiles) instead of convblock_kernel
};
// A 48 -> 48 projection applied to a fused block's OUTPUT in its epilogue (convblock_pipe_kernel PROJ): one half of the
// 96 -> 48 projection behind a concat, proj(cat(a, b)) = Wa a + Wb b + bias (networks/new_unet.py:85-88, 321-329)
struct NextProj {
    const float* frag;       // split-f16 fragments of 2^s W [48][48] (net_convnext.hip finalize_convnext), 9 KiB
    const float* bias;       // [48] or null; used when `add` is null
    const float* add;        // NHWC48 map of the block's output size added to the projection (the other half, with the bias), or null
    int inv_e;               // -s: added to a float's exponent field it multiplies by 2^-s
};
// the whole ConvBlock in ONE kernel (convblock_kernel): x -> x + ls * MLP(LayerNorm(dwconv7x7(x))); x, out NHWC48
// [B][H][W], out != x.  _out3: also the 1x1 conv 48 -> 3 on the block's output (out_nchw [B][3][H*W], out_nhwc4
// [B][H*W][4]; either may be null)
hipError_t launch_next_block(const float* x, float* out, const NextBlockW& w, int B, int H, int W, hipStream_t s);
// the same, and MaxPool2d(2) of the block's output into pooled [B][H/2][W/2] (NHWC48) from the epilogue
hipError_t launch_next_block_pool(const float* x, float* out, float* pooled, const NextBlockW& w, int B, int H, int W, hipStream_t s);
hipError_t launch_next_block_out3(const float* x, float* out, const NextBlockW& w, int B, int H, int W, const float* w3x48,
                                  const float* b3, float* out_nchw, float* out_nhwc4, hipStream_t s);
// the fused block (pipelined split-f16 form only: w.fc1_h set) storing pj's projection of its output (+ pj.bias + pj.add) in
// place of the output; pooled (nullable): MaxPool2d(2) of the UNPROJECTED output, as launch_next_block_pool
hipError_t launch_next_block_proj(const float* x, float* out, float* pooled, const NextBlockW& w, const NextProj& pj, int B, int H,
                                  int W, hipStream_t s);
// 1x1 projection on MFMA: in1 NHWC[c1] (+ in2 NHWC[c2]) -> out NHWC48; (c1,c2) = (16,0) or (48,48)
hipError_t launch_proj1x1(const float* in1, int c1, const float* in2, int c2, const float* w,
                          const float* b, float* out, int64_t npix, hipStream_t s);
// zero_pad_features: src [B][h][w] -> dst [B][H][W] at (oy,ox), zeros elsewhere (NHWC48)
hipError_t launch_pad_copy(const float* src, float* dst, int B, int h, int w, int H, int W, int oy, int ox,
                           hipStream_t s);

// srgb.hip -- sRGB post-processing + display-domain metrics (dataset/fwd_ppipe.py)
hipError_t launch_ppipe(const float* img, int n, int H, int W, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int bit_depth,
                        const float gains[3], int iso, uint8_t* out_u8, float* out_f32, hipStream_t s);
size_t srgb_metrics_workspace(int n, int H, int W);
hipError_t launch_srgb_metrics(const uint8_t* a, const uint8_t* b, int n, int H, int W, void* ws, hipStream_t s);

// ycbcr.hip -- display images as frames of a Y'CbCr 4:2:0 video (rvdd_ycbcr; the rule: include/rvdd.h)
// disp [n][H][W][3] display values (launch_ppipe's out_f32) -> frames [n][H*W*3/2] samples, uint8 (depth 8) or uint16 (depth 10): per
// image the Y plane [H][W], then Cb, then Cr [H/2][W/2].  H, W even and >= 2; n <= 0 launches nothing
hipError_t launch_ycbcr(const float* disp, int n, int H, int W, int depth, void* frames, hipStream_t s);
// whether that launch takes the wide form (a thread owns two rows of eight pixels), and its grid; -1 = more than 2^31 - 1 blocks
bool ycbcr_wide(const float* disp, int W, const void* frames);
int64_t ycbcr_blocks(int n, int H, int W, bool wide);

// ingest.hip -- sensor frames to the inputs of a step and of TV-L1 (rvdd_ingest_raw), and rvdd_video_push's copy kernels
// frames: n frames, dtype 0 = u16 / 1 = f32, layout 0 = mosaic [n][2hh][2ww] / 1 = packed HWC [n][hh][ww][4];
// packed [n][4][hh][ww] = 2 * (dn / (2^bit_depth - 1)) - 1, gray [n][hh][ww] = (((c0 + c1) + c2) + c3) * 0.25 in DN; either nullable
hipError_t launch_ingest_raw(const void* frames, int dtype, int layout, int n, int hh, int ww, int bit_depth, float* packed, float* gray,
                             hipStream_t s);
// rgb [n][3][2hh][2ww] in [-1,1] -> gray [n][hh][ww] in DN of its re-mosaic in pattern `bayer` (enum rvdd_bayer): per cell
// (((dn0 + dn1) + dn2) + dn3) * 0.25 with dn_k = ((v_k + 1) * 0.5) * (2^bit_depth - 1), v_k the pattern's colour at CFA position k
hipError_t launch_gray_of_rgb(const float* rgb, int n, int hh, int ww, int bayer, int bit_depth, float* gray, hipStream_t s);
// The re-mosaic's colour table, the one copy of it: the RGB plane of each GBRG site -- G(e,e), B(e,o), R(o,e), G(o,o) -- and the
// phase (py << 1) | px of the pattern; CFA position k of pattern `bayer` (enum rvdd_bayer, 0..3) is the GBRG site k ^ phase
// (demosaic.h's bayer_phase).  -> the four plane indices, two bits each: col(k) = (cols >> 2k) & 3.
inline int bayer_cols(int bayer) {
    constexpr int gbrg[4] = {1, 2, 0, 1}, phase[4] = {0, 3, 2, 1};
    int cols = 0;
    for (int k = 0; k < 4; ++k) cols |= gbrg[k ^ phase[bayer]] << (2 * k);
    return cols;
}
// a denoised frame in the containers a sensor pipeline reads (rvdd_egress).  rgb [n][3][H][W] in [-1,1]; layout enum
// rvdd_out_layout (0 [n][H][W][3], 1 the mosaic [n][H][W], 2 packed [n][H/2][W/2][4]; H, W even for 1 and 2), dtype 0 = u16
// (rint, clamped to 0 .. 2^bit_depth - 1) / 1 = f32 (DN as computed), bayer ignored for layout 0
hipError_t launch_egress(const float* rgb, int n, int H, int W, int layout, int dtype, int bit_depth, int bayer, void* out, hipStream_t s);
// the grid of that launch (n, H, W >= 1) and whether it takes the wide form; -1 = more than 2^31 - 1 blocks
int64_t egress_blocks(const float* rgb, int n, int H, int W, int layout, int dtype, const void* out, bool* wide);
// The same two directions on frames of packed bit_depth = 10 / 12 / 14-bit samples (rvdd_ingest_bits, rvdd_egress_bits): order enum
// rvdd_bits_order (0 MIPI CSI-2 groups, 1 MSB-first bit string per row), rows and frames tight.  A row of 2ww samples:
inline int64_t bits_row_bytes(int ww, int bit_depth) { return (2 * (int64_t)ww * bit_depth + 7) / 8; }
// packed / gray / the u16 samples are those of launch_ingest_raw(u16 mosaic) / launch_egress(mosaic, u16) on the unpacked frames
hipError_t launch_ingest_bits(const uint8_t* frames, int order, int n, int hh, int ww, int bit_depth, float* packed, float* gray, hipStream_t s);
hipError_t launch_egress_bits(const float* rgb, int n, int H, int W, int order, int bit_depth, int bayer, uint8_t* out, hipStream_t s);
// whether those launches take the dword form (a thread owns 16 pixels of both sensor rows), and their grid; -1 = more than 2^31 - 1 blocks
bool ingest_bits_fast(const uint8_t* frames, int ww, const float* packed, const float* gray);
bool egress_bits_fast(const float* rgb, int W, const uint8_t* out);
int64_t bits_blocks(int n, int hh, int ww, bool fast);
// the flow batch of a push: I0 / I1 [npairs][hw] from the gray planes [B][hw] of the ring positions of the centre, previous and
// next (nullable: no future frame) frames.  pairs[q] = slot | direction << 6 of pair q (direction 0: (centre, previous), 1: (centre,
// next)); with npairs = B * directions -- every slot has every pair -- pair q is slot q % B, direction q / B, and pairs is not read.
// A slot whose bit of from_den is set has its (centre, previous) pair matched against dgray [B][hw] instead of gray_p (B <= 64).
hipError_t launch_stream_gather(const float* gray_c, const float* gray_p, const float* gray_n, const float* dgray, uint64_t from_den,
                                float* I0, float* I1, const uint8_t* pairs, int npairs, int B, int64_t hw, hipStream_t s);
// flows [ndir][B][2][hw] of the step from the batch's u [npairs][2][hw]: zero for every (slot, direction) without a pair (B <= 64;
// npairs = 0 zeroes them all and does not read u)
hipError_t launch_stream_scatter(const float* u, float* flows, const uint8_t* pairs, int npairs, int ndir, int B, int64_t hw, hipStream_t s);
// option "stream_all_frames": the packed frame [4][hw] of every listed slot copied between ring_prev and ring_pos [B][4][hw], the ring
// positions before this push's and this push's: previous -> this push's where bit slot of to_pos is set, the other way elsewhere
hipError_t launch_stream_dup(float* ring_prev, float* ring_pos, const int* slots, int nslots, uint64_t to_pos, int B, int64_t hw, hipStream_t s);

// dpc.hip -- dynamic defective-pixel correction of packed frames (rvdd_dpc, the stage of rvdd_video_push behind rvdd_set_dpc)
// k2_* = k_* * k_* rounded to f32 (formed once on the host); a side whose k_* is 0 is off; top is filled in by the launch
struct DpcParams {
    float k_hot, k_dead, k2_hot, k2_dead, a, b, floor, top;
};
// pin [n][4][hh][ww] -> pout (no overlap), flagged samples replaced by the median of their eight same-plane neighbours; gray [n][hh][ww]
// (nullable) re-formed at the cells with a flag; counts [n][2] u32 (nullable): hot / dead flags per frame, added.  hh, ww >= 2.
hipError_t launch_dpc(const float* pin, float* pout, float* gray, int n, int hh, int ww, int bit_depth, const DpcParams& p, unsigned* counts,
                      hipStream_t s);
// whether that launch takes the wide form (a thread owns four cells), and its grid (*per_frame: the blocks of one frame); -1 = more
// than 2^31 - 1 blocks
bool dpc_wide(const float* pin, const float* pout, const float* gray, int ww);
int64_t dpc_blocks(int n, int hh, int ww, bool wide, int64_t* per_frame);

// dpc_map.hip -- the static defect map: persistence counts per site (rvdd_dpc_detect) and the correction by map (rvdd_dpc_map_apply,
// the stage of rvdd_video_push behind rvdd_set_dpc_map)
// hits [4][hh][ww] u32 (hot frames | dead frames << 16, each half added to and saturating at 65535) of packed [n][4][hh][ww] under
// launch_dpc's rule with the (tolerate + 1)-th largest / smallest neighbour (tolerate 0..3) in place of hi / lo; a thread owns its
// sites across the n frames: plain load, add and store.  hh, ww >= 2; n <= 0 launches nothing.
hipError_t launch_dpc_detect(const float* packed, int n, int hh, int ww, int bit_depth, const DpcParams& p, int tolerate, unsigned* hits,
                             hipStream_t s);
// whether that launch takes the wide form (a thread owns four sites of a row), and its grid; -1 = more than 2^31 - 1 blocks
bool dpc_detect_wide(const float* packed, const unsigned* hits, int ww);
int64_t dpc_detect_blocks(int hh, int ww, bool wide);
// packed [n][4][hh][ww] IN PLACE, gray [n][hh][ww] (nullable) in place: the defective samples of the `ncells` cells listed in `cells`
// (DEVICE, indices y * ww + x; mask: DEVICE [hh][ww], bit k = plane k of the cell is defective) replaced by the middle of the good
// sites of the first ring that has one, the cells' gray values re-formed; one thread per (frame, cell).  hh, ww >= 3; no cell or no
// frame launches nothing.
hipError_t launch_dpc_map_apply(float* packed, float* gray, int n, int hh, int ww, int bit_depth, const uint8_t* mask, const int* cells,
                                int64_t ncells, hipStream_t s);
int64_t dpc_map_blocks(int n, int64_t ncells);      // the grid of that launch; -1 = more than 2^31 - 1 blocks

// match.hip -- footage matched to the checkpoint's noise curve (rvdd_match_raw, rvdd_unmatch_rgb, the stage behind rvdd_set_match)
// `count` dense floats in -> out (the same pointer, or no overlap): (scale * v) + offset, or with `inverse` (v - offset) * r with
// r = (float)(1.0 / (double)scale) formed here; each operation rounded to f32 on its own.  scale finite and > 0, offset finite.
hipError_t launch_match(const float* in, float* out, int64_t count, float scale, float offset, bool inverse, hipStream_t s);
// whether that launch takes the wide form (a thread owns four samples), and its grid; -1 = more than 2^31 - 1 blocks
bool match_wide(const float* in, const float* out, int64_t count);
int64_t match_blocks(int64_t count, bool wide);

// noise.hip -- block statistics of packed frames for the noise-curve estimate (rvdd_noise_hist)
struct rvdd_noise_acc;
typedef rvdd_noise_acc NoiseAcc;      // include/rvdd.h: u32 hist[64][512], u64 msum[64], u64 counters[4]
// the 8 x 8 blocks of packed [n][4][hh][ww] added to *acc (DEVICE), a lane per block; zero blocks launches nothing
hipError_t launch_noise_hist(const float* packed, int n, int hh, int ww, int bit_depth, NoiseAcc* acc, hipStream_t s);
// whether that launch takes the wide form (two 16-byte loads per block row), and its grid (*blocks: the blocks of the call; n, hh, ww
// >= 0); -1 = more than 2^31 - 1 workgroups
bool noise_wide(const float* packed, int ww);
int64_t noise_groups(int n, int hh, int ww, int64_t* blocks);

// cuts.hip -- one integer signature per frame for scene-cut detection (rvdd_frame_sigs)
struct rvdd_frame_sig;
// sig[i] (DEVICE, every word overwritten) = the signature of gray [n][hh][ww], one workgroup per (frame, band); n = 0 launches nothing;
// hh, ww >= 16, n <= (2^31 - 1) / 16
hipError_t launch_frame_sigs(const float* gray, int n, int hh, int ww, int bit_depth, rvdd_frame_sig* sig, hipStream_t s);
// whether that launch takes the wide form (16-byte loads)
bool frame_sig_wide(const float* gray, int ww);

// resid.hip -- residual statistics of outputs against their noisy frames (rvdd_resid_stats, the stage behind rvdd_set_resid)
struct rvdd_resid_acc;
// the sums of packed [n][4][hh][ww] against rgb [n][3][2hh][2ww] in pattern `bayer` added to acc[i] (DEVICE, 8-byte aligned), one
// accumulator per frame; n = 0 launches nothing; hh, ww >= 1
hipError_t launch_resid(const float* packed, const float* rgb, int n, int hh, int ww, int bayer, int bit_depth, rvdd_resid_acc* acc,
                        hipStream_t s);
// whether that launch takes the wide form (a thread owns four cells), and its grid (*groups: the workgroups of one frame); -1 = more
// than 2^31 - 1 blocks, or tensors whose element offsets leave 64 bits
bool resid_wide(const float* packed, const float* rgb, int ww);
int64_t resid_blocks(int n, int hh, int ww, bool wide, int* groups);

// rows.hip -- row noise: one offset per frame, row parity and plane row (rvdd_rows_estimate, rvdd_rows_apply, the stage behind rvdd_set_rows)
struct rvdd_rows_acc;
// k2 = k_gate * k_gate rounded to f32 (formed once on the host); top is filled in by the launch
struct RowsParams {
    float k2, a, b, floor, max_dn, top;
};
// offsets / state [n][2][hh] (DEVICE, every word written) of packed [n][4][hh][ww], the rows' counts added to acc[i] (DEVICE, nullable);
// one workgroup per (frame, parity, row).  hh >= 5, 1 <= ww <= rows_max_ww(); n <= 0 launches nothing
hipError_t launch_rows_estimate(const float* packed, int n, int hh, int ww, int bit_depth, const RowsParams& p, float* offsets, uint8_t* state,
                                rvdd_rows_acc* acc, hipStream_t s);
int rows_max_ww();                                // the widest plane a workgroup's registers hold
int64_t rows_estimate_blocks(int n, int hh);      // the grid of that launch; -1 = more than 2^31 - 1 blocks
// packed [n][4][hh][ww] IN PLACE, gray [n][hh][ww] (nullable) in place: offsets [n][2][hh] taken out of the rows where they are not zero
hipError_t launch_rows_apply(float* packed, float* gray, const float* offsets, int n, int hh, int ww, int bit_depth, hipStream_t s);
// whether an apply launch of rows.hip or cols.hip takes the wide form (a thread owns four cells: ww % 4 == 0 and every tensor it is
// given 16-byte aligned), and its grid of kLineApplyThreads (*per_frame: the blocks of one frame); -1 = more than 2^31 - 1 blocks
constexpr int kLineApplyThreads = 256;
template <class... T>
inline bool line_apply_wide(int ww, const T*... tensors) {
    return (ww & 3) == 0 && ((reinterpret_cast<uintptr_t>(tensors) | ...) & 15) == 0;
}
inline int64_t line_apply_blocks(int n, int hh, int ww, bool wide, int64_t* per_frame) {
    const int64_t per = (int64_t)hh * (wide ? ww >> 2 : ww);         // threads per frame
    const int64_t bpf = (per + kLineApplyThreads - 1) / kLineApplyThreads;
    if (per_frame) *per_frame = bpf;
    if (bpf > 0x7fffffffll || (bpf > 0 && n > 0x7fffffffll / bpf)) return -1;
    return n * bpf;
}

// cols.hip -- column fixed-pattern noise: one offset per frame, column parity and plane column (rvdd_cols_estimate), a static map
// taken out (rvdd_cols_apply, the stage behind rvdd_set_cols).  The gate's parameters are RowsParams (max_dn is not read: no clamp here)
// offsets / state [n][2][ww] (DEVICE, every word written) of packed [n][4][hh][ww]; one workgroup per (frame, parity, strip of
// cols_strip(hh) columns).  1 <= hh <= cols_max_hh(), ww >= 5; n <= 0 launches nothing
hipError_t launch_cols_estimate(const float* packed, int n, int hh, int ww, int bit_depth, const RowsParams& p, float* offsets, uint8_t* state,
                                hipStream_t s);
int cols_max_hh();                                       // the tallest plane whose column keys fit a CU's LDS four columns at a time
int cols_strip(int hh);                                  // the columns of a workgroup's strip: 32, 16, 8 or 4
int64_t cols_estimate_blocks(int n, int hh, int ww);     // the grid of that launch; -1 = more than 2^31 - 1 blocks
// packed [n][4][hh][ww] IN PLACE, gray [n][hh][ww] (nullable) in place: map [2][ww] (DEVICE, DN) taken out of the columns where it is not zero
hipError_t launch_cols_apply(float* packed, float* gray, const float* map, int n, int hh, int ww, int bit_depth, hipStream_t s);

// green.hip -- green imbalance: the gain of the green plane of CFA row 0 (A) against that of CFA row 1 (B) per frame and block of
// RVDD_GREEN_BLOCK^2 cells (rvdd_green_estimate), a static map taken out (rvdd_green_apply, the stage behind rvdd_set_green).  The
// gate's parameters are RowsParams (max_dn is not read)
inline int green_plane_a(int bayer) { return bayer >= 2 ? 1 : 0; }      // enum rvdd_bayer -> plane A: 0 (GBRG, GRBG) or 1 (RGGB, BGGR); B is 3 - A
void green_grid(int hh, int ww, int* gh, int* gw);                       // the blocks of a frame: ceil(hh / 32) x ceil(ww / 32)
int64_t green_estimate_blocks(int n, int hh, int ww);                    // the grid of the estimate's launch; -1 = more than 2^31 - 1 blocks
// e / level / state [n][gh][gw] (DEVICE, every word written) of packed [n][4][hh][ww]; one workgroup per (frame, block).  hh, ww >= 2;
// n <= 0 launches nothing
hipError_t launch_green_estimate(const float* packed, int n, int hh, int ww, int bit_depth, int bayer, const RowsParams& p, float* e, float* level,
                                 uint8_t* state, hipStream_t s);
// packed [n][4][hh][ww] IN PLACE, gray [n][hh][ww] (nullable) in place: the gains map [gh][gw] (DEVICE; the frame's grid, or [1][1])
// interpolated per cell and taken out of the two green planes where they are not zero; the grid is line_apply_blocks'
hipError_t launch_green_apply(float* packed, float* gray, const float* map, int gh, int gw, float black, int n, int hh, int ww, int bit_depth,
                              int bayer, hipStream_t s);

// unprocess.hip -- sRGB video to the raw dataset's four images (dataset/generate_raw_from_RGB.py) and the random planes alone
// srgb [n][2hh][2ww][3] u8; g: the three inverted gains; dither [n][2hh][2ww][3] / normal [n][hh][ww][4] nullable (drawn from
// (seed, frame0 + image) then); lin_f32 / lin_u16 [n][2hh][2ww][3], gt_raw / noisy [n][hh][ww][4], each nullable
hipError_t launch_unprocess(const uint8_t* srgb, int n, int hh, int ww, const float g[3], int iso, int bayer, const float* dither,
                            const float* normal, uint64_t seed, int64_t frame0, float* lin_f32, uint16_t* lin_u16, float* gt_raw, float* noisy,
                            hipStream_t s);
hipError_t launch_unprocess_draws(uint64_t seed, int64_t frame0, int n, int hh, int ww, float* dither, float* normal, hipStream_t s);

// ------------------------------------------------------------------ TV-L1 --
struct Tvl1Workspace;
hipError_t tvl1_alloc(Tvl1Workspace** out, int nx, int ny);
void tvl1_free(Tvl1Workspace* w);
int tvl1_num_scales(int nx, int ny);
bool tvl1_size_ok(int nx, int ny);   // false where the reference's own pyramid reads out of bounds (very skinny images)
// I0, I1 [ny][nx] -> u [2][ny][nx]; synchronises the stream every few iterations (convergence peek)
hipError_t tvl1_run(Tvl1Workspace* w, const float* I0, const float* I1, float* u, hipStream_t st, int* total_iters);
hipError_t tvl1_run_batch(Tvl1Workspace* w, const float* I0, const float* I1, float* u, int n, hipStream_t st, int* iters, bool async = false);
hipError_t tvl1_check(Tvl1Workspace* w, hipStream_t st);      // what an asynchronous batch left unread (synchronises when something is pending)
int tvl1_ws_nx(const Tvl1Workspace* w);
int tvl1_ws_ny(const Tvl1Workspace* w);
