// Host side of librvdd_hip.so: the handle, the host types of both nets and of a frame-step, and the functions that cross
// the host translation units (handle, net_convunet, net_convnext, step, stream, stages, ops, profile).  Kernel files do not
// include it: what they share with the host is rvdd_internal.h.  Nothing here is exported: the library's dynamic symbols
// are the rvdd_ functions of include/rvdd.h alone (rvdd.map).
#pragma once
#include "../../include/rvdd.h"
#include "rvdd_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

struct Conv3 {            // one 3x3 conv layer, split per 48-channel source
    int nsrc = 0;
    int cin_real[2] = {0, 0};
    int cin_pad[2] = {0, 0};
    float* w[2] = {nullptr, nullptr};
    float* wu[2] = {nullptr, nullptr};   // Winograd F(2x2,3x3) transformed bank (48-channel sources only)
    float* wh[2] = {nullptr, nullptr};   // split-f16 banks of conv3x3h.hip (hi / lo halves of 2^s w; 48-channel sources only)
    float wh_inv[2] = {1.f, 1.f};        // 2^-s of each
    float* bias = nullptr;
};

struct ProfClass {
    std::string name;
    int64_t seen = 0;
    int64_t launches = 0;
    double ms = 0, flops = 0, bytes = 0;
};
struct ProfPending {
    int cls;
    hipEvent_t e0, e1;
};

struct NextBlk {          // one ConvBlock of the ConvNeXt net (networks/new_unet.py:74-103)
    NextBlockW w{};
    int c1 = 0, c2 = 0;   // projection sources (0,0 = identity)
    // a 96 -> 48 projection as two halves for the epilogues of the blocks that form its two sources (convnext.hip PROJ):
    // half[0] over the first 48 input channels (frag, inv_e set; bias = proj_b), half[1] over the last 48 (no bias)
    NextProj half[2] = {};
};

// Every entry point acts on the handle's device, whatever the caller's current device is, and leaves
// the caller's current device as it found it.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// The 3x3 conv layers of the convunet by position in the schedule (run_convunet): names are resolved ONCE, in
// rvdd_finalize_weights, into h->cu[]; a frame-step touches no string and no map.
enum CuLayer {
    CU_PRE, CU_ENC0_0, CU_ENC0_1, CU_DOWN0, CU_ENC1_0, CU_ENC1_1, CU_DOWN1, CU_ENC2_0, CU_ENC2_1, CU_DOWN2, CU_ENC3_0,
    CU_ENC3_1, CU_BOT0, CU_BOT1, CU_UP0, CU_DEC0_0, CU_DEC0_1, CU_UP1, CU_DEC1_0, CU_DEC1_1, CU_UP2, CU_DEC2_0, CU_DEC2_1,
    CU_POST, CU_COUNT
};
inline const char* const kCuNames[CU_COUNT] = {
    "preprocessing_layer", "EncoderConvs.0.blocks.0.0", "EncoderConvs.0.blocks.1.0", "EncoderDown.0.conv",
    "EncoderConvs.1.blocks.0.0", "EncoderConvs.1.blocks.1.0", "EncoderDown.1.conv", "EncoderConvs.2.blocks.0.0",
    "EncoderConvs.2.blocks.1.0", "EncoderDown.2.conv", "EncoderConvs.3.blocks.0.0", "EncoderConvs.3.blocks.1.0",
    "bottleneck.0.0", "bottleneck.1.0", "DecoderUp.0.up.1", "DecoderConvs.0.blocks.0.0", "DecoderConvs.0.blocks.1.0",
    "DecoderUp.1.up.1", "DecoderConvs.1.blocks.0.0", "DecoderConvs.1.blocks.1.0", "DecoderUp.2.up.1",
    "DecoderConvs.2.blocks.0.0", "DecoderConvs.2.blocks.1.0", "PostConvs.0.0"};
constexpr int cu_enc(int level, int j) { return level == 0 ? CU_ENC0_0 + j : CU_ENC1_0 + 3 * (level - 1) + j; }
constexpr int cu_down(int i) { return CU_DOWN0 + 3 * i; }
constexpr int cu_up(int i) { return CU_UP0 + 3 * i; }
constexpr int cu_dec(int i, int j) { return CU_DEC0_0 + 3 * i + j; }
// amax words (rvdd_internal.h: block floating point of the split-f16 kernels): one slot of B x kAmaxSeqWords words per map a
// split kernel reads.  A SET of regular slots -- the output of every conv layer (its CuLayer), the network input, the features
// a caller hands to rvdd_unet_forward -- is written during one forward and must be zero when it starts.  Three sets: frame-steps
// use sets 0 and 1 in turn, and the first kernel of a step (netin_bound_kernel) zeroes the OTHER set for the step after it
// (nobody touches that set during this step; a memset node per step cost 2 % of a 0.3 ms frame); rvdd_unet_forward uses set 2
// and zeroes it itself.  The RECURRENT features' words cross the step boundary: the map PostConvs[0] writes in step t is the
// map step t + 1 gathers its warped features from (a bicubic gather never exceeds 1.9 x the map's maximum, far inside the
// margin of the scaling, so the warped map shares the words) -- three slots in rotation: step t reads (t + 2) % 3, writes
// t % 3, and its first kernel zeroes (t + 1) % 3.
enum { AMAX_REL_NETIN = CU_COUNT, AMAX_REL_FWDFEAT, AMAX_NREG };
enum { AMAX_FEAT0 = 3 * AMAX_NREG, AMAX_SLOTS = AMAX_FEAT0 + 3 };

// The ConvBlocks of the ConvNeXt net by position in the schedule (run_convnext), resolved once like the above.
enum NxBlock {
    NX_PRE, NX_ENC0_0, NX_ENC0_1, NX_DOWN0, NX_ENC1_0, NX_ENC1_1, NX_DOWN1, NX_ENC2_0, NX_ENC2_1, NX_DOWN2, NX_ENC3_0,
    NX_ENC3_1, NX_BOT0, NX_BOT1, NX_UP0, NX_DEC0_0, NX_DEC0_1, NX_UP1, NX_DEC1_0, NX_DEC1_1, NX_UP2, NX_DEC2_0, NX_DEC2_1,
    NX_POST0, NX_POST1, NX_COUNT
};
inline const char* const kNxNames[NX_COUNT] = {
    "preprocessing_layer.blocks.0", "encoder_convs.0.blocks.0", "encoder_convs.0.blocks.1", "encoder_downs.0.postconv",
    "encoder_convs.1.blocks.0", "encoder_convs.1.blocks.1", "encoder_downs.1.postconv", "encoder_convs.2.blocks.0",
    "encoder_convs.2.blocks.1", "encoder_downs.2.postconv", "encoder_convs.3.blocks.0", "encoder_convs.3.blocks.1",
    "bottleneck.blocks.0", "bottleneck.blocks.1", "decoder_ups.0.postconv", "decoder_convs.0.blocks.0",
    "decoder_convs.0.blocks.1", "decoder_ups.1.postconv", "decoder_convs.1.blocks.0", "decoder_convs.1.blocks.1",
    "decoder_ups.2.postconv", "decoder_convs.2.blocks.0", "decoder_convs.2.blocks.1", "postprocessing.0.blocks.0",
    "postprocessing.0.blocks.1"};
constexpr int nx_enc(int level, int j) { return level == 0 ? NX_ENC0_0 + j : NX_ENC1_0 + 3 * (level - 1) + j; }
constexpr int nx_down(int i) { return NX_DOWN0 + 3 * i; }
constexpr int nx_up(int i) { return NX_UP0 + 3 * i; }
constexpr int nx_dec(int i, int j) { return NX_DEC0_0 + 3 * i + j; }

struct Level {
    int H = 0, W = 0;
    float* t[3] = {nullptr, nullptr, nullptr};
    float* skip = nullptr;
    float* part = nullptr;      // convunet only
};

// Which kernel runs the convunet's 3x3 convs: the values of option "conv_kernel".
enum ConvSel {
    CONV_SPLIT16 = 0,   // the default: the F16 matrix pipe with split f32 operands (conv3x3h.hip) wherever a layer has that bank
    CONV_DIRECT = 1,    // the direct f32 kernel everywhere
    CONV_WINO = 2,      // the Winograd f32 kernel everywhere, also where it is the slower choice (tests, A/B measurements)
    CONV_F32 = 4        // f32 kernels, direct or Winograd by launch size (wino_applies)
};

// Everything rvdd_set_option sets, per handle; one row of RVDD_OPTIONS each (include/rvdd.h describes them).  All int: a row
// names its field by one kind of member pointer; flags hold 0 or 1.
struct Options {
    int no_warp = 0;          // --no_warp: previous output / features / next frame enter the net unwarped
    int warp_raw = 0;         // --warp_raw: warp the re-mosaicked frames at raw resolution, demosaic afterwards
    int prev_noisy = 0;       // --prev_noisy_frame: the next step's "previous frame" is the demosaiced noisy one
    int bayer = 0;            // enum rvdd_bayer of the packed raw frames: every demosaic and re-mosaic of a step
    int conv = CONV_SPLIT16;  // enum ConvSel
    int bfp = 1;              // block floating point of the split-f16 convs (amax words per map and sequence); 0: operands split as
                              // they are, the round-3 behaviour with its 2^-14 .. 65504 domain -- A/B reference only
    int seq_major = 0;        // 1 = full-resolution stages one sequence at a time (see seq_major_on)
    int fuse_upsample = 1;    // UpConv's bilinear x2 inside the patch load of the conv behind it (0: separate kernel)
    int cout_split = 1;       // split-f16 convs: small launches give a tile to three workgroups of 16 output channels (conv3x3h.hip MT = 1)
    int small_prestage = 1;   // the three pre-stage kernels of a small frame-step without a future frame as one (netin_small_kernel)
    int fuse_pre = 1;         // feat nets: preprocessing_layer and EncoderConvs[0][0] composed (0: one after the other, A/B reference)
    int pre5_cin8 = 1;        // 0: the 13-chunk bank of that composition also where the 7-chunk one exists (A/B reference)
    int warp48_pairs = 0;     // 1: the feature warp shares its gather within pairs of pixels only, not within 2x2 quads (A/B reference)
    int next_split = 1;       // ConvNeXt, fused blocks: the two 1x1 convs on the F16 matrix pipe with split f32 operands (0: f32 MFMA)
    int next_pipe = 1;        // ConvNeXt, fused split-f16 blocks as a front / back pipeline over tiles (0: convblock_kernel's phases)
    int next_pool = 1;        // ConvNeXt, fused blocks: MaxPool2d(2) from the epilogue of the block in front of a DownConv
    int next_projfuse = 1;    // ConvNeXt, pipelined split-f16 blocks: the 96 -> 48 projection behind a concat as two halves in the
                              // epilogues of the blocks that form the concatenated maps (0: proj1x1_kernel)
    int tvl1_async = 0;       // rvdd_tvl1flow_batch without iteration counts enqueues and returns
    int stream_reset_each = 0;            // every ready step of rvdd_video_push carries the reset mark of every ready slot
    int stream_flow_from_denoised = 0;    // rvdd_video_push: the flow towards the previous frame is matched against the previous output
    int stream_all_frames = 0;            // rvdd_video_push: also a video's first frame and, on an IDLE behind its last frame, that frame
    int stream_container = 0;             // rvdd_video_push: the frames are packed 10 / 12 / 14-bit samples, 1 = MIPI CSI-2, 2 = MSB first (0: one number each)
    int use_graphs = 0;       // replay captured frame-steps (measured slower, off)

    bool split16() const { return conv == CONV_SPLIT16; }
    bool wino_allowed() const { return conv != CONV_DIRECT; }
    bool wino_forced() const { return conv == CONV_WINO; }
};

struct rvdd_handle {
    rvdd_cfg cfg{};
    std::string err;
    bool finalized = false;
    uint64_t reset_marks = 0;     // the sequences that start a video on the next step that covers them: slots_below(batch) = all of them
                                  // (create, rvdd_reset), some after rvdd_reset_slots (B <= 64; beyond that only none or all occur)
    uint64_t undef_mask = 0;      // rvdd_step_live / rvdd_move_slots: the sequences whose recurrent state is undefined (they sat a step out, or
                                  // were moved away); a step may cover one only together with a reset mark for it
    Options opt;                  // what rvdd_set_option sets (kOptions)
    bool serpentine = false;      // sequence order of the next forward (flips with every one when seq_major is on)
    std::map<std::string, HostTensor> staged;
    std::vector<void*> allocs;

    // weights
    Conv3 cu[CU_COUNT];       // convunet layers in schedule order (CuLayer)
    // preprocessing_layer composed with the first source of EncoderConvs[0][0] (feat nets; conv3x3h.hip HGeo, KS = 5)
    float* pre5_w = nullptr;  // the composed 5x5 bank (split f16)
    float pre5_inv = 1.f;
    float* pre5_b = nullptr;  // [48] composed bias
    float* pre5_w8 = nullptr; // the same bank over the first 8 input channels only (7 chunks instead of 13): at most 8 real channels, else null
    float pre5_inv8 = 1.f;
    float* pre_w1 = nullptr;  // [9][16][48]: preprocessing_layer weight, tap-major, input channel, its output channel m (border fix)
    float* pre_b1 = nullptr;  // [48]
    float* pre_w2 = nullptr;  // [9][48 m][48 o]: EncoderConvs[0][0] weight over the preprocessing layer's channels (border fix)
    float* w_out = nullptr;   // [3][48]
    float* b_out = nullptr;   // [3]
    NextBlk nx[NX_COUNT];     // ConvNeXt blocks in schedule order (NxBlock)

    // workspace
    Level lv[4];
    float* netin = nullptr;      // NHWC16
    float* lastden4 = nullptr;   // NHWC4
    float* next4 = nullptr;      // NHWC4
    float* green = nullptr;      // [B][H][W]
    float* featw = nullptr;      // NHWC48 warped features
    float* lastfeat = nullptr;   // NHWC48 recurrent features
    unsigned* amax = nullptr;    // [AMAX_SLOTS][B][kAmaxSeqWords] max |x| per map and sequence, zeroed at the start of every forward
    int step_ctr = 0;            // frame-steps enqueued, mod 6: picks the amax slots of a step (step_amax)
    double* loss_batch = nullptr;    // rvdd_psnr_l1[_batch]: partial sums and results of every slice (ensure_loss_batch)
    size_t loss_batch_cap = 0;       // doubles
    float* scratch = nullptr;
    size_t scratch_bytes = 0;
    Tvl1Workspace* tvl1 = nullptr;   // cached for the last (nx, ny)

    // rvdd_video_push: the last 2 + future ingested frames of every slot, allocated by the first push.  The slots share ONE
    // ring position per push (push k writes position k % depth of every slot that gets a frame), so the centre, previous and
    // next frames of all slots are dense [B] tensors and the step takes them without a copy.
    struct Stream {
        int depth = 0;               // 2 + future
        float* packed = nullptr;     // [depth][B][4][hh][ww]
        float* gray = nullptr;       // [depth][B][hh][ww]
        float* I0 = nullptr;         // [(1 + future) B][hh][ww]: the flow batch's operands (launch_stream_gather)
        float* I1 = nullptr;
        float* u = nullptr;          // [(1 + future) B][2][hh][ww]: its flows when only some slots are ready
        float* flows = nullptr;      // [1 + future][B][2][hh][ww]: flow_prev | flow_next of the step
        uint64_t pushes = 0;
        std::vector<int> count;      // per slot: frames of its video pushed in a row (0: never started, or idle on the last push)
        std::vector<uint8_t> was_idle;
        std::vector<uint8_t> head;   // per slot: its video's FIRST came under option "stream_all_frames" and left frame 0 also in the ring
                                     // position before its own, where a head's step reads the previous frame
        float* dgray = nullptr;      // [B][hh][ww]: gray plane of every slot's last output (option "stream_flow_from_denoised"; allocated by
                                     // the first push that has the option on)
        std::vector<uint8_t> dgray_ok;   // per slot: dgray holds the output of the push before this one
    } st;

    // rvdd_set_dpc: defective-pixel correction between the ingest and the ring of rvdd_video_push
    struct Dpc {
        bool on = false;
        DpcParams p{};                   // the checked parameters (dpc_params)
        float* in = nullptr;             // [B][4][hh][ww]: where a push with the stage on ingests the packed planes (allocated by the first)
        unsigned* counts = nullptr;      // DEVICE [B][2]: hot / dead flags per slot since rvdd_dpc_counts last folded them into `total`
        std::vector<uint64_t> total;     // [B][2] since the stage was last switched on
    } dpc;

    // rvdd_set_dpc_map: the static defect map rvdd_dpc_map_apply corrects by, and the stage of rvdd_video_push behind the ingest
    struct DpcMap {
        bool on = false;
        int hh = 0, ww = 0;              // the map's size in cells
        uint8_t* mask = nullptr;         // DEVICE [hh][ww]: bit k = plane k of the cell is defective (freed by rvdd_set_dpc_map / rvdd_destroy)
        int* cells = nullptr;            // DEVICE [ncells]: the indices y * ww + x of the defective cells, ascending
        int64_t ncells = 0;
    } dmap;

    // rvdd_set_match: the ring's packed frames mapped onto the checkpoint's noise curve, out_rgb mapped back (rvdd_video_push)
    struct Match {
        bool on = false;
        rvdd_match_cfg cfg{};            // the checked coefficients (match_params)
    } match;

    // rvdd_set_resid: residual statistics of every output against its centre frame (rvdd_video_push), read by rvdd_resid_read
    struct Resid {
        bool on = false;
        rvdd_resid_acc* acc = nullptr;   // DEVICE [B]: one accumulator per slot (allocated by the first push that has the stage on)
    } resid;

    // rvdd_set_rows: row noise taken out of the ring's frames behind the correction (rvdd_video_push), counted for rvdd_rows_read
    struct Rows {
        bool on = false;
        RowsParams p{};                  // the checked parameters (rows_params)
        float* offsets = nullptr;        // DEVICE [B][2][hh]: the offsets of every slot's last frame (allocated by the first push that has the stage on)
        uint8_t* state = nullptr;        // DEVICE [B][2][hh]
        rvdd_rows_acc* acc = nullptr;    // DEVICE [B]: one accumulator per slot
    } rows;

    // rvdd_set_cols: the static column map taken out of the ring's frames behind the correction and in front of the rows (rvdd_video_push)
    struct Cols {
        bool on = false;
        int ww = 0;                      // the map's width in cells
        float* map = nullptr;            // DEVICE [2][ww]: DN of the pushes' bit depth (freed by rvdd_set_cols / rvdd_destroy)
    } cols;

    // rvdd_set_green: the static map of green gains taken out of the ring's frames behind the rows and in front of the match (rvdd_video_push)
    struct Green {
        bool on = false;
        int gh = 0, gw = 0;              // the map's grid: a frame's blocks, or 1 x 1 for a flat gain
        float black = 0.0f;              // the level without signal, DN of the pushes' bit depth
        float* map = nullptr;            // DEVICE [gh][gw]: gains of plane A relative to plane B (freed by rvdd_set_green / rvdd_destroy)
    } geq;

    // hipGraph replay of a frame-step (see rvdd_step)
    struct StepKey {
        const void* p[6];
        int64_t stride[2];
        int flags;
        bool operator<(const StepKey& o) const {
            if (const int c = std::memcmp(p, o.p, sizeof p)) return c < 0;
            if (const int c = std::memcmp(stride, o.stride, sizeof stride)) return c < 0;
            return flags < o.flags;
        }
    };
    struct StepGraph {
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        uint64_t last_use = 0;
    };
    std::map<StepKey, StepGraph> graphs;
    uint64_t graph_tick = 0;
    bool ran_eagerly = false;       // the first step of a handle is never captured (it sets the kernels' attributes)
    hipStream_t gstream = nullptr;  // the stream the graphs are captured on and replayed in
    hipEvent_t g_in = nullptr, g_out = nullptr;

    // measurement
    bool prof_on = false;
    std::string prof_filter;      // empty = every kernel class
    int prof_stride = 1;          // bracket every prof_stride-th launch of a class
    std::vector<ProfClass> prof;
    std::vector<ProfPending> pending;
    std::vector<hipEvent_t> event_pool;
    hipEvent_t t0 = nullptr, t1 = nullptr;

    bool has_feat() const { return cfg.arch == RVDD_ARCH_CONVUNET_FEAT || cfg.arch == RVDD_ARCH_CONVNEXT_FEAT; }
    bool is_next() const { return cfg.arch == RVDD_ARCH_CONVNEXT || cfg.arch == RVDD_ARCH_CONVNEXT_FEAT; }
    bool amax_on() const { return opt.bfp && opt.split16() && !is_next(); }      // the convs read amax words (block floating point)
    int cin_real() const { return 3 * (2 + cfg.future); }
};

inline uint64_t slots_below(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }      // slots [0, n) as a mask (every slot it has, from 64 on)

int fail(rvdd_t* h, int code, const char* fmt, ...);      // sets the handle's (h null: the thread's create) error string, returns code

#define RC(expr)               \
    do {                       \
        int rc__ = (expr);     \
        if (rc__) return rc__; \
    } while (0)

// The refusals the entry points of ops.hip, stream.hip and stages.hip share, each with the sentence its callers wrote out by hand before:
// 0, or RVDD_ERR_ARG through fail().  A call site uses one only where this IS its sentence, byte for byte (tests/abi_refusals.cpp and
// its golden hold every one); combined and differently worded refusals stay written out where they are.  `fn`: the entry point's name.
inline int need_bit_depth(rvdd_t* h, const char* fn, int bit_depth) {
    return bit_depth < 1 || bit_depth > 16 ? fail(h, RVDD_ERR_ARG, "%s: bit_depth must be 1..16, got %d", fn, bit_depth) : RVDD_OK;
}
inline int need_bayer(rvdd_t* h, const char* fn, int pattern) {
    return pattern < RVDD_BAYER_GBRG || pattern > RVDD_BAYER_BGGR
               ? fail(h, RVDD_ERR_ARG, "%s: pattern %d is not an rvdd_bayer (0 GBRG, 1 GRBG, 2 RGGB, 3 BGGR)", fn, pattern) : RVDD_OK;
}
inline int need_count(rvdd_t* h, const char* fn, int n) { return n < 0 ? fail(h, RVDD_ERR_ARG, "%s: n must be >= 0, got %d", fn, n) : RVDD_OK; }
inline int need_ptr(rvdd_t* h, const char* fn, const void* p, const char* name) {
    return p ? RVDD_OK : fail(h, RVDD_ERR_ARG, "%s: %s is required", fn, name);
}
// several of them, refused in the order given
inline int need_ptrs(rvdd_t* h, const char* fn, std::initializer_list<std::pair<const void*, const char*>> ptrs) {
    for (const auto& p : ptrs) RC(need_ptr(h, fn, p.first, p.second));
    return RVDD_OK;
}
// `why`: the reason in the sentence's parentheses, or null for the sentence without them
inline int need_min(rvdd_t* h, const char* fn, const char* name, int v, int least, const char* why = nullptr) {
    if (v >= least) return RVDD_OK;
    return why ? fail(h, RVDD_ERR_ARG, "%s: %s must be >= %d (%s), got %d", fn, name, least, why, v)
               : fail(h, RVDD_ERR_ARG, "%s: %s must be >= %d, got %d", fn, name, least, v);
}
// the refusal of a launch over `product` (the caller's words, "n * hh * ww") of more than 2^31 - 1 blocks: `blocks` is the kernel's own count, -1 for that
inline int need_blocks(rvdd_t* h, const char* fn, int64_t blocks, const char* product, int a, int b, int c) {
    return blocks < 0 ? fail(h, RVDD_ERR_ARG, "%s: %s = %d * %d * %d needs a launch of more than 2^31 - 1 blocks", fn, product, a, b, c) : RVDD_OK;
}

#define ENTER(h)                                                                            \
    DeviceGuard guard__((h)->cfg.device);                                                   \
    if (guard__.err != hipSuccess)                                                          \
        return fail((h), RVDD_ERR_HIP, "cannot select device %d: %s", (h)->cfg.device, hipGetErrorString(guard__.err))

#define HIPCHK(h, expr)                                                                     \
    do {                                                                                    \
        hipError_t e__ = (expr);                                                            \
        if (e__ != hipSuccess)                                                              \
            return fail((h), RVDD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                \
    } while (0)

// the amax words (rvdd_internal.h) of map `slot`, from sequence b0 on
inline unsigned* amax_words(const rvdd_t* h, int slot, size_t b0 = 0) { return h->amax + ((size_t)slot * h->cfg.batch + b0) * kAmaxSeqWords; }
constexpr size_t amax_bytes(int B, int nslots) { return (size_t)nslots * B * kAmaxSeqWords * sizeof(unsigned); }

// The amax slots of one forward: the first slot of its regular set, and the absolute slots it reads the old features' words
// from / writes the new ones to.  A frame-step's follow step_ctr; rvdd_unet_forward has a set of its own, so that the
// frame-steps' sets and the recurrent slots stay untouched.
struct AmaxSlots {
    int base = 0, feat_in = 0, post_out = 0;
};
constexpr AmaxSlots step_amax(int ctr) { return {(ctr & 1) * AMAX_NREG, AMAX_FEAT0 + (ctr + 2) % 3, AMAX_FEAT0 + ctr % 3}; }
constexpr AmaxSlots forward_amax() { return {2 * AMAX_NREG, 2 * AMAX_NREG + AMAX_REL_FWDFEAT, 2 * AMAX_NREG + CU_POST}; }

// What a frame-step does in front of the net (run_prologue: demosaic, warps) works on: the caller's frame and flow pointers of one step.
struct StepInputs {
    const float* raw_prev = nullptr;      // only on the first step of a video (of any sequence)
    unsigned long long latch = 0;         // the sequences that start a video on this step: ~0 = all, else bit b (B <= 64)
    const float* raw_cur = nullptr;
    const float* raw_next = nullptr;
    const float* flow_prev = nullptr;
    const float* flow_next = nullptr;
    size_t rawf = 0, flowf = 0;       // floats from one sequence to the next in the caller's raw / flow tensors
};

// One forward of the net, handed down to everything that launches for it: a frame-step (enqueue_step) or a bare
// rvdd_unet_forward.
struct NetRun {
    int n = 0;                        // the sequences it covers: slots [0, n) of the handle's maps
    AmaxSlots amax;
    bool zero_pending = false;        // the first network-input launch zeroes the set and features slot of the step after (run_prologue)
    bool netin_proj = false;          // lv[0].t[0] already holds the first ConvBlock's projection of the network input (run_prologue)
    bool featw_proj = false;          // `featw` holds W_f warp(features) + bias (run_prologue, next_pf_pre), not the warped features
    bool zero_feat = false;           // the first step of a video for every sequence, composed first layer: the recurrent features are
                                      // zero, nobody warps or convolves them (enqueue_step, run_convunet) -- `featw` is not written
    const StepInputs* in = nullptr;   // what a frame-step does in front of the net (run_prologue); null for rvdd_unet_forward
};
inline int amax_layer(const NetRun& run, int layer) { return run.amax.base + layer; }

struct ConvCall {
    const float* in = nullptr;
    int src = 0;             // which weight slice of the layer
    const float* acc_in = nullptr;
    int epi = EPI_RELU;
    const float* res1 = nullptr;
    const float* res2 = nullptr;
    float* out = nullptr;
    int H = 0, W = 0;        // conv domain
    int Hout = 0, Wout = 0, oy = 0, ox = 0;
    float* out3_nchw = nullptr;    // EPI_RELU_OUT3 targets
    float* out3_nhwc4 = nullptr;
    bool ups = false;        // `in` is the half-resolution map whose bilinear x2 upsample the conv reads (UpConv)
    int amax_in = -1;        // amax slot of `in` (-1: no scaling) and of `out` (-1: no split kernel reads it)
    int amax_out = -1;
    int variant = 0;         // launch_conv3x3's A/B forms (rvdd_debug_conv_bench only)
};

// Sequences [b0, b0 + nb) of the batch: the maps of a ConvCall are those of the WHOLE batch, a launch may cover a part.
struct Sub {
    int b0, nb;
};

// ---- profile.hip
int prof_class(rvdd_t* h, const char* name);
hipEvent_t get_event(rvdd_t* h);

struct Scope {   // brackets one launch with events when profiling is on
    rvdd_t* h;
    hipStream_t s;
    int cls = -1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    Scope(rvdd_t* h_, hipStream_t s_, const char* name, double flops, double bytes) : h(h_), s(s_) {
        if (!h->prof_on) return;
        if (!h->prof_filter.empty() && h->prof_filter != name) return;
        const int c = prof_class(h, name);
        if (h->prof[c].seen++ % h->prof_stride) return;
        cls = c;
        h->prof[cls].flops += flops;
        h->prof[cls].bytes += bytes;
        h->prof[cls].launches += 1;
        e0 = get_event(h);
        e1 = get_event(h);
        (void)hipEventRecord(e0, s);
    }
    ~Scope() {
        if (cls < 0) return;
        (void)hipEventRecord(e1, s);
        h->pending.push_back({cls, e0, e1});
    }
};

// fn(b, e) for every maximal run [b, e) of consecutive slots i < n with pred(i), in order; a non-zero return of fn ends the walk
// and is handed back
template <class Pred, class Fn>
int for_each_run(int n, Pred pred, Fn fn) {
    for (int b = 0; b < n;) {
        if (!pred(b)) { ++b; continue; }
        int e = b + 1;
        while (e < n && pred(e)) ++e;
        RC(fn(b, e));
        b = e;
    }
    return RVDD_OK;
}

// ---- handle.hip
int dmalloc(rvdd_t* h, void** p, size_t bytes, bool zero = true);      // freed by rvdd_destroy
int upload(rvdd_t* h, float** dst, const std::vector<float>& v);
int ensure_scratch(rvdd_t* h, size_t bytes);
int ensure_loss_batch(rvdd_t* h, size_t doubles);
uint16_t f16_bits(float x, bool toward_zero);
float f16_value(uint16_t u);
std::vector<std::string> convunet_conv_names(bool feat);
int next_proj_cin(const rvdd_t* h, const std::string& blk);
// ---- net_convunet.hip
int finalize_convunet(rvdd_t* h);
bool seq_major_on(const rvdd_t* h, int n);
bool pre5_fused(const rvdd_t* h);      // EncoderConvs[0][0]'s first source runs as the composed 5x5 conv of the network input
int run_convunet(rvdd_t* h, NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw, float* out_nhwc4,
                 hipStream_t s);
// ---- net_convnext.hip
bool next_pf_pre(const rvdd_t* h);
int finalize_convnext(rvdd_t* h);
int run_convnext(rvdd_t* h, const NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw,
                 float* out_nhwc4, hipStream_t s);
// ---- step.hip
int run_prologue(rvdd_t* h, NetRun& run, Sub sb, hipStream_t s);
// ---- ops.hip
// the checks rvdd_dpc and rvdd_set_dpc share: 0 and *out = the kernel's parameters, or RVDD_ERR_ARG with the field named
int dpc_params(rvdd_t* h, const char* fn, const rvdd_dpc_cfg* cfg, DpcParams* out);
// the checks rvdd_rows_estimate and rvdd_set_rows share: 0 and *out = the kernel's parameters, or RVDD_ERR_ARG with the field named
int rows_params(rvdd_t* h, const char* fn, const rvdd_rows_cfg* cfg, RowsParams* out);
// the checks rvdd_match_raw, rvdd_unmatch_rgb and rvdd_set_match share: 0, or RVDD_ERR_ARG with the field named
int match_params(rvdd_t* h, const char* fn, const rvdd_match_cfg* cfg);
int tvl1flow_batch(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t n, int32_t nx, int32_t ny, int32_t* iterations,
                   void* stream, bool async);
// ---- stages.hip: the state of the stages of rvdd_video_push between its ingest and its output
// do frames of hh x ww cells fit every stage as it is set (0, or the stage's refusal), and is the first-use storage of those that are on there
int stages_fit(rvdd_t* h, int hh, int ww);
// rvdd_set_rows' stage on slots [b, e): estimate and apply, each inside its profile class; `packed` and `gray` point at slot b
int rows_run(rvdd_t* h, float* packed, float* gray, int b, int e, int hh, int ww, int bit_depth, hipStream_t s);
void stages_free(rvdd_t* h);      // rvdd_destroy: the device maps the setters own
// launch_cols_apply inside its profile class, for rvdd_cols_apply and the stage behind rvdd_set_cols: 0, or the HIP error on the handle
int run_cols_apply(rvdd_t* h, float* packed, float* gray, const float* map_dev, int n, int hh, int ww, int bit_depth, hipStream_t s);
// launch_green_apply inside its profile class, for rvdd_green_apply and the stage behind rvdd_set_green: 0, or the HIP error on the handle
int run_green_apply(rvdd_t* h, float* packed, float* gray, const float* map_dev, int gh, int gw, float black, int n, int hh, int ww, int bit_depth,
                    int bayer, hipStream_t s);
