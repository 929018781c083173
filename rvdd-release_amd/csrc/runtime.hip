// librvdd_hip.so -- C ABI (include/rvdd.h), handle, weight repacking, workspace
// and the per-frame schedule of the recurrent denoise+demosaic path
// (models/recurrent_model.py:105-135 set_input, :161-349 forward, test branch).
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

namespace {

thread_local std::string g_create_error;

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
const char* const kCuNames[CU_COUNT] = {
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
const char* const kNxNames[NX_COUNT] = {
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
    float* part = nullptr;
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
    int next_split = 1;       // ConvNeXt, fused blocks: the two 1x1 convs on the F16 matrix pipe with split f32 operands (0: f32 MFMA)
    int next_pipe = 1;        // ConvNeXt, fused split-f16 blocks as a front / back pipeline over tiles (0: convblock_kernel's phases)
    int next_pool = 1;        // ConvNeXt, fused blocks: MaxPool2d(2) from the epilogue of the block in front of a DownConv
    int next_projfuse = 1;    // ConvNeXt, pipelined split-f16 blocks: the 96 -> 48 projection behind a concat as two halves in the
                              // epilogues of the blocks that form the concatenated maps (0: proj1x1_kernel)
    int tvl1_async = 0;       // rvdd_tvl1flow_batch without iteration counts enqueues and returns
    int stream_reset_each = 0;            // every ready step of rvdd_video_push carries the reset mark of every ready slot
    int stream_flow_from_denoised = 0;    // rvdd_video_push: the flow towards the previous frame is matched against the previous output
    int use_graphs = 0;       // replay captured frame-steps (measured slower, off)

    bool split16() const { return conv == CONV_SPLIT16; }
    bool wino_allowed() const { return conv != CONV_DIRECT; }
    bool wino_forced() const { return conv == CONV_WINO; }
};

}  // namespace

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
    double* loss_partial = nullptr;
    double* loss_result = nullptr;
    double* loss_batch = nullptr;    // rvdd_psnr_l1_batch: partial sums and results of every slice, grown on demand
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
        float* dgray = nullptr;      // [B][hh][ww]: gray plane of every slot's last output (option "stream_flow_from_denoised"; allocated by
                                     // the first push that has the option on)
        std::vector<uint8_t> dgray_ok;   // per slot: dgray holds the output of the push before this one
    } st;

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

namespace {

int fail(rvdd_t* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

// One row per option: ABI name | environment variable read at rvdd_create (nullptr: none) | field of Options | accepted range
// lo .. hi | message of a value outside it (nullptr: a flag, any value counts as value != 0) | hook that does the storing itself
// (nullptr: plain store).  F is the first row, X every other: the table and the unknown-option message expand this one list.
int opt_graphs(rvdd_t* h, int32_t value);
int opt_warp_raw(rvdd_t* h, int32_t value);
int opt_tvl1_async(rvdd_t* h, int32_t value);
int opt_block_fp(rvdd_t* h, int32_t value);
int opt_conv_kernel(rvdd_t* h, int32_t value);
#define CONV_KERNEL_RANGE "rvdd_set_option: conv_kernel must be 0 (default), 1 (direct f32), 2 (winograd f32) or 4 (f32 by size)"
#define RVDD_OPTIONS(F, X)                                                                                                       \
    F("no_warp", nullptr, no_warp, 0, 1, nullptr, nullptr)                                                                       \
    X("warp_raw", nullptr, warp_raw, 0, 1, nullptr, opt_warp_raw)                                                                \
    X("prev_noisy_frame", nullptr, prev_noisy, 0, 1, nullptr, nullptr)                                                           \
    X("conv_kernel", "RVDD_CONV", conv, 0, 4, CONV_KERNEL_RANGE, opt_conv_kernel)                                                \
    X("seq_major", "RVDD_SEQ_MAJOR", seq_major, 0, 1, "rvdd_set_option: seq_major must be 0 or 1", nullptr)                      \
    X("graphs", "RVDD_GRAPH", use_graphs, 0, 1, nullptr, opt_graphs)                                                             \
    X("fuse_upsample", "RVDD_FUSE_UPSAMPLE", fuse_upsample, 0, 1, nullptr, nullptr)                                              \
    X("next_split", "RVDD_NEXT_SPLIT", next_split, 0, 1, nullptr, nullptr)                                                       \
    X("next_pipe", "RVDD_NEXT_PIPE", next_pipe, 0, 1, nullptr, nullptr)                                                          \
    X("next_pool", "RVDD_NEXT_POOL", next_pool, 0, 1, nullptr, nullptr)                                                          \
    X("next_projfuse", "RVDD_NEXT_PROJFUSE", next_projfuse, 0, 1, nullptr, nullptr)                                              \
    X("tvl1_async", nullptr, tvl1_async, 0, 1, nullptr, opt_tvl1_async)                                                          \
    X("block_fp", "RVDD_BFP", bfp, 0, 1, nullptr, opt_block_fp)                                                                  \
    X("fuse_pre", "RVDD_FUSE_PRE", fuse_pre, 0, 1, nullptr, nullptr)                                                             \
    X("pre5_cin8", nullptr, pre5_cin8, 0, 1, nullptr, nullptr)                                                                   \
    X("cout_split", "RVDD_COUT_SPLIT", cout_split, 0, 1, nullptr, nullptr)                                                       \
    X("small_prestage", "RVDD_SMALL_PRESTAGE", small_prestage, 0, 1, nullptr, nullptr)                                           \
    X("bayer_pattern", nullptr, bayer, RVDD_BAYER_GBRG, RVDD_BAYER_BGGR,                                                         \
      "rvdd_set_option: bayer_pattern must be 0 (GBRG), 1 (GRBG), 2 (RGGB) or 3 (BGGR)", nullptr)                                \
    X("stream_reset_each", nullptr, stream_reset_each, 0, 1, nullptr, nullptr)                                                   \
    X("stream_flow_from_denoised", nullptr, stream_flow_from_denoised, 0, 1, nullptr, nullptr)
struct OptRow {
    const char* name;
    const char* env;
    int Options::*field;
    int lo, hi;
    const char* range_msg;
    int (*hook)(rvdd_t*, int32_t);
};
#define OPT_ROW(name, env, field, lo, hi, msg, hook) {name, env, &Options::field, lo, hi, msg, hook},
const OptRow kOptions[] = {RVDD_OPTIONS(OPT_ROW, OPT_ROW)};
#define OPT_NAME_FIRST(name, ...) name
#define OPT_NAME(name, ...) ", " name
const char kUnknownOption[] = "rvdd_set_option: unknown option '%s' (known: " RVDD_OPTIONS(OPT_NAME_FIRST, OPT_NAME) ")";

// The one decoder of the conv selector: option "conv_kernel"'s integer (word == nullptr; -1: not a selector), or RVDD_CONV's
// word -- direct | winograd | f32, anything else = the default.
int conv_decode(const char* word, int32_t value) {
    static const struct { int sel; const char* word; } known[] = {
        {CONV_SPLIT16, nullptr}, {CONV_DIRECT, "direct"}, {CONV_WINO, "winograd"}, {CONV_F32, "f32"}};
    for (const auto& k : known)
        if (word ? (k.word && std::strcmp(word, k.word) == 0) : value == k.sel) return k.sel;
    return word ? CONV_SPLIT16 : -1;
}

// range check, then the row's hook or a plain store
int set_option_row(rvdd_t* h, const OptRow& row, int32_t value) {
    if (!row.range_msg) value = value != 0;
    else if (value < row.lo || value > row.hi) return fail(h, RVDD_ERR_ARG, "%s", row.range_msg);
    if (row.hook) return row.hook(h, value);
    h->opt.*row.field = value;
    return RVDD_OK;
}

uint64_t slots_below(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }      // slots [0, n) as a mask (every slot it has, from 64 on)

void drop_graphs(rvdd_t* h) {
    for (auto& kv : h->graphs) {
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    }
    h->graphs.clear();
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

#define RC(expr)               \
    do {                       \
        int rc__ = (expr);     \
        if (rc__) return rc__; \
    } while (0)

int dmalloc(rvdd_t* h, void** p, size_t bytes, bool zero = true) {
    HIPCHK(h, hipMalloc(p, bytes ? bytes : 16));
    h->allocs.push_back(*p);
    if (zero) HIPCHK(h, hipMemset(*p, 0, bytes ? bytes : 16));
    return RVDD_OK;
}

int upload(rvdd_t* h, float** dst, const std::vector<float>& v) {
    int rc = dmalloc(h, reinterpret_cast<void**>(dst), v.size() * sizeof(float), false);
    if (rc) return rc;
    HIPCHK(h, hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    return RVDD_OK;
}

// OIHW [48][cin_total][3][3], channels [c0, c0+cn) -> [tap][j][m][lane = 16g + cout&15][i] with
// channel = c0 + 16j + 4g + i (zero beyond cn): the A-fragment order of conv3x3.hip (lane-linear).
std::vector<float> arrange_conv3x3(const HostTensor& t, int c0, int cn, int cin_pad) {
    const int cin_total = (int)t.shape[1];
    const int NJ = cin_pad / 16;
    std::vector<float> out((size_t)9 * NJ * 48 * 16, 0.f);
    for (int tap = 0; tap < 9; ++tap)
        for (int j = 0; j < NJ; ++j)
            for (int co = 0; co < 48; ++co)
                for (int g = 0; g < 4; ++g)
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * j + 4 * g + i;
                        if (c >= cn) continue;
                        out[(((size_t)(tap * NJ + j) * 3 + co / 16) * 64 + g * 16 + co % 16) * 4 + i] =
                            t.data[(((size_t)co * cin_total + c0 + c) * 3 + tap / 3) * 3 + tap % 3];
                    }
    return out;
}

// OIHW [48][cin_total][3][3], channels [c0, c0+48) -> U = G g G^T per (cout, cin), stored
// [pos 16][j 3][m 3][lane = 16g + (cout&15)][i 4] with channel = c0 + 16j+4g+i: the A-fragment order of wino3x3.hip,
// lane-linear so that each lane group of a ds_read_b128 covers one whole 256-B bank row (no bank conflict).
// nj = 3: input channels c0 .. c0+47 of the filter; nj = 1: the first layer, channels 0 .. cin_total-1 (6 or 9)
// zero-padded to 16
std::vector<float> arrange_wino3x3(const HostTensor& t, int c0, int nj = 3) {
    const int cin_total = (int)t.shape[1];
    const int nc = nj == 3 ? 48 : (cin_total < 16 ? cin_total : 16);
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> out((size_t)16 * nj * 3 * 256, 0.f);
    for (int co = 0; co < 48; ++co)
        for (int c = 0; c < nc; ++c) {
            const float* gk = &t.data[((size_t)co * cin_total + c0 + c) * 9];
            double tmp[4][3], u[4][4];
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 3; ++k) tmp[i][k] = G[i][0] * gk[k] + G[i][1] * gk[3 + k] + G[i][2] * gk[6 + k];
            for (int i = 0; i < 4; ++i)
                for (int k = 0; k < 4; ++k) u[i][k] = tmp[i][0] * G[k][0] + tmp[i][1] * G[k][1] + tmp[i][2] * G[k][2];
            const int j = c / 16, g = (c % 16) / 4, ii = c % 4, m = co / 16, lr = co % 16;
            for (int pos = 0; pos < 16; ++pos)
                out[(((size_t)(pos * nj + j) * 3 + m) * 64 + g * 16 + lr) * 4 + ii] = (float)u[pos / 4][pos % 4];
        }
    return out;
}

// f32 -> f16 bits, toward zero (saturating) or to nearest even; f16 bits -> f32.  Host-side twins of v_cvt_pkrtz_f16_f32 /
// v_cvt_f16_f32 for the split filter banks.
uint16_t f16_bits(float x, bool toward_zero) {
    _Float16 hv = (_Float16)x;                   // to nearest even
    uint16_t u;
    std::memcpy(&u, &hv, 2);
    if (toward_zero) {
        if ((u & 0x7fffu) == 0x7c00u) u = (uint16_t)((u & 0x8000u) | 0x7bffu);      // an overflow saturates
        else if (std::fabs((float)hv) > std::fabs(x)) u = (uint16_t)(u - 1);        // magnitude one step down
    }
    return u;
}
float f16_value(uint16_t u) {
    _Float16 hv;
    std::memcpy(&hv, &u, 2);
    return (float)hv;
}

// OIHW [48][cin_total][3][3], channels [c0, c0+48) -> the split bank of conv3x3h.hip: w' = 2^s w (s = the largest power
// keeping |w'| <= 1024, returned as 2^-s), hi = f16(w') toward zero, lo = f16(w' - hi); stored
// [chunk 14][cout block 3][hi, lo][lane = 16g + (cout & 15)][e 8] as f16 with 8-channel group G = 4 chunk + g = channels
// 8 (G % 6) + e of tap G / 6 (groups 54, 55 zero): lane-linear 16-B A fragments of v_mfma_f32_16x16x32_f16.
// (ks = 5: the composed first layer, [48][cin][5][5], 13 chunks)
std::vector<float> arrange_conv3x3h(const HostTensor& t, int c0, float* inv_scale, int cin_pad = 48, int ks = 3) {
    const int cin_total = (int)t.shape[1];
    const int nc = cin_pad == 48 ? 48 : std::min(cin_total, 16);      // 16: the first layer, 6 or 9 real channels, zero filters beyond
    const int ntap = ks * ks;
    const int gpt = cin_pad / 8, ng = ntap * gpt, nch = (ng + 3) / 4;
    float mx = 0.f;
    for (int co = 0; co < 48; ++co)
        for (int c = 0; c < nc; ++c)
            for (int k = 0; k < ntap; ++k) mx = std::max(mx, std::fabs(t.data[((size_t)co * cin_total + c0 + c) * ntap + k]));
    int sft = 0;
    if (mx > 0.f && std::isfinite(mx)) sft = std::min(40, std::max(-40, (int)std::floor(std::log2(1024.0 / mx))));
    const float sc = std::ldexp(1.0f, sft);
    *inv_scale = std::ldexp(1.0f, -sft);
    const size_t halves = (size_t)nch * 3 * 2 * 512;
    if (halves * 2 != (ks == 5 ? conv5x5h_weight_bytes(cin_pad) : conv3x3h_weight_bytes(cin_pad))) return {};
    std::vector<uint16_t> bank(halves, 0);
    for (int G = 0; G < ng; ++G) {
        const int j = G / 4, g = G % 4, tap = G / gpt, cg = (G % gpt) * 8;
        for (int co = 0; co < 48; ++co)
            for (int e = 0; e < 8; ++e) {
                if (cg + e >= nc) continue;
                const float w = t.data[((size_t)co * cin_total + c0 + cg + e) * ntap + tap] * sc;      // exact: a power of two
                const uint16_t hi = f16_bits(w, true);
                const uint16_t lo = f16_bits(w - f16_value(hi), false);
                const size_t frag = ((size_t)(j * 3 + co / 16) * 2) * 512 + (size_t)(g * 16 + co % 16) * 8 + e;
                bank[frag] = hi;
                bank[frag + 512] = lo;
            }
    }
    std::vector<float> out(halves / 2);
    std::memcpy(out.data(), bank.data(), halves * 2);
    return out;
}


// preprocessing_layer (3x3, cin -> 48, NO activation: networks/unet.py:742) followed by the first 48 input channels of
// EncoderConvs[0][0] (3x3, :743) is one linear map of the network input: out(p) = sum_d W2[d] y(p + d - 1), y(q) = b1 +
// sum_e W1[e] x(q + e - 1)  =>  out(p) = b + sum_u Wc[u] x(p + u - 2), Wc[u] = sum_{d + e = u} W2[d] W1[e] (5x5, 48 x cin),
// b = sum_d W2[d] b1 (+ the layer's own bias, which the pass already adds).  Composed in double.  One 16-channel 5x5 conv
// (K = 400) instead of a 16 -> 48 conv, a full-resolution 48-channel map written and read back, and a 48 -> 48 conv (K = 576).
// The one thing the composition gets wrong is the zero padding BETWEEN the layers: y is ZERO outside the image, the composed
// conv sees b1 + (partial windows) there.  Only pixels on the image border are affected; launch_pre_border_fix subtracts those
// terms (it needs W1, b1, W2 in plain layouts).
int compose_pre_enc0(rvdd_t* h) {
    const HostTensor& w1 = h->staged.at("preprocessing_layer.weight");            // [48 m][cin][3][3]
    const HostTensor& b1 = h->staged.at("preprocessing_layer.bias");
    const HostTensor& w2 = h->staged.at("EncoderConvs.0.blocks.0.0.weight");      // [48 o][96][3][3], channels 0..47 = m
    const int cin = (int)w1.shape[1];
    HostTensor wc;
    wc.shape = {48, cin, 5, 5};
    std::vector<double> acc((size_t)48 * cin * 25, 0.0);
    for (int o = 0; o < 48; ++o)
        for (int m = 0; m < 48; ++m)
            for (int d = 0; d < 9; ++d) {
                const double a = w2.data[((size_t)o * 96 + m) * 9 + d];
                if (a == 0.0) continue;
                const int dy = d / 3, dx = d % 3;
                for (int c = 0; c < cin; ++c)
                    for (int e = 0; e < 9; ++e)
                        acc[((size_t)o * cin + c) * 25 + (dy + e / 3) * 5 + dx + e % 3] += a * (double)w1.data[((size_t)m * cin + c) * 9 + e];
            }
    wc.data.resize(acc.size());
    for (size_t i = 0; i < acc.size(); ++i) wc.data[i] = (float)acc[i];
    std::vector<float> bc(48);
    for (int o = 0; o < 48; ++o) {
        double b = 0.0;
        for (int m = 0; m < 48; ++m)
            for (int d = 0; d < 9; ++d) b += (double)w2.data[((size_t)o * 96 + m) * 9 + d] * (double)b1.data[m];
        bc[o] = (float)(b + (double)h->staged.at("EncoderConvs.0.blocks.0.0.bias").data[o]);      // + the layer's own bias (pass 1 adds it)
    }
    RC(upload(h, &h->pre5_w, arrange_conv3x3h(wc, 0, &h->pre5_inv, 16, 5)));
    // without a future frame (6 real channels) the second 8-channel group of every tap is zero filters on zero input: the bank of
    // the first groups alone, 25 groups in 7 chunks.  Both banks are kept, "pre5_cin8" chooses per launch.
    h->pre5_w8 = nullptr;
    if (h->cin_real() <= 8) RC(upload(h, &h->pre5_w8, arrange_conv3x3h(wc, 0, &h->pre5_inv8, 8, 5)));
    RC(upload(h, &h->pre5_b, bc));
    std::vector<float> a1((size_t)9 * 16 * 48, 0.f), a2((size_t)9 * 48 * 48);
    for (int e = 0; e < 9; ++e)
        for (int c = 0; c < cin; ++c)
            for (int m = 0; m < 48; ++m) a1[((size_t)e * 16 + c) * 48 + m] = w1.data[((size_t)m * cin + c) * 9 + e];
    for (int d = 0; d < 9; ++d)
        for (int m = 0; m < 48; ++m)
            for (int o = 0; o < 48; ++o) a2[((size_t)d * 48 + m) * 48 + o] = w2.data[((size_t)o * 96 + m) * 9 + d];
    RC(upload(h, &h->pre_w1, a1));
    RC(upload(h, &h->pre_b1, b1.data));
    RC(upload(h, &h->pre_w2, a2));
    return RVDD_OK;
}

// ---- expected state_dict -------------------
struct KeySpec {
    std::string key;
    std::vector<int64_t> shape;
};

std::vector<std::string> convunet_conv_names(bool feat) {
    std::vector<std::string> n;
    for (int i = feat ? 0 : 1; i < CU_COUNT; ++i) n.push_back(kCuNames[i]);
    return n;
}

int convunet_cin(const rvdd_t* h, const std::string& name) {
    const bool feat = h->has_feat();
    if (name == "preprocessing_layer") return h->cin_real();
    if (name == "EncoderConvs.0.blocks.0.0") return feat ? 96 : h->cin_real();
    if (name.rfind("DecoderConvs.", 0) == 0 && name.find(".blocks.0.0") != std::string::npos) return 96;
    return 48;
}

std::vector<std::string> next_block_names(bool feat) {
    std::vector<std::string> n;
    for (int i = feat ? 0 : 1; i < NX_COUNT; ++i) n.push_back(kNxNames[i]);
    return n;
}

int next_proj_cin(const rvdd_t* h, const std::string& blk) {
    const bool feat = h->has_feat();
    if (blk == "preprocessing_layer.blocks.0") return h->cin_real();
    if (blk == "encoder_convs.0.blocks.0") return feat ? 96 : h->cin_real();
    if (blk.rfind("decoder_convs.", 0) == 0 && blk.find(".blocks.0") != std::string::npos) return 96;
    return 0;
}

std::vector<KeySpec> expected_keys(const rvdd_t* h) {
    std::vector<KeySpec> k;
    if (!h->is_next()) {
        for (const auto& n : convunet_conv_names(h->has_feat())) {
            k.push_back({n + ".weight", {48, convunet_cin(h, n), 3, 3}});
            k.push_back({n + ".bias", {48}});
        }
        k.push_back({"PostConvs.1.weight", {3, 48, 1, 1}});
        k.push_back({"PostConvs.1.bias", {3}});
    } else {
        for (const auto& b : next_block_names(h->has_feat())) {
            const int pc = next_proj_cin(h, b);
            if (pc) {
                k.push_back({b + ".proj.weight", {48, pc, 1, 1}});
                k.push_back({b + ".proj.bias", {48}});
            }
            k.push_back({b + ".block.0.weight", {48, 1, 7, 7}});
            k.push_back({b + ".block.0.bias", {48}});
            k.push_back({b + ".block.1.weight", {48}});
            k.push_back({b + ".block.1.bias", {48}});
            k.push_back({b + ".block.2.weight", {192, 48, 1, 1}});
            k.push_back({b + ".block.2.bias", {192}});
            k.push_back({b + ".block.4.weight", {48, 192, 1, 1}});
            k.push_back({b + ".block.4.bias", {48}});
            k.push_back({b + ".layerscale.layerscale", {48}});
        }
        k.push_back({"postprocessing.1.weight", {3, 48, 1, 1}});
        k.push_back({"postprocessing.1.bias", {3}});
    }
    return k;
}

// ---- measurement -------------------------------------------------------------
int prof_class(rvdd_t* h, const char* name) {
    for (size_t i = 0; i < h->prof.size(); ++i)
        if (h->prof[i].name == name) return (int)i;
    h->prof.push_back(ProfClass{name});
    return (int)h->prof.size() - 1;
}

hipEvent_t get_event(rvdd_t* h) {
    if (!h->event_pool.empty()) {
        hipEvent_t e = h->event_pool.back();
        h->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

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

int prof_flush(rvdd_t* h) {
    for (auto& p : h->pending) {
        HIPCHK(h, hipEventSynchronize(p.e1));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, p.e0, p.e1));
        h->prof[p.cls].ms += ms;
        h->event_pool.push_back(p.e0);
        h->event_pool.push_back(p.e1);
    }
    h->pending.clear();
    return RVDD_OK;
}

// ---- conv helper ---------------------------------------------------------------
const char* conv_name(int cin, int epi, bool acc) {
    static const char* names[2][4][2] = {
        {{"conv3x3_kernel<16, 0, false>", "conv3x3_kernel<16, 0, true>"},
         {"conv3x3_kernel<16, 1, false>", "conv3x3_kernel<16, 1, true>"},
         {"conv3x3_kernel<16, 2, false>", "conv3x3_kernel<16, 2, true>"},
         {"conv3x3_kernel<16, 3, false>", "conv3x3_kernel<16, 3, true>"}},
        {{"conv3x3_kernel<48, 0, false>", "conv3x3_kernel<48, 0, true>"},
         {"conv3x3_kernel<48, 1, false>", "conv3x3_kernel<48, 1, true>"},
         {"conv3x3_kernel<48, 2, false>", "conv3x3_kernel<48, 2, true>"},
         {"conv3x3_kernel<48, 3, false>", "conv3x3_kernel<48, 3, true>"}}};
    return names[cin == 48][epi][acc];
}

const char* wino_name(int epi, bool acc) {
    static const char* names[5][2] = {{"wino3x3_kernel<0, false>", "wino3x3_kernel<0, true>"},
                                      {"wino3x3_kernel<1, false>", "wino3x3_kernel<1, true>"},
                                      {"wino3x3_kernel<2, false>", "wino3x3_kernel<2, true>"},
                                      {"wino3x3_kernel<3, false>", "wino3x3_kernel<3, true>"},
                                      {"wino3x3_kernel<4, false>", "wino3x3_kernel<4, true>"}};
    return names[epi][acc];
}

const char* conv_name_h(int epi, bool acc) {
    static const char* names[5][2] = {{"conv3x3h_kernel<48, 0, false, false>", "conv3x3h_kernel<48, 0, true, false>"},
                                      {"conv3x3h_kernel<48, 1, false, false>", "conv3x3h_kernel<48, 1, true, false>"},
                                      {"conv3x3h_kernel<48, 2, false, false>", "conv3x3h_kernel<48, 2, true, false>"},
                                      {"conv3x3h_kernel<48, 3, false, false>", "conv3x3h_kernel<48, 3, true, false>"},
                                      {"conv3x3h_kernel<48, 4, false, false>", "conv3x3h_kernel<48, 4, true, false>"}};
    return names[epi][acc];
}


// the amax words (rvdd_internal.h) of map `slot`, from sequence b0 on
unsigned* amax_words(const rvdd_t* h, int slot, size_t b0 = 0) { return h->amax + ((size_t)slot * h->cfg.batch + b0) * kAmaxSeqWords; }
constexpr size_t amax_bytes(int B, int nslots) { return (size_t)nslots * B * kAmaxSeqWords * sizeof(unsigned); }

// The amax slots of one forward: the first slot of its regular set, and the absolute slots it reads the old features' words
// from / writes the new ones to.  A frame-step's follow step_ctr; rvdd_unet_forward has a set of its own, so that the
// frame-steps' sets and the recurrent slots stay untouched.
struct AmaxSlots {
    int base = 0, feat_in = 0, post_out = 0;
};
constexpr AmaxSlots step_amax(int ctr) { return {(ctr & 1) * AMAX_NREG, AMAX_FEAT0 + (ctr + 2) % 3, AMAX_FEAT0 + ctr % 3}; }
constexpr AmaxSlots forward_amax() { return {2 * AMAX_NREG, 2 * AMAX_NREG + AMAX_REL_FWDFEAT, 2 * AMAX_NREG + CU_POST}; }

// One forward of the net, handed down to everything that launches for it: a frame-step (enqueue_step) or a bare
// rvdd_unet_forward.
struct StepInputs;
struct NetRun {
    int n = 0;                        // the sequences it covers: slots [0, n) of the handle's maps
    AmaxSlots amax;
    bool zero_pending = false;        // the first network-input launch zeroes the set and features slot of the step after (run_prologue)
    bool netin_proj = false;          // lv[0].t[0] already holds the first ConvBlock's projection of the network input (run_prologue)
    bool featw_proj = false;          // `featw` holds W_f warp(features) + bias (run_prologue, next_pf_pre), not the warped features
    const StepInputs* in = nullptr;   // what a frame-step does in front of the net (run_prologue); null for rvdd_unet_forward
};
int amax_layer(const NetRun& run, int layer) { return run.amax.base + layer; }

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

// Winograd needs enough 8x32-pixel units to fill the chip (its 144 KiB filter bank is loaded once
// per workgroup); the 1/8-resolution level of a single 720p sequence (60 units) runs faster direct
bool wino_applies(const rvdd_t* h, const NetRun& run, int H, int W) {
    return h->opt.wino_allowed() && (h->opt.wino_forced() || run.n * ((W + 31) / 32) * ((H + 7) / 8) >= 200);
}

// Sequences [b0, b0 + nb) of the batch: the maps of a ConvCall are those of the WHOLE batch, a launch may cover a part.
struct Sub {
    int b0, nb;
};

// Full-resolution stages one sequence at a time (depth first) instead of all B sequences per layer -- an option
// (rvdd_set_option "seq_major"), off by default.  The idea: a 48-channel map of ONE 720p sequence (177 MB) stays in
// the 256 MiB Infinity Cache between the layer that writes it and the layer that reads it, the maps of four (708 MB)
// do not.  Measured (profiles/r02_c_seq_major.json): 424 frames/s against 456 batched -- per-sequence launches lose
// more to their tails (3600 units on 256 CUs = 14.06 rounds) and to four filter-bank loads per layer than the cache
// gives back.  Kept because it is free and pins an invariant the tests use: a launch's batch size does not enter a
// tile's sums, so both schedules give bit-identical frames.
bool seq_major_on(const rvdd_t* h, int n) { return n > 1 && h->opt.seq_major == 1; }

int run_conv(rvdd_t* h, const NetRun& run, const Conv3& L, const ConvCall& c, hipStream_t s, Sub sub) {
    const int cin = L.cin_pad[c.src];
    const int Ho = c.epi == EPI_POOL ? c.H / 2 : (c.Hout ? c.Hout : c.H), Wo = c.epi == EPI_POOL ? c.W / 2 : (c.Wout ? c.Wout : c.W);
    const size_t px_in = (size_t)sub.b0 * c.H * c.W, px_out = (size_t)sub.b0 * Ho * Wo;
    ConvArgs a{};
    a.in = c.in + (c.ups ? px_in / 4 : px_in) * cin;
    a.ups = c.ups ? 1 : 0;
    a.w = L.w[c.src];
    a.bias = L.bias;
    a.acc_in = c.acc_in ? c.acc_in + px_in * kF : nullptr;
    a.res1 = c.res1 ? c.res1 + px_in * kF : nullptr;
    a.res2 = c.res2 ? c.res2 + px_in * kF : nullptr;
    a.out = c.out + px_out * kF;
    a.B = sub.nb;
    a.H = c.H;
    a.W = c.W;
    a.Hout = Ho;
    a.Wout = Wo;
    a.oy = c.oy;
    a.ox = c.ox;
    a.tiles_x = (c.W + 15) / 16;
    a.tiles_y = (c.H + 7) / 8;
    a.ntiles = a.B * a.tiles_x * a.tiles_y;
    const double px = (double)a.B * c.H * c.W;
    const double flops = 2.0 * 9.0 * L.cin_real[c.src] * 48.0 * px;
    double bytes = px * 4.0 * (L.cin_real[c.src] + (c.epi == EPI_POOL ? 12.0 : 48.0));
    if (c.acc_in) bytes += px * 192.0;
    if (c.epi == EPI_RELU_ADD2) bytes += px * 384.0;
    a.w3 = h->w_out;
    a.b3 = h->b_out;
    a.out3_nchw = c.out3_nchw ? c.out3_nchw + px_in * 3 : nullptr;
    a.out3_nhwc4 = c.out3_nhwc4 ? c.out3_nhwc4 + px_in * 4 : nullptr;
    a.amax_in = (c.amax_in >= 0 && h->opt.bfp) ? amax_words(h, c.amax_in, sub.b0) : nullptr;
    a.amax_out = (c.amax_out >= 0 && h->opt.bfp) ? amax_words(h, c.amax_out, sub.b0) : nullptr;
    const bool c16_ok = cin != 48 && !c.acc_in && (c.epi == EPI_NONE || c.epi == EPI_RELU);
    if (c.ups && !(cin == 48 && ((h->opt.split16() && L.wh[c.src]) || (L.wu[c.src] && wino_applies(h, run, c.H, c.W)))))
        return fail(h, RVDD_ERR_STATE, "run_conv: the fused upsample exists in the split-f16 and the Winograd kernels only");
    if (c.ups) bytes -= px * 4.0 * 36.0;          // reads the quarter-size map
    // the F16 matrix pipe with split operands: every layer of the convunet
    if (h->opt.split16() && L.wh[c.src] && (cin == 48 || c16_ok)) {
        a.w = L.wh[c.src];
        a.wscale = L.wh_inv[c.src];
        Scope sc(h, s, c.ups ? "conv3x3h_kernel<48, 1, false, true>" : cin == 48 ? conv_name_h(c.epi, c.acc_in != nullptr)
                           : (c.epi == EPI_NONE ? "conv3x3h_kernel<16, 0, false, false>" : "conv3x3h_kernel<16, 1, false, false>"), flops, bytes);
        HIPCHK(h, launch_conv3x3h(a, cin == 48 ? 48 : 16, c.epi, s, h->opt.cout_split));
        return RVDD_OK;
    }
    if ((cin == 48 || c16_ok) && L.wu[c.src] && wino_applies(h, run, c.H, c.W)) {
        a.w = L.wu[c.src];
        Scope sc(h, s, c.ups ? "wino3x3_ups_kernel<1>" : cin == 48 ? wino_name(c.epi, c.acc_in != nullptr)
                                 : (c.epi == EPI_NONE ? "wino3x3_c16_kernel<0>" : "wino3x3_c16_kernel<1>"), flops, bytes);
        HIPCHK(h, launch_wino3x3(a, cin == 48 ? 48 : 16, c.epi, s));
        return RVDD_OK;
    }
    Scope sc(h, s, conv_name(cin, c.epi, c.acc_in != nullptr), flops, bytes);
    HIPCHK(h, launch_conv3x3(a, cin, c.epi, s, c.variant));
    return RVDD_OK;
}


// The composed 5x5 conv of the network input (compose_pre_enc0) into `part`, and its border fix; sequences of `sub`.
int run_pre5(rvdd_t* h, const NetRun& run, const float* netin, float* part, hipStream_t s, Sub sub) {
    const int H = h->cfg.height, W = h->cfg.width;
    const size_t px0 = (size_t)sub.b0 * H * W;
    ConvArgs a{};
    a.in = netin + px0 * kNetInC;
    const bool c8 = h->opt.pre5_cin8 && h->pre5_w8;      // at most 8 real channels: only the first 8 of the 16-channel pixel are multiplied
    a.w = c8 ? h->pre5_w8 : h->pre5_w;
    a.wscale = c8 ? h->pre5_inv8 : h->pre5_inv;
    a.bias = h->pre5_b;
    a.out = part + px0 * kF;
    a.B = sub.nb;
    a.H = a.Hout = H;
    a.W = a.Wout = W;
    a.amax_in = h->opt.bfp ? amax_words(h, run.amax.base + AMAX_REL_NETIN, sub.b0) : nullptr;
    const double px = (double)sub.nb * H * W;
    {
        Scope sc(h, s, c8 ? "conv5x5h_kernel<8>" : "conv5x5h_kernel<16>", 2.0 * 25.0 * h->cin_real() * 48.0 * px, px * 4.0 * (h->cin_real() + 48.0));
        HIPCHK(h, c8 ? launch_conv5x5h_c8(a, s) : launch_conv5x5h_c16(a, s));
    }
    HIPCHK(h, launch_pre_border_fix(a.in, h->pre_w1, h->pre_b1, h->pre_w2, a.out, sub.nb, H, W, s));
    return RVDD_OK;
}

// What rvdd_step does in front of the net (demosaic, warps): the caller's frame and flow pointers of one step.
// run_convunet calls it per sequence when the full-resolution stages run depth first.
struct StepInputs {
    const float* raw_prev = nullptr;      // only on the first step of a video (of any sequence)
    unsigned long long latch = 0;         // the sequences that start a video on this step: ~0 = all, else bit b (B <= 64)
    const float* raw_cur = nullptr;
    const float* raw_next = nullptr;
    const float* flow_prev = nullptr;
    const float* flow_next = nullptr;
    size_t rawf = 0, flowf = 0;       // floats from one sequence to the next in the caller's raw / flow tensors
};
int run_prologue(rvdd_t* h, NetRun& run, Sub sb, hipStream_t s);

// networks/unet.py:544-588 as specialised by UNet_FixedFeatures[_feat] (:595-825).
int run_convunet(rvdd_t* h, NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw,
                 float* out_nhwc4, hipStream_t s) {
    const bool feat = h->has_feat();
    const int B = run.n;
    Level* lv = h->lv;
    const Conv3* cu = h->cu;
    // `from` = the amax slot of the input map (L(the layer that wrote it), AMAX_NETIN, run.amax.feat_in); a layer's output slot is L(its id)
    auto conv = [&](int layer, const float* in, int from, float* out, int lvl, int epi, Sub sub) {
        ConvCall c;
        c.in = in; c.out = out; c.H = lv[lvl].H; c.W = lv[lvl].W; c.epi = epi;
        c.amax_in = from; c.amax_out = amax_layer(run, layer);
        return run_conv(h, run, cu[layer], c, s, sub);
    };
    const auto L = [&](int layer) { return amax_layer(run, layer); };
    const int AMAX_NETIN = run.amax.base + AMAX_REL_NETIN;
    // two-source (virtual concat) conv: pass 1 leaves bias + sum over source A in `part`
    auto conv2 = [&](int layer, const float* inA, int fromA, const float* inB, int fromB, float* out, int lvl, Sub sub) {
        ConvCall c;
        c.in = inA; c.src = 0; c.out = lv[lvl].part; c.H = lv[lvl].H; c.W = lv[lvl].W; c.epi = EPI_NONE;
        c.amax_in = fromA;
        RC(run_conv(h, run, cu[layer], c, s, sub));
        c.in = inB; c.src = 1; c.acc_in = lv[lvl].part; c.out = out; c.epi = EPI_RELU;
        c.amax_in = fromB; c.amax_out = amax_layer(run, layer);
        return run_conv(h, run, cu[layer], c, s, sub);
    };
    const Sub all{0, B};
    // the full-resolution stages run per sequence when that keeps their maps in the Infinity Cache (seq_major_on),
    // in an order that alternates from frame to frame so that a step begins with the sequence the last one ended on
    const bool per_seq = seq_major_on(h, B);
    const int nsub = per_seq ? B : 1;
    auto sub_at = [&](int k) { return per_seq ? Sub{h->serpentine ? B - 1 - k : k, 1} : all; };

    // ---- pre-stages + encoder level 0
    for (int k = 0; k < nsub; ++k) {
        const Sub sb = sub_at(k);
        if (run.in) RC(run_prologue(h, run, sb, s));
        if (feat && h->opt.fuse_pre && h->opt.split16() && h->pre5_w) {
            // preprocessing_layer (:742, no activation) and the first source of EncoderConvs[0][0] (:743) as ONE 5x5 conv of the
            // network input (compose_pre_enc0), its border ring put right, then the second source (the old features) as before
            RC(run_pre5(h, run, netin, lv[0].part, s, sb));
            ConvCall c;
            c.in = featw; c.src = 1; c.acc_in = lv[0].part; c.out = lv[0].t[1]; c.H = lv[0].H; c.W = lv[0].W; c.epi = EPI_RELU;
            c.amax_in = run.amax.feat_in; c.amax_out = L(CU_ENC0_0);
            RC(run_conv(h, run, cu[CU_ENC0_0], c, s, sb));
        } else if (feat) {
            RC(conv(CU_PRE, netin, AMAX_NETIN, lv[0].t[0], 0, EPI_NONE, sb));               // :742 (no activation)
            RC(conv2(CU_ENC0_0, lv[0].t[0], L(CU_PRE), featw, run.amax.feat_in, lv[0].t[1], 0, sb)); // cat[y, old_features] :743
        } else {
            RC(conv(CU_ENC0_0, netin, AMAX_NETIN, lv[0].t[1], 0, EPI_RELU, sb));
        }
        RC(conv(CU_ENC0_1, lv[0].t[1], L(CU_ENC0_0), lv[0].skip, 0, EPI_RELU, sb));
        RC(conv(CU_DOWN0, lv[0].skip, L(CU_ENC0_1), lv[1].t[0], 0, EPI_POOL, sb));          // :207-208
    }
    // ---- encoder levels 1..3 (all sequences per launch: these levels need the batch to fill the chip)
    for (int i = 1; i <= 3; ++i) {
        if (i > 1) RC(conv(cu_down(i - 1), lv[i - 1].skip, L(cu_enc(i - 1, 1)), lv[i].t[0], i - 1, EPI_POOL, all));
        RC(conv(cu_enc(i, 0), lv[i].t[0], L(cu_down(i - 1)), lv[i].t[1], i, EPI_RELU, all));
        RC(conv(cu_enc(i, 1), lv[i].t[1], L(cu_enc(i, 0)), i < 3 ? lv[i].skip : lv[3].t[2], i, EPI_RELU, all));
    }
    // ---- bottleneck: d = e3 + d1 + d2 (:561-567)
    float* e3 = lv[3].t[2];
    RC(conv(CU_BOT0, e3, L(cu_enc(3, 1)), lv[3].t[0], 3, EPI_RELU, all));
    {
        ConvCall c;
        c.in = lv[3].t[0]; c.out = lv[3].t[1]; c.H = lv[3].H; c.W = lv[3].W;
        c.epi = EPI_RELU_ADD2; c.res1 = e3; c.res2 = lv[3].t[0];
        c.amax_in = L(CU_BOT0); c.amax_out = L(CU_BOT1);
        RC(run_conv(h, run, cu[CU_BOT1], c, s, all));
    }
    const float* d = lv[3].t[1];
    int d_from = L(CU_BOT1);
    // ---- decoder (:570-579); its last level again per sequence, together with the post convs
    float* fdst = feat_dst ? feat_dst : lv[0].t[2];
    for (int i = 0; i < 3; ++i) {
        const int lo = 3 - i, hi = 2 - i;
        const int uh = 2 * lv[lo].H, uw = 2 * lv[lo].W;      // size after nn.Upsample(x2)
        for (int k = 0; k < (hi == 0 ? nsub : 1); ++k) {
            const Sub sb = hi == 0 ? sub_at(k) : all;
            const size_t lo_px = (size_t)sb.b0 * lv[lo].H * lv[lo].W, hi_px = (size_t)sb.b0 * lv[hi].H * lv[hi].W;
            // UpConv: bilinear x2, conv, ReLU (:137-142).  Where the Winograd kernel runs the conv, the interpolation
            // happens in its patch load and the upsampled map is never written; elsewhere it is made first.
            const bool fused = h->opt.fuse_upsample && (h->opt.split16() || wino_applies(h, run, uh, uw));
            if (!fused) {
                Scope sc(h, s, "upsample2x_kernel", 0.0, (double)sb.nb * uh * uw * 192.0 * 1.25);
                HIPCHK(h, launch_upsample2x(d + lo_px * kF, lv[hi].t[0] + (size_t)sb.b0 * uh * uw * kF, sb.nb, lv[lo].H, lv[lo].W, uh,
                                            uw, 0, 0, false, s));
            }
            // conv + ReLU at the upsampled size, written into a map of the skip's size
            // (zero_pad_features, :151-170; identity when sizes agree)
            ConvCall c;
            c.in = fused ? d : lv[hi].t[0]; c.ups = fused;
            c.out = lv[hi].t[1]; c.H = uh; c.W = uw; c.epi = EPI_RELU;
            c.Hout = lv[hi].H; c.Wout = lv[hi].W;
            c.oy = (lv[hi].H - uh) / 2; c.ox = (lv[hi].W - uw) / 2;
            // (an interpolated value never exceeds the map's maximum: the upsampled map shares the words of its source)
            c.amax_in = d_from; c.amax_out = L(cu_up(i));
            if (uh != lv[hi].H || uw != lv[hi].W)
                HIPCHK(h, hipMemsetAsync(lv[hi].t[1] + hi_px * kF, 0, (size_t)sb.nb * lv[hi].H * lv[hi].W * kF * sizeof(float), s));
            RC(run_conv(h, run, cu[cu_up(i)], c, s, sb));
            RC(conv2(cu_dec(i, 0), lv[hi].skip, L(cu_enc(hi, 1)), lv[hi].t[1], L(cu_up(i)), lv[hi].t[0], hi, sb));        // cat(skip, dec) :541
            RC(conv(cu_dec(i, 1), lv[hi].t[0], L(cu_dec(i, 0)), lv[hi].t[1], hi, EPI_RELU, sb));
            if (hi > 0) continue;
            // ---- post: hooked 48-ch map = next frame's features (:808-812), then 1x1 -> 3
            if (h->opt.split16() || wino_applies(h, run, lv[0].H, lv[0].W)) {
                // PostConvs[1] (1x1, 48 -> 3) rides in the epilogue of PostConvs[0]'s kernel (split-f16: at every size; Winograd
                // f32: where it runs) -- and with it the output frame's share of the words the next step's input bound reads
                ConvCall pc;
                pc.in = lv[0].t[1]; pc.out = fdst; pc.H = lv[0].H; pc.W = lv[0].W; pc.epi = EPI_RELU_OUT3;
                pc.out3_nchw = out_nchw; pc.out3_nhwc4 = out_nhwc4;
                pc.amax_in = L(cu_dec(2, 1)); pc.amax_out = run.amax.post_out;
                RC(run_conv(h, run, cu[CU_POST], pc, s, sb));
            } else {
                ConvCall pc;
                pc.in = lv[0].t[1]; pc.out = fdst; pc.H = lv[0].H; pc.W = lv[0].W; pc.epi = EPI_RELU;
                pc.amax_in = L(cu_dec(2, 1)); pc.amax_out = run.amax.post_out;
                RC(run_conv(h, run, cu[CU_POST], pc, s, sb));
                const size_t px0 = (size_t)sb.b0 * h->cfg.height * h->cfg.width;
                const double px = (double)sb.nb * h->cfg.height * h->cfg.width;
                Scope sc(h, s, "conv1x1_out_kernel", 2.0 * 48 * 3 * px, px * (192.0 + 12.0 + 16.0));
                HIPCHK(h, launch_conv1x1_out(fdst + px0 * kF, h->w_out, h->b_out, out_nchw + px0 * 3,
                                             out_nhwc4 ? out_nhwc4 + px0 * 4 : nullptr, sb.nb, h->cfg.height, h->cfg.width, s));
            }
        }
        d = lv[hi].t[1];
        d_from = L(cu_dec(i, 1));
    }
    return RVDD_OK;
}

int ensure_scratch(rvdd_t* h, size_t bytes) {
    if (h->scratch_bytes >= bytes) return RVDD_OK;
    if (h->scratch) {
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, hipFree(h->scratch));
        h->scratch = nullptr;
        h->scratch_bytes = 0;
    }
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->scratch), bytes));
    h->scratch_bytes = bytes;
    return RVDD_OK;
}

}  // namespace

#include "runtime_next.inc"

namespace {
int run_net(rvdd_t* h, NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw,
            float* out_nhwc4, hipStream_t s) {
    if (!h->is_next()) return run_convunet(h, run, netin, featw, feat_dst, out_nchw, out_nhwc4, s);
    if (run.in) RC(run_prologue(h, run, Sub{0, run.n}, s));
    return run_convnext(h, run, netin, featw, feat_dst, out_nchw, out_nhwc4, s);
}
}  // namespace

// =============================================================== C ABI =====
extern "C" {

const char* rvdd_version(void) { return "rvdd-hip 0.1 (gfx950)"; }

const char* rvdd_last_error(const rvdd_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

namespace {
bool graph_stream(rvdd_t* h) {
    if (h->gstream) return true;
    if (hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->g_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->g_out, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (h->gstream) (void)hipStreamDestroy(h->gstream);
        h->gstream = nullptr;
        return false;
    }
    return true;
}

// ---- the options that do more than store a value (kOptions)
int opt_graphs(rvdd_t* h, int32_t value) {        // the capture stream on demand (see rvdd_create)
    h->opt.use_graphs = value && graph_stream(h);
    return RVDD_OK;
}
int opt_warp_raw(rvdd_t* h, int32_t value) {
    // the reference warps the full-resolution features with the raw-resolution flow in this mode and fails on the shapes
    if (value && h->has_feat()) return fail(h, RVDD_ERR_ARG, "rvdd_set_option: warp_raw is not defined with feature recurrence (the reference fails there too)");
    h->opt.warp_raw = value;
    return RVDD_OK;
}
int opt_tvl1_async(rvdd_t* h, int32_t value) {    // 0 switches back and reports what is pending now (the control word, see rvdd.h)
    if (!value && h->tvl1) {
        ENTER(h);
        HIPCHK(h, hipDeviceSynchronize());
        if (hipError_t e = tvl1_check(h->tvl1, nullptr); e != hipSuccess)
            return fail(h, RVDD_ERR_HIP, "rvdd_set_option(tvl1_async, 0): a pending asynchronous flow batch failed: %s", hipGetErrorString(e));
    }
    h->opt.tvl1_async = value;
    return RVDD_OK;
}
int opt_block_fp(rvdd_t* h, int32_t value) {
    h->opt.bfp = value;
    if (h->amax) {
        ENTER(h);
        HIPCHK(h, hipMemset(h->amax, 0, amax_bytes(h->cfg.batch, AMAX_SLOTS)));      // no stale words across the switch
    }
    return RVDD_OK;
}
int opt_conv_kernel(rvdd_t* h, int32_t value) {
    const int sel = conv_decode(nullptr, value);
    if (sel < 0) return fail(h, RVDD_ERR_ARG, "%s", CONV_KERNEL_RANGE);
    h->opt.conv = sel;
    return RVDD_OK;
}
}  // namespace

int rvdd_create(const rvdd_cfg* cfg, rvdd_t** out) {
    if (!cfg || !out) return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: null argument");
    *out = nullptr;
    if (cfg->arch < 0 || cfg->arch > 3) return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: unknown arch %d", cfg->arch);
    if (cfg->future < 0 || cfg->future > 1) return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: future must be 0 or 1");
    if (cfg->batch < 1) return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: batch must be >= 1");
    if (cfg->height < 16 || cfg->width < 16 || (cfg->height & 1) || (cfg->width & 1))
        return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: frame size %dx%d must be even and >= 16", cfg->height, cfg->width);
    // byte offsets inside one 48-channel map are 32-bit in every kernel (buffer addressing): the map must stay below 2 GiB
    if ((size_t)cfg->height * cfg->width * kF * sizeof(float) >= 0x80000000ull)
        return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: frame %dx%d too large: one 48-channel map must stay below 2 GiB (11.1 Mpx)",
                    cfg->height, cfg->width);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, RVDD_ERR_HIP, "rvdd_create: no HIP device available (%s); this runtime has no CPU fallback",
                    hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(nullptr, RVDD_ERR_ARG, "rvdd_create: device %d out of range (0..%d)", cfg->device, ndev - 1);
    DeviceGuard guard(cfg->device);
    if (guard.err != hipSuccess) return fail(nullptr, RVDD_ERR_HIP, "cannot select device %d: %s", cfg->device, hipGetErrorString(guard.err));

    rvdd_t* h = new rvdd_handle();
    h->cfg = *cfg;
    h->reset_marks = slots_below(cfg->batch);
    const int B = cfg->batch, H = cfg->height, W = cfg->width;
    int rc = RVDD_OK;
    auto A = [&](float** p, size_t floats) {
        if (rc == RVDD_OK) rc = dmalloc(h, reinterpret_cast<void**>(p), floats * sizeof(float));
    };
    int lh = H, lw = W;
    for (int l = 0; l < 4; ++l) {
        h->lv[l].H = lh;
        h->lv[l].W = lw;
        const size_t n = (size_t)B * lh * lw * kF;
        for (int k = 0; k < 3; ++k) A(&h->lv[l].t[k], n);
        A(&h->lv[l].skip, n);
        A(&h->lv[l].part, n);
        lh /= 2;
        lw /= 2;
    }
    const size_t npix = (size_t)B * H * W;
    A(&h->netin, npix * kNetInC);
    A(&h->lastden4, npix * 4);
    A(&h->next4, npix * 4);
    A(&h->green, npix);
    if (h->has_feat()) {
        A(&h->featw, npix * kF);
        A(&h->lastfeat, npix * kF);
    }
    if (rc == RVDD_OK) rc = dmalloc(h, reinterpret_cast<void**>(&h->amax), amax_bytes(B, AMAX_SLOTS));
    if (rc == RVDD_OK) rc = dmalloc(h, reinterpret_cast<void**>(&h->loss_partial), 2 * 1024 * sizeof(double));
    if (rc == RVDD_OK) rc = dmalloc(h, reinterpret_cast<void**>(&h->loss_result), 2 * sizeof(double));
    if (rc != RVDD_OK) {
        g_create_error = h->err;
        rvdd_destroy(h);
        return rc;
    }
    (void)hipEventCreate(&h->t0);
    (void)hipEventCreate(&h->t1);
    // The capture stream (option graphs) is created when the option first asks for it, not here: every stream a process holds is a
    // hardware queue the device's scheduler keeps mapped, and a handle that merely EXISTED beside another one -- with the two idle
    // streams every handle used to create -- made that one's cooperative TV-L1 launches and the kernels behind them 20 % slower
    // (profiles/r05k_online_flow_two_handles.txt)
    // The measurement switches of the environment: a number (0 = off), RVDD_CONV a word.  They go the way of rvdd_set_option, hooks
    // included: RVDD_GRAPH makes the capture stream, RVDD_BFP clears the amax words once more, RVDD_CONV's word comes back from
    // conv_decode as a selector that opt_conv_kernel accepts.  Last in create, so that a hook finds the handle complete; a hook's
    // failure does not fail create, its message stays in the handle's error string.
    for (const OptRow& row : kOptions)
        if (const char* v = row.env ? std::getenv(row.env) : nullptr)
            (void)set_option_row(h, row, row.field == &Options::conv ? conv_decode(v, 0) : std::atoi(v) != 0);
    *out = h;
    return RVDD_OK;
}

void rvdd_destroy(rvdd_t* h) {
    if (!h) return;
    DeviceGuard guard(h->cfg.device);
    (void)hipDeviceSynchronize();
    drop_graphs(h);
    if (h->g_in) (void)hipEventDestroy(h->g_in);
    if (h->g_out) (void)hipEventDestroy(h->g_out);
    if (h->gstream) (void)hipStreamDestroy(h->gstream);
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->scratch) (void)hipFree(h->scratch);
    if (h->loss_batch) (void)hipFree(h->loss_batch);
    tvl1_free(h->tvl1);
    for (auto& p : h->pending) {
        (void)hipEventDestroy(p.e0);
        (void)hipEventDestroy(p.e1);
    }
    for (auto e : h->event_pool) (void)hipEventDestroy(e);
    if (h->t0) (void)hipEventDestroy(h->t0);
    if (h->t1) (void)hipEventDestroy(h->t1);
    delete h;
}

int rvdd_set_weight(rvdd_t* h, const char* key, const float* host, const int64_t* shape, int32_t ndim) {
    if (!h || !key || !host || !shape || ndim < 1 || ndim > 4) return fail(h, RVDD_ERR_ARG, "rvdd_set_weight: bad argument");
    if (h->finalized) return fail(h, RVDD_ERR_STATE, "rvdd_set_weight: weights already finalized");
    const auto exp = expected_keys(h);
    const KeySpec* spec = nullptr;
    for (const auto& k : exp)
        if (k.key == key) spec = &k;
    if (!spec) return fail(h, RVDD_ERR_WEIGHT, "unexpected state_dict key '%s' for this architecture", key);
    std::vector<int64_t> shp(shape, shape + ndim);
    if (shp != spec->shape) {
        std::string got, want;
        for (auto v : shp) got += std::to_string(v) + ",";
        for (auto v : spec->shape) want += std::to_string(v) + ",";
        return fail(h, RVDD_ERR_WEIGHT, "state_dict key '%s' has shape [%s] but [%s] is expected", key, got.c_str(), want.c_str());
    }
    size_t n = 1;
    for (auto v : shp) n *= (size_t)v;
    HostTensor t;
    t.shape = shp;
    t.data.assign(host, host + n);
    h->staged[key] = std::move(t);
    return RVDD_OK;
}

int rvdd_finalize_weights(rvdd_t* h) {
    if (!h) return RVDD_ERR_ARG;
    if (h->finalized) return RVDD_OK;
    for (const auto& k : expected_keys(h))
        if (!h->staged.count(k.key)) return fail(h, RVDD_ERR_WEIGHT, "missing state_dict key '%s'", k.key.c_str());
    ENTER(h);
    if (!h->is_next()) {
        for (const auto& n : convunet_conv_names(h->has_feat())) {
            const HostTensor& wt = h->staged.at(n + ".weight");
            Conv3 L;
            const int cin = (int)wt.shape[1];
            if (cin == 96) {
                L.nsrc = 2;
                for (int sidx = 0; sidx < 2; ++sidx) {
                    L.cin_real[sidx] = 48;
                    L.cin_pad[sidx] = 48;
                    RC(upload(h, &L.w[sidx], arrange_conv3x3(wt, 48 * sidx, 48, 48)));
                    RC(upload(h, &L.wu[sidx], arrange_wino3x3(wt, 48 * sidx)));
                    RC(upload(h, &L.wh[sidx], arrange_conv3x3h(wt, 48 * sidx, &L.wh_inv[sidx])));
                }
            } else {
                L.nsrc = 1;
                L.cin_real[0] = cin;
                L.cin_pad[0] = cin == 48 ? 48 : kNetInC;
                RC(upload(h, &L.w[0], arrange_conv3x3(wt, 0, cin, L.cin_pad[0])));
                RC(upload(h, &L.wu[0], cin == 48 ? arrange_wino3x3(wt, 0) : arrange_wino3x3(wt, 0, 1)));
                RC(upload(h, &L.wh[0], arrange_conv3x3h(wt, 0, &L.wh_inv[0], cin == 48 ? 48 : 16)));
            }
            RC(upload(h, &L.bias, h->staged.at(n + ".bias").data));
            for (int li = 0; li < CU_COUNT; ++li)
                if (n == kCuNames[li]) h->cu[li] = L;
        }
        RC(upload(h, &h->w_out, h->staged.at("PostConvs.1.weight").data));
        RC(upload(h, &h->b_out, h->staged.at("PostConvs.1.bias").data));
        if (h->has_feat()) RC(compose_pre_enc0(h));
    } else {
        RC(finalize_convnext(h));
    }
    h->staged.clear();
    h->finalized = true;
    return RVDD_OK;
}

// Host-only helper of the TIFF reader (rvdd-release_amd/tiffio.py): TIFF 6.0 section 13 LZW (MSB-first codes of
// 9..12 bits, ClearCode 256, EndOfInformation 257, "early change").  The pure-Python decoder does ~1 MB/s, a
// 1280x720 four-channel float frame is 15 MB.  Returns the number of bytes produced, or -1 on a corrupt stream / a
// full output buffer.
int64_t rvdd_tiff_lzw_decode(const uint8_t* in, int64_t n, uint8_t* out, int64_t cap) {
    if (!in || !out || n < 0 || cap < 0) return -1;
    struct Entry { int32_t prev; uint16_t len; uint8_t first, last; };
    static thread_local Entry tab[4096];
    for (int i = 0; i < 256; ++i) tab[i] = Entry{-1, 1, (uint8_t)i, (uint8_t)i};
    int next = 258, nbits = 9, prev = -1;
    uint32_t buf = 0;
    int have = 0;
    int64_t pos = 0, o = 0;
    for (;;) {
        while (have < nbits) {
            if (pos >= n) return o;                    // streams without an EOI code end with the data
            buf = (buf << 8) | in[pos++];
            have += 8;
        }
        const int code = (int)((buf >> (have - nbits)) & ((1u << nbits) - 1u));
        have -= nbits;
        if (code == 257) return o;
        if (code == 256) {
            next = 258;
            nbits = 9;
            prev = -1;
            continue;
        }
        int cur;
        if (prev < 0) {
            if (code >= 256) return -1;
            cur = code;
        } else if (code < next) {
            cur = code;
            if (next < 4096) {
                tab[next] = Entry{prev, (uint16_t)(tab[prev].len + 1), tab[prev].first, tab[code].first};
                ++next;
            }
        } else if (code == next && next < 4096) {
            tab[next] = Entry{prev, (uint16_t)(tab[prev].len + 1), tab[prev].first, tab[prev].first};
            cur = next++;
        } else {
            return -1;
        }
        const int len = tab[cur].len;
        if (o + len > cap) return -1;
        for (int e = cur, k = len - 1; k >= 0; --k, e = tab[e].prev) out[o + k] = tab[e].last;
        o += len;
        prev = cur;
        if (next >= 2047) nbits = 12;
        else if (next >= 1023) nbits = 11;
        else if (next >= 511) nbits = 10;
    }
}

int rvdd_set_option(rvdd_t* h, const char* name, int32_t value) {
    if (!h || !name) return RVDD_ERR_ARG;
    {
        ENTER(h);
        (void)hipDeviceSynchronize();
        drop_graphs(h);            // a captured step has the options it was captured with
    }
    for (const OptRow& row : kOptions)
        if (std::strcmp(name, row.name) == 0) return set_option_row(h, row, value);
    return fail(h, RVDD_ERR_ARG, kUnknownOption, name);
}

int rvdd_reset(rvdd_t* h) {
    if (!h) return RVDD_ERR_ARG;
    h->reset_marks = slots_below(h->cfg.batch);
    return RVDD_OK;
}

int rvdd_reset_slots(rvdd_t* h, const uint8_t* mask) {
    if (!h) return RVDD_ERR_ARG;
    if (!mask) return fail(h, RVDD_ERR_ARG, "rvdd_reset_slots: mask is required");
    const int B = h->cfg.batch;
    int count = 0;
    for (int b = 0; b < B; ++b) count += mask[b] != 0;
    if (count == 0) return RVDD_OK;
    if (count == B) return rvdd_reset(h);      // every slot
    if (B > 64) return fail(h, RVDD_ERR_ARG, "rvdd_reset_slots: a mask of some slots needs batch <= 64 (batch is %d)", B);
    for (int b = 0; b < B; ++b)
        if (mask[b]) h->reset_marks |= 1ull << b;
    return RVDD_OK;
}

}  // extern "C"

namespace {

// The stages in front of the net for sequences [sb.b0, sb.b0 + sb.nb): one launch covers them all -- the kernels take
// the caller's batch strides (channel slices of the reference's wider `n` / `flow` tensors are strided over the batch).
int run_prologue(rvdd_t* h, NetRun& run, Sub sb, hipStream_t s) {
    const StepInputs& in = *run.in;
    const bool nw = h->opt.no_warp;
    const int H = h->cfg.height, W = h->cfg.width;
    const size_t img = (size_t)H * W, npix = (size_t)h->cfg.batch * img;
    const size_t o = (size_t)sb.b0;
    const int n = sb.nb;
    const float* rc_ = in.raw_cur + o * in.rawf;
    const float* fp_ = in.flow_prev ? in.flow_prev + o * in.flowf : nullptr;
    const float* rn_ = in.raw_next ? in.raw_next + o * in.rawf : nullptr;
    const float* fn_ = in.flow_next ? in.flow_next + o * in.flowf : nullptr;
    float* green = h->green + o * img;
    float* netin = h->netin + o * img * kNetInC;
    // amax words of the maps the split-f16 convs read first (block floating point, rvdd_internal.h)
    const bool bfp = h->amax_on();
    unsigned* amax_netin = bfp ? amax_words(h, run.amax.base + AMAX_REL_NETIN, o) : nullptr;
    // the zeroing for the step after this one rides in the first netin_bound launch of the step; a step without one memsets
    const AmaxSlots after = step_amax(h->step_ctr + 1);
    unsigned* zero_a = amax_words(h, after.base);
    unsigned* zero_b = amax_words(h, after.post_out);
    const size_t zero_na = amax_bytes(h->cfg.batch, AMAX_NREG) / 4, zero_nb = amax_bytes(h->cfg.batch, 1) / 4;
    const bool zero_now = bfp && run.zero_pending;
    run.zero_pending = false;
    // which of these sequences start a video (rvdd_reset_slots): they bound the network input from raw_prev, the others from the
    // words of their previous output -- each sequence gets the words it would get alone
    const unsigned long long latch = in.latch == ~0ull ? ~0ull : (o < 64 ? in.latch >> o : 0ull);
    if (h->opt.warp_raw && !nw) {
        // warp_frame with --warp_raw (models/recurrent_model.py:149-152): HA(warp(remosaick(frame), raw-resolution flow)).
        // remosaick(HA(raw)) is raw itself, so the next frame is warped as it came.  next4 is free in this mode: its
        // first quarter holds the re-mosaicked previous output, the second the warped planes.  The generic NCHW warp
        // takes dense tensors: one sequence at a time when the caller's are strided (a mode without checkpoints of its own).
        const bool dense = in.rawf == (size_t)4 * (H / 2) * (W / 2) && in.flowf == (size_t)2 * (H / 2) * (W / 2);
        {
            Scope sc(h, s, "demosaic(ha_green+ha_rb)", 0.0, (double)n * img * 16.0);
            HIPCHK(h, launch_demosaic(rc_, green, netin + 3, n, H / 2, W / 2, (int64_t)H * W * kNetInC, kNetInC, 1, s, (int64_t)in.rawf,
                                      h->opt.bayer));
        }
        for (int b = 0; b < n; b += dense ? n : 1) {
            const int nb = dense ? n : 1;
            float* packed = h->next4 + (o + b) * img;
            float* warped = h->next4 + npix + (o + b) * img;
            HIPCHK(h, launch_remosaick4(h->lastden4 + (o + b) * img * 4, packed, nb, H, W, s, h->opt.bayer));
            HIPCHK(h, launch_warp_nchw(packed, fp_ + b * in.flowf, warped, nb, 4, H / 2, W / 2, s));
            HIPCHK(h, launch_demosaic(warped, green + b * img, netin + b * img * kNetInC + 0, nb, H / 2, W / 2, (int64_t)H * W * kNetInC,
                                      kNetInC, 1, s, 0, h->opt.bayer));
            if (h->cfg.future) {
                HIPCHK(h, launch_warp_nchw(rn_ + b * in.rawf, fn_ + b * in.flowf, warped, nb, 4, H / 2, W / 2, s));
                HIPCHK(h, launch_demosaic(warped, green + b * img, netin + b * img * kNetInC + 6, nb, H / 2, W / 2,
                                          (int64_t)H * W * kNetInC, kNetInC, 1, s, 0, h->opt.bayer));
            }
        }
        if (amax_netin) HIPCHK(h, launch_amax_reduce(netin, n, (int64_t)img * kNetInC, amax_netin, s));
        if (zero_now) {
            HIPCHK(h, hipMemsetAsync(zero_a, 0, zero_na * 4, s));
            HIPCHK(h, hipMemsetAsync(zero_b, 0, zero_nb * 4, s));
        }
    } else {
        // the whole NHWC16 input pixel in one pass: warp of the previous output | demosaic of the current frame |
        // warp of the demosaicked next frame
        float* next4 = nullptr;
        if (h->cfg.future) {
            next4 = h->next4 + o * img * 4;
            HIPCHK(h, launch_demosaic(rn_, green, next4, n, H / 2, W / 2, (int64_t)H * W * 4, 4, 1, s, (int64_t)in.rawf, h->opt.bayer));
        }
        Scope sc(h, s, "netin(ha_green+netin_kernel)", 0.0, (double)n * img * (16.0 + 16.0 + 48.0 + (next4 ? 16.0 : 0.0)));
        // small frames without a future frame: the bound, the green plane and the network input in ONE launch
        if (!h->is_next() && !h->opt.prev_noisy && netin_small_applies(n, H / 2, W / 2, h->cfg.future != 0, h->opt.small_prestage)) {
            const float* rp_ = in.raw_prev ? in.raw_prev + o * in.rawf : nullptr;
            HIPCHK(h, launch_netin_small(rc_, rp_, h->lastden4 + o * img * 4, fp_, netin, n, H / 2, W / 2, (int64_t)in.rawf, (int64_t)in.flowf,
                                         amax_netin && latch != ~0ull ? amax_words(h, run.amax.feat_in, o) : nullptr, amax_netin, s,
                                         zero_now ? zero_a : nullptr, zero_na, zero_now ? zero_b : nullptr, zero_nb, latch, h->opt.bayer));
            goto prologue_features;
        }
        if (amax_netin) {
            // (block floating point) a bound of max |netin| from the raw frames and from the words PostConvs wrote last step;
            // with --prev_noisy_frame the "previous output" is a demosaicked frame whose raw data is gone: its own maximum
            const float* rp_ = in.raw_prev ? in.raw_prev + o * in.rawf : nullptr;
            HIPCHK(h, launch_netin_bound(rc_, rn_, rp_, n, H / 2, W / 2, (int64_t)in.rawf,
                                         latch == ~0ull ? nullptr : amax_words(h, run.amax.feat_in, o), amax_netin, s,
                                         zero_now ? zero_a : nullptr, zero_na, zero_now ? zero_b : nullptr, zero_nb, latch));
            if (h->opt.prev_noisy && latch != ~0ull)      // over the runs of sequences that continue a video (one run without a reset)
                for (int b = 0; b < n;) {
                    if ((latch >> b) & 1ull) { ++b; continue; }
                    int e = b + 1;
                    while (e < n && !((latch >> e) & 1ull)) ++e;
                    HIPCHK(h, launch_amax_reduce(h->lastden4 + (o + b) * img * 4, e - b, (int64_t)img * 4, amax_netin + (size_t)b * kAmaxSeqWords, s, 1));
                    b = e;
                }
        }
        // ConvNeXtUnet: the input's only reader is the 1x1 projection of the first ConvBlock, which rides in the same kernel
        const NextBlk* first = h->is_next() && h->opt.next_projfuse ? &h->nx[h->has_feat() ? NX_PRE : NX_ENC0_0] : nullptr;
        run.netin_proj = first != nullptr;
        HIPCHK(h, launch_netin(rc_, green, h->lastden4 + o * img * 4, fp_, next4, fn_, netin, n, H / 2, W / 2, s, (int64_t)in.rawf,
                               (int64_t)in.flowf, first ? first->w.proj_w : nullptr, first ? first->w.proj_b : nullptr,
                               first ? h->lv[0].t[0] + o * img * kF : nullptr, h->opt.bayer));
    }
prologue_features:
    if (h->has_feat() && !nw) {
        run.featw_proj = next_pf_pre(h);
        Scope sc(h, s, "warp48_kernel", run.featw_proj ? 2.0 * 48 * 48 * n * img : 0.0, (double)n * img * (384.0 + 2.0));
        if (run.featw_proj)
            HIPCHK(h, launch_warp48_proj(h->lastfeat + o * img * kF, fp_, h->featw + o * img * kF, n, H, W, h->nx[NX_ENC0_0].half[1].frag,
                                         h->nx[NX_ENC0_0].half[1].inv_e, h->nx[NX_ENC0_0].w.proj_b, s, (int64_t)in.flowf));
        else
            HIPCHK(h, launch_warp48(h->lastfeat + o * img * kF, fp_, h->featw + o * img * kF, n, H, W, s, (int64_t)in.flowf));
    }
    return RVDD_OK;
}

// One frame-step as step_n planned it: the caller's tensors, the slots it covers and which of them start a video.
struct StepPlan {
    int n;                  // slots [0, n): cfg.batch, or the live ones of rvdd_step_live
    const float *raw_prev, *raw_cur, *raw_next, *flow_prev, *flow_next;
    int64_t raw_stride, flow_stride;
    float* out_rgb;
    bool init;              // every covered slot starts a video
    uint64_t pend;          // else: the covered slots that do (rvdd_reset_slots)
};

// Every launch of one frame-step, in order, on stream s.  The handle is read only: commit_step moves it on.
int enqueue_step(rvdd_t* h, const StepPlan& p, hipStream_t s) {
    const bool nw = h->opt.no_warp, init = p.init;
    const int B = p.n, H = h->cfg.height, W = h->cfg.width;
    const size_t npix = (size_t)B * H * W;
    const uint64_t pend = p.pend;
    const float *raw_prev = p.raw_prev, *raw_cur = p.raw_cur;
    StepInputs in;
    in.raw_prev = init || pend ? raw_prev : nullptr;
    in.latch = init ? ~0ull : pend;
    in.raw_cur = raw_cur; in.raw_next = p.raw_next; in.flow_prev = p.flow_prev; in.flow_next = p.flow_next;
    in.rawf = p.raw_stride ? (size_t)p.raw_stride : (size_t)4 * (H / 2) * (W / 2);
    in.flowf = p.flow_stride ? (size_t)p.flow_stride : (size_t)2 * (H / 2) * (W / 2);
    NetRun run;
    run.n = B;
    run.amax = step_amax(h->step_ctr);
    run.in = &in;
    // amax words: everything but the recurrent features' words this step reads (zero features at the start of a video: zero words)
    if (h->amax_on()) {
        // the first step of a video starts from zero features: zero words; later steps find their set zeroed by the step before
        if (init) HIPCHK(h, hipMemsetAsync(h->amax, 0, amax_bytes(h->cfg.batch, AMAX_SLOTS), s));
        run.zero_pending = true;
    }
    if (init) {
        // lastden = n[:, :3] (demosaiced previous noisy frame), features = 0
        // (models/recurrent_model.py:233-245)
        HIPCHK(h, launch_demosaic(raw_prev, h->green, h->lastden4, B, H / 2, W / 2, (int64_t)H * W * 4, 4, 1, s, (int64_t)in.rawf,
                                  h->opt.bayer));
        if (h->has_feat()) HIPCHK(h, hipMemsetAsync(h->lastfeat, 0, npix * kF * sizeof(float), s));
    } else if (pend) {
        // some sequences start a video (rvdd_reset_slots): the same latch for them alone -- the demosaic over each run of
        // them, then ONE launch that zeroes their features and their words in every set (the rotation of the sets by step_ctr
        // is harmless only because a latched sequence has all of them zeroed)
        const size_t img = (size_t)H * W;
        for (int b = 0; b < B;) {
            if (!((pend >> b) & 1u)) { ++b; continue; }
            int e = b + 1;
            while (e < B && ((pend >> e) & 1u)) ++e;
            HIPCHK(h, launch_demosaic(raw_prev + b * in.rawf, h->green + b * img, h->lastden4 + b * img * 4, e - b, H / 2, W / 2,
                                      (int64_t)H * W * 4, 4, 1, s, (int64_t)in.rawf, h->opt.bayer));
            b = e;
        }
        HIPCHK(h, launch_latch_zero(pend, h->has_feat() ? h->lastfeat : nullptr, (int64_t)img * kF, h->amax_on() ? h->amax : nullptr, AMAX_SLOTS,
                                    h->cfg.batch, s));
    }
    // without warping the previous features are read in place: the net consumes them in its first layer and only
    // its last one writes the new ones
    const int rc = run_net(h, run, h->netin, nw ? h->lastfeat : h->featw, h->lastfeat, p.out_rgb, h->lastden4, s);
    if (rc == RVDD_OK && h->opt.prev_noisy)     // store_frame = the noisy current frame (models/recurrent_model.py:335-337)
        HIPCHK(h, launch_demosaic(raw_cur, h->green, h->lastden4, B, H / 2, W / 2, (int64_t)H * W * 4, 4, 1, s, (int64_t)in.rawf,
                                  h->opt.bayer));
    return rc;
}

constexpr size_t kMaxStepGraphs = 128;      // one per distinct set of caller buffers; least recently used goes first

// A frame-step is ~30-45 launches.  The schedule is fixed by (configuration, options, first-frame flag) and the six
// caller pointers, so each distinct pointer set can be captured once into a hipGraph (on a stream of the handle) and
// replayed afterwards -- rvdd_set_option(h, "graphs", 1) or RVDD_GRAPH=1; the caller's stream is joined on both sides
// with events, so stream order is what it would be launch by launch.  OFF by default: on ROCm 7.2 the replay is
// SLOWER than the eager launches it replaces at every size measured (profiles/r02_e_hipgraph_step_ab.log: 256x256
// B = 1 2110 vs 2440 frames/s, B = 4 5035 vs 5320; 720p B = 1 398.6 vs 404.5, B = 4 456.9 vs 459.4).  The eager path
// is not host-bound -- launches are asynchronous and the queue stays full -- and kernel boundaries cost the same
// either way, so a graph has only its own launch cost to add.  Parity is identical (the GPU suite passes in both modes).
// Where no graph can be made, this step and every later one of the handle are enqueued launch by launch instead.
int replay_step(rvdd_t* h, const StepPlan& p, hipStream_t s) {
    rvdd_handle::StepKey key{{p.init ? p.raw_prev : nullptr, p.raw_cur, p.raw_next, p.flow_prev, p.flow_next, p.out_rgb},
                             {p.raw_stride, p.flow_stride}, (p.init ? 1 : 0) | (h->serpentine ? 2 : 0) | (h->step_ctr << 2)};
    auto it = h->graphs.find(key);
    if (it == h->graphs.end()) {
        hipGraph_t g = nullptr;
        hipGraphExec_t ex = nullptr;
        hipError_t e = hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal);
        int rc = RVDD_OK;
        if (e == hipSuccess) {
            rc = enqueue_step(h, p, h->gstream);
            e = hipStreamEndCapture(h->gstream, &g);
        }
        if (e == hipSuccess && rc == RVDD_OK) e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
        if (e != hipSuccess || rc != RVDD_OK) {
            // no graph for this process: run this step and every later one launch by launch, on the caller's stream
            // (whatever failed -- the capture, the instantiation or a launch inside the capture -- nothing has run yet)
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            h->opt.use_graphs = 0;
            return enqueue_step(h, p, s);
        }
        if (h->graphs.size() >= kMaxStepGraphs) {
            auto old = h->graphs.begin();
            for (auto jt = h->graphs.begin(); jt != h->graphs.end(); ++jt)
                if (jt->second.last_use < old->second.last_use) old = jt;
            (void)hipGraphExecDestroy(old->second.exec);
            (void)hipGraphDestroy(old->second.graph);
            h->graphs.erase(old);
        }
        rvdd_handle::StepGraph sg;
        sg.graph = g;
        sg.exec = ex;
        it = h->graphs.emplace(key, sg).first;
    }
    it->second.last_use = ++h->graph_tick;
    HIPCHK(h, hipEventRecord(h->g_in, s));
    HIPCHK(h, hipStreamWaitEvent(h->gstream, h->g_in, 0));
    HIPCHK(h, hipGraphLaunch(it->second.exec, h->gstream));
    HIPCHK(h, hipEventRecord(h->g_out, h->gstream));
    HIPCHK(h, hipStreamWaitEvent(s, h->g_out, 0));
    return RVDD_OK;
}

// A step over slots [0, n) has been enqueued: their marks are spent (`keep`: those of the others), the slots that sat it
// out are undefined, the amax words' set and slots (step_amax) and the sequence order move on.  A step that failed half
// way never gets here: the handle still asks for the first frame of a video (raw_prev, zeroed features), never for a
// later frame on stale state.
void commit_step(rvdd_t* h, int n, uint64_t keep) {
    h->reset_marks = keep;
    h->undef_mask = slots_below(h->cfg.batch) & ~slots_below(n);
    h->step_ctr = (h->step_ctr + 1) % 6;
    if (seq_major_on(h, n)) h->serpentine = !h->serpentine;
}

// rvdd_step_strided (n = cfg.batch) and rvdd_step_live: validate, plan, enqueue or replay, commit
int step_n(rvdd_t* h, const int n, const float* raw_prev, const float* raw_cur, const float* raw_next, const float* flow_prev,
           const float* flow_next, int64_t raw_stride, int64_t flow_stride, float* out_rgb, void* stream) {
    ENTER(h);
    if (!h->finalized) return fail(h, RVDD_ERR_STATE, "rvdd_step: weights not finalized");
    {
        const int64_t rd = (int64_t)4 * (h->cfg.height / 2) * (h->cfg.width / 2), fd = rd / 2;
        if ((raw_stride && raw_stride < rd) || (flow_stride && flow_stride < fd))
            return fail(h, RVDD_ERR_ARG, "rvdd_step_strided: a batch stride must be 0 (dense) or at least one sequence (%lld / %lld floats)",
                        (long long)rd, (long long)fd);
    }
    const bool nw = h->opt.no_warp;
    if (!raw_cur || (!flow_prev && !nw) || !out_rgb) return fail(h, RVDD_ERR_ARG, "rvdd_step: raw_cur, flow_prev and out_rgb are required");
    if (h->cfg.future && (!raw_next || (!flow_next && !nw))) return fail(h, RVDD_ERR_ARG, "rvdd_step: raw_next and flow_next are required when future=1");
    if (nw) flow_prev = flow_next = nullptr;      // the flows are not looked at (the reference's dataset does not even load them)
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the marks of the covered slots are this step's, those of the others stay pending.  Every covered slot marked = the
    // first step of a handle of n sequences, launch for launch (one demosaic, memsets), not the per-run latch of `pend`.
    const uint64_t live = slots_below(n), keep = h->reset_marks & ~live;
    const bool init = (h->reset_marks & live) == live;
    const uint64_t pend = init ? 0 : h->reset_marks & live;
    if (const uint64_t bad = h->undef_mask & live & ~(init ? live : pend))
        return fail(h, RVDD_ERR_STATE, "rvdd_step: the state of slot %d is undefined (it sat out a step of fewer slots, or was moved "
                    "away): mark it with rvdd_reset_slots, set its state, or move a sequence into it first", __builtin_ctzll(bad));
    if ((init || pend) && !raw_prev) return fail(h, RVDD_ERR_ARG, "rvdd_step: raw_prev is required on the first step of a video");
    const StepPlan plan{n, raw_prev, raw_cur, raw_next, flow_prev, flow_next, raw_stride, flow_stride, out_rgb, init, pend};
    // never captured: a profiled step, the first step of a handle, a partial reset, a step of some slots
    const bool replay = h->opt.use_graphs && !h->prof_on && h->ran_eagerly && h->gstream && !pend && n == h->cfg.batch;
    h->ran_eagerly = true;
    RC(replay ? replay_step(h, plan, s) : enqueue_step(h, plan, s));
    commit_step(h, n, keep);
    return RVDD_OK;
}

}  // namespace

extern "C" {

int rvdd_step(rvdd_t* h, const float* raw_prev, const float* raw_cur, const float* raw_next,
              const float* flow_prev, const float* flow_next, float* out_rgb, void* stream) {
    return rvdd_step_strided(h, raw_prev, raw_cur, raw_next, flow_prev, flow_next, 0, 0, out_rgb, stream);
}

int rvdd_step_strided(rvdd_t* h, const float* raw_prev, const float* raw_cur, const float* raw_next,
                      const float* flow_prev, const float* flow_next, int64_t raw_stride, int64_t flow_stride,
                      float* out_rgb, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    return step_n(h, h->cfg.batch, raw_prev, raw_cur, raw_next, flow_prev, flow_next, raw_stride, flow_stride, out_rgb, stream);
}

// Slots [0, n_live) alone: the launches of a step of n_live sequences over the first n_live slices of the handle's maps (every
// launch of a step takes a sequence range already; the amax words keep the handle's own batch stride).  The sequences that sit
// the step out are undefined afterwards: the sets of words rotate with step_ctr, which this step advances for the whole handle.
int rvdd_step_live(rvdd_t* h, int32_t n_live, const float* raw_prev, const float* raw_cur, const float* raw_next,
                   const float* flow_prev, const float* flow_next, int64_t raw_stride, int64_t flow_stride,
                   float* out_rgb, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (n_live < 1 || n_live > h->cfg.batch)
        return fail(h, RVDD_ERR_ARG, "rvdd_step_live: n_live must be 1..%d (the handle's batch), got %d", h->cfg.batch, n_live);
    if (n_live < h->cfg.batch && h->cfg.batch > 64)
        return fail(h, RVDD_ERR_ARG, "rvdd_step_live: a step of some slots needs batch <= 64 (batch is %d)", h->cfg.batch);
    return step_n(h, n_live, raw_prev, raw_cur, raw_next, flow_prev, flow_next, raw_stride, flow_stride, out_rgb, stream);
}

int rvdd_move_slots(rvdd_t* h, const int32_t* from, const int32_t* to, int32_t count, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (count == 0) return RVDD_OK;
    if (count < 0 || !from || !to) return fail(h, RVDD_ERR_ARG, "rvdd_move_slots: bad argument");
    const int B = h->cfg.batch, H = h->cfg.height, W = h->cfg.width;
    if (B > 64) return fail(h, RVDD_ERR_ARG, "rvdd_move_slots: needs batch <= 64 (batch is %d)", B);
    uint64_t seen = 0;
    for (int k = 0; k < count; ++k)
        for (const int b : {from[k], to[k]}) {
            if (b < 0 || b >= B) return fail(h, RVDD_ERR_ARG, "rvdd_move_slots: slot %d outside 0..%d", b, B - 1);
            if ((seen >> b) & 1ull)
                return fail(h, RVDD_ERR_ARG, "rvdd_move_slots: slot %d appears twice (the pairs of a call must be disjoint)", b);
            seen |= 1ull << b;
        }
    // (disjoint slots below 64: count <= 32 = kMaxMovePairs)
    ENTER(h);
    const size_t img = (size_t)H * W;
    HIPCHK(h, launch_move_slots(from, to, count, h->lastden4, (int64_t)img * 4, h->has_feat() ? h->lastfeat : nullptr, (int64_t)img * kF,
                                h->amax_on() ? h->amax : nullptr, AMAX_SLOTS, B, static_cast<hipStream_t>(stream)));
    // the host-side marks travel with the state; the source is undefined from here on (and has no mark of its own any more)
    uint64_t marks = h->reset_marks, undef = h->undef_mask;
    for (int k = 0; k < count; ++k) {
        const uint64_t f = 1ull << from[k], t = 1ull << to[k];
        marks = (marks & ~(f | t)) | ((marks & f) ? t : 0);
        undef = (undef & ~t) | ((undef & f) ? t : 0) | f;
    }
    h->reset_marks = marks;
    h->undef_mask = undef;
    return RVDD_OK;
}

int rvdd_get_state(rvdd_t* h, float* lastden, float* lastfeat, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = h->cfg.batch, H = h->cfg.height, W = h->cfg.width;
    if (lastden) HIPCHK(h, launch_nhwc_to_nchw(h->lastden4, lastden, B, 3, H, W, 4, s));
    if (lastfeat) {
        if (!h->has_feat()) return fail(h, RVDD_ERR_ARG, "rvdd_get_state: this architecture has no recurrent features");
        HIPCHK(h, launch_nhwc_to_nchw(h->lastfeat, lastfeat, B, kF, H, W, kF, s));
    }
    return RVDD_OK;
}

int rvdd_set_state(rvdd_t* h, const float* lastden, const float* lastfeat, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = h->cfg.batch, H = h->cfg.height, W = h->cfg.width;
    if (lastfeat && !h->has_feat()) return fail(h, RVDD_ERR_ARG, "rvdd_set_state: this architecture has no recurrent features");
    if (lastden) {
        HIPCHK(h, launch_nchw_to_nhwc(lastden, h->lastden4, B, 3, H, W, 4, s));
        h->reset_marks = 0;
        h->undef_mask = 0;
    }
    if (lastfeat) HIPCHK(h, launch_nchw_to_nhwc(lastfeat, h->lastfeat, B, kF, H, W, kF, s));
    if ((lastden || lastfeat) && h->amax_on()) {
        // The words the next step reads as the bound of "the previous output" (block floating point): features and output frame
        // together, as PostConvs leaves them -- rebuilt from the state as it now stands, whichever half the caller replaced
        unsigned* w = amax_words(h, step_amax(h->step_ctr).feat_in);
        HIPCHK(h, hipMemsetAsync(w, 0, amax_bytes(B, 1), s));
        if (h->has_feat()) HIPCHK(h, launch_amax_reduce(h->lastfeat, B, (int64_t)H * W * kF, w, s));
        HIPCHK(h, launch_amax_reduce(h->lastden4, B, (int64_t)H * W * 4, w, s));
    }
    return RVDD_OK;
}

int rvdd_psnr_l1(rvdd_t* h, const float* den, const float* gt, int64_t count, float* out2, void* stream) {
    if (!h || !den || !gt || !out2 || count <= 0) return fail(h, RVDD_ERR_ARG, "rvdd_psnr_l1: bad argument");
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int nblk = (int)((count + 256 * 16 - 1) / (256 * 16));
    if (nblk > 1024) nblk = 1024;
    HIPCHK(h, launch_loss_reduce(den, gt, count, h->loss_partial, nblk, h->loss_result, s));
    double r[2];
    HIPCHK(h, hipMemcpyAsync(r, h->loss_result, sizeof r, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (hipError_t e = tvl1_check(h->tvl1, s); e != hipSuccess)       // an asynchronous flow batch in front of the frames just measured
        return fail(h, RVDD_ERR_HIP, "rvdd_psnr_l1: an asynchronous rvdd_tvl1flow_batch before this call failed: %s", hipGetErrorString(e));
    out2[0] = (float)(100.0 * r[0] / (double)count);
    out2[1] = (float)(10.0 * std::log10(4.0 / (r[1] / (double)count)));
    return RVDD_OK;
}

int rvdd_psnr_l1_batch(rvdd_t* h, const float* den, const float* gt, int32_t n, int64_t count, float* out, void* stream) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !den || !gt || !out || n < 0 || count <= 0) return fail(h, RVDD_ERR_ARG, "rvdd_psnr_l1_batch: bad argument");
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int nblk = (int)((count + 256 * 16 - 1) / (256 * 16));      // rvdd_psnr_l1's partition of every slice
    if (nblk > 1024) nblk = 1024;
    const size_t need = (size_t)n * (2 * nblk + 2);
    if (h->loss_batch_cap < need) {
        if (h->loss_batch) {
            HIPCHK(h, hipDeviceSynchronize());
            HIPCHK(h, hipFree(h->loss_batch));
            h->loss_batch = nullptr;
            h->loss_batch_cap = 0;
        }
        HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->loss_batch), need * sizeof(double)));
        h->loss_batch_cap = need;
    }
    double* res = h->loss_batch + (size_t)n * 2 * nblk;
    HIPCHK(h, launch_loss_reduce_batch(den, gt, n, count, h->loss_batch, nblk, res, s));
    std::vector<double> r((size_t)2 * n);
    HIPCHK(h, hipMemcpyAsync(r.data(), res, r.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (hipError_t e = tvl1_check(h->tvl1, s); e != hipSuccess)
        return fail(h, RVDD_ERR_HIP, "rvdd_psnr_l1_batch: an asynchronous rvdd_tvl1flow_batch before this call failed: %s", hipGetErrorString(e));
    for (int i = 0; i < n; ++i) {
        out[2 * i] = (float)(100.0 * r[2 * i] / (double)count);
        out[2 * i + 1] = (float)(10.0 * std::log10(4.0 / (r[2 * i + 1] / (double)count)));
    }
    return RVDD_OK;
}

int rvdd_unet_forward(rvdd_t* h, const float* x, const float* feat_in, float* out, float* feat_out, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    ENTER(h);
    if (!h->finalized) return fail(h, RVDD_ERR_STATE, "rvdd_unet_forward: weights not finalized");
    if (!x || !out) return fail(h, RVDD_ERR_ARG, "rvdd_unet_forward: x and out are required");
    if (h->has_feat() && !feat_in)
        return fail(h, RVDD_ERR_STATE, "Old features is None, please call get_rec_nil_features first.");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int B = h->cfg.batch, H = h->cfg.height, W = h->cfg.width;
    HIPCHK(h, launch_nchw_to_nhwc(x, h->netin, B, h->cin_real(), H, W, kNetInC, s));
    if (h->has_feat()) HIPCHK(h, launch_nchw_to_nhwc(feat_in, h->featw, B, kF, H, W, kF, s));
    // amax words of the caller's maps (block floating point of the split-f16 convs); the recurrent features' words stay as they are
    NetRun run;
    run.n = B;
    run.amax = forward_amax();
    if (h->amax_on()) {
        HIPCHK(h, hipMemsetAsync(amax_words(h, run.amax.base), 0, amax_bytes(B, AMAX_NREG), s));
        HIPCHK(h, launch_amax_reduce(h->netin, B, (int64_t)H * W * kNetInC, amax_words(h, run.amax.base + AMAX_REL_NETIN), s));
        if (h->has_feat()) HIPCHK(h, launch_amax_reduce(h->featw, B, (int64_t)H * W * kF, amax_words(h, run.amax.feat_in), s));
    }
    RC(run_net(h, run, h->netin, h->featw, h->lv[0].t[2], out, nullptr, s));
    if (seq_major_on(h, B) && !h->is_next()) h->serpentine = !h->serpentine;      // the order alternates with every forward
    if (h->has_feat() && feat_out) HIPCHK(h, launch_nhwc_to_nchw(h->lv[0].t[2], feat_out, B, kF, H, W, kF, s));
    return RVDD_OK;
}

int rvdd_demosaic_ha_bayer(rvdd_t* h, const float* raw, int32_t n, int32_t hh, int32_t ww, int32_t pattern, float* rgb, void* stream) {
    if (h && (pattern < RVDD_BAYER_GBRG || pattern > RVDD_BAYER_BGGR))
        return fail(h, RVDD_ERR_ARG, "rvdd_demosaic_ha_bayer: pattern %d is not an rvdd_bayer (0 GBRG, 1 GRBG, 2 RGGB, 3 BGGR)", pattern);
    if (h && n == 0) return RVDD_OK;       // an empty batch is valid and launches nothing
    if (!h || !raw || !rgb || n < 0 || hh < 1 || ww < 1) return fail(h, RVDD_ERR_ARG, "rvdd_demosaic_ha_bayer: bad argument");
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    RC(ensure_scratch(h, (size_t)n * 4 * hh * ww * sizeof(float)));
    const int64_t hw = (int64_t)4 * hh * ww;
    HIPCHK(h, launch_demosaic(raw, h->scratch, rgb, n, hh, ww, 3 * hw, 1, (int)hw, s, 0, pattern));
    return RVDD_OK;
}

int rvdd_demosaic_ha(rvdd_t* h, const float* raw, int32_t n, int32_t hh, int32_t ww, float* rgb, void* stream) {
    return rvdd_demosaic_ha_bayer(h, raw, n, hh, ww, RVDD_BAYER_GBRG, rgb, stream);
}

int rvdd_warp_bicubic(rvdd_t* h, const float* x, const float* flow, int32_t n, int32_t c, int32_t H, int32_t W,
                      float* y, void* stream) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !x || !flow || !y || n < 0 || c < 1 || H < 2 || W < 2) return fail(h, RVDD_ERR_ARG, "rvdd_warp_bicubic: bad argument");
    ENTER(h);
    HIPCHK(h, launch_warp_nchw(x, flow, y, n, c, H, W, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_upsample_factor_2(rvdd_t* h, const float* t, int32_t n, int32_t c, int32_t hh, int32_t ww,
                           float multiply_by, float* out, void* stream) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !t || !out || n < 0 || c < 1 || hh < 1 || ww < 1) return fail(h, RVDD_ERR_ARG, "rvdd_upsample_factor_2: bad argument");
    ENTER(h);
    HIPCHK(h, launch_upsample_flow(t, out, n * c, hh, ww, multiply_by, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_tvl1flow(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t nx, int32_t ny, int32_t* iterations,
                  void* stream) {
    if (!h || !I0 || !I1 || !u || nx < 16 || ny < 16) return fail(h, RVDD_ERR_ARG, "rvdd_tvl1flow: bad argument (images must be >= 16x16)");
    ENTER(h);
    if (!tvl1_size_ok(nx, ny))
        return fail(h, RVDD_ERR_ARG, "rvdd_tvl1flow: image too skinny for its pyramid (the reference reads out of bounds at this size)");
    if (!h->tvl1 || tvl1_ws_nx(h->tvl1) != nx || tvl1_ws_ny(h->tvl1) != ny) {
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, tvl1_check(h->tvl1, static_cast<hipStream_t>(stream)));      // what an asynchronous batch on the old workspace left unread
        tvl1_free(h->tvl1);
        h->tvl1 = nullptr;
        HIPCHK(h, tvl1_alloc(&h->tvl1, nx, ny));
    }
    int it = 0;
    HIPCHK(h, tvl1_run(h->tvl1, I0, I1, u, static_cast<hipStream_t>(stream), iterations ? &it : nullptr));
    if (iterations) *iterations = it;
    return RVDD_OK;
}

int rvdd_ppipe(rvdd_t* h, const float* img, int32_t n, int32_t H, int32_t W, int64_t sn, int64_t sc, int64_t sy, int64_t sx,
               int32_t bit_depth, double rgb_gain, double red_gain, double blue_gain, int32_t iso, uint8_t* out_u8,
               float* out_f32, void* stream) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !img || !out_u8 || n < 0 || H < 1 || W < 1) return fail(h, RVDD_ERR_ARG, "rvdd_ppipe: bad argument");
    ENTER(h);
    if (!(rgb_gain != 0.0) || !(red_gain != 0.0) || !(blue_gain != 0.0)) return fail(h, RVDD_ERR_ARG, "rvdd_ppipe: zero gain");
    // fwd_ppipe.py:29: a float32 tensor of Python-double quotients
    const float gains[3] = {(float)(1.0 / (red_gain * rgb_gain)), (float)(1.0 / rgb_gain), (float)(1.0 / (blue_gain * rgb_gain))};
    HIPCHK(h, launch_ppipe(img, n, H, W, sn, sc, sy, sx, bit_depth, gains, iso, out_u8, out_f32, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_srgb_metrics(rvdd_t* h, const uint8_t* a, const uint8_t* b, int32_t n, int32_t H, int32_t W, double* psnr,
                      double* ssim, void* stream) {
    if (!h || !a || !b || n < 1) return fail(h, RVDD_ERR_ARG, "rvdd_srgb_metrics: bad argument");
    ENTER(h);
    if (H < 7 || W < 7) return fail(h, RVDD_ERR_ARG, "rvdd_srgb_metrics: win_size exceeds image extent (images must be >= 7x7)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    RC(ensure_scratch(h, srgb_metrics_workspace(n, H, W)));
    HIPCHK(h, launch_srgb_metrics(a, b, n, H, W, h->scratch, s));
    std::vector<unsigned long long> ssd(n);
    std::vector<double> sums(n);
    HIPCHK(h, hipMemcpyAsync(ssd.data(), h->scratch, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(sums.data(), reinterpret_cast<char*>(h->scratch) + (size_t)n * 8, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        // mean((a/255 - b/255)^2) = SSD / 255^2 / count; 10 log10(1 / 0) = inf as in numpy
        if (psnr) psnr[i] = 10.0 * std::log10(1.0 / ((double)ssd[i] / (255.0 * 255.0) / ((double)H * W * 3)));
        if (ssim) ssim[i] = sums[i] / (3.0 * (double)(H - 6) * (double)(W - 6));
    }
    return RVDD_OK;
}

}  // extern "C"

namespace {
// rvdd_tvl1flow_batch; `async`: without iteration counts the batch is enqueued and the call returns (option "tvl1_async")
int tvl1flow_batch(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t n, int32_t nx, int32_t ny, int32_t* iterations,
                   void* stream, bool async) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !I0 || !I1 || !u || n < 0 || nx < 16 || ny < 16)
        return fail(h, RVDD_ERR_ARG, "rvdd_tvl1flow_batch: bad argument (images must be >= 16x16)");
    ENTER(h);
    if (!tvl1_size_ok(nx, ny))
        return fail(h, RVDD_ERR_ARG, "rvdd_tvl1flow_batch: image too skinny for its pyramid (the reference reads out of bounds at this size)");
    if (!h->tvl1 || tvl1_ws_nx(h->tvl1) != nx || tvl1_ws_ny(h->tvl1) != ny) {
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, tvl1_check(h->tvl1, static_cast<hipStream_t>(stream)));      // what an asynchronous batch on the old workspace left unread
        tvl1_free(h->tvl1);
        h->tvl1 = nullptr;
        HIPCHK(h, tvl1_alloc(&h->tvl1, nx, ny));
    }
    std::vector<int> it((size_t)n, 0);
    HIPCHK(h, tvl1_run_batch(h->tvl1, I0, I1, u, n, static_cast<hipStream_t>(stream), iterations ? it.data() : nullptr, async));
    if (iterations)
        for (int i = 0; i < n; ++i) iterations[i] = it[(size_t)i];
    return RVDD_OK;
}
}  // namespace

extern "C" {

int rvdd_tvl1flow_batch(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t n, int32_t nx, int32_t ny,
                        int32_t* iterations, void* stream) {
    return tvl1flow_batch(h, I0, I1, u, n, nx, ny, iterations, stream, h && h->opt.tvl1_async);
}

int rvdd_ingest_raw(rvdd_t* h, const void* frames, int32_t dtype, int32_t layout, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
                    float* packed, float* gray, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (dtype != RVDD_RAW_U16 && dtype != RVDD_RAW_F32) return fail(h, RVDD_ERR_ARG, "rvdd_ingest_raw: dtype must be 0 (u16) or 1 (f32), got %d", dtype);
    if (layout != RVDD_RAW_MOSAIC && layout != RVDD_RAW_PACKED_HWC)
        return fail(h, RVDD_ERR_ARG, "rvdd_ingest_raw: layout must be 0 (mosaic) or 1 (packed HWC), got %d", layout);
    if (bit_depth < 1 || bit_depth > 16) return fail(h, RVDD_ERR_ARG, "rvdd_ingest_raw: bit_depth must be 1..16, got %d", bit_depth);
    if (n == 0) return RVDD_OK;
    if (!frames || n < 0 || hh < 1 || ww < 1) return fail(h, RVDD_ERR_ARG, "rvdd_ingest_raw: bad argument (frames, n >= 0, hh, ww >= 1)");
    ENTER(h);
    HIPCHK(h, launch_ingest_raw(frames, dtype, layout, n, hh, ww, bit_depth, packed, gray, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_gray_of_rgb(rvdd_t* h, const float* rgb, int32_t n, int32_t H, int32_t W, int32_t pattern, int32_t bit_depth, float* gray,
                     void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (pattern < RVDD_BAYER_GBRG || pattern > RVDD_BAYER_BGGR)
        return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: pattern %d is not an rvdd_bayer (0 GBRG, 1 GRBG, 2 RGGB, 3 BGGR)", pattern);
    if (bit_depth < 1 || bit_depth > 16) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: bit_depth must be 1..16, got %d", bit_depth);
    if (H < 2 || (H & 1)) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: H must be even and >= 2, got %d", H);
    if (W < 2 || (W & 1)) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: W must be even and >= 2, got %d", W);
    if (n == 0) return RVDD_OK;
    if (n < 0) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: n must be >= 0, got %d", n);
    if (!rgb || !gray) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: rgb and gray are required");
    ENTER(h);
    HIPCHK(h, launch_gray_of_rgb(rgb, n, H / 2, W / 2, pattern, bit_depth, gray, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

// the shape checks rvdd_unprocess and rvdd_unprocess_draws share; 0 = fine
static int unprocess_shape(rvdd_t* h, const char* fn, int32_t n, int32_t H, int32_t W) {
    if (H < 2 || (H & 1)) return fail(h, RVDD_ERR_ARG, "%s: H must be even and >= 2, got %d", fn, H);
    if (W < 2 || (W & 1)) return fail(h, RVDD_ERR_ARG, "%s: W must be even and >= 2, got %d", fn, W);
    if ((int64_t)H * W >= (1ll << 32)) return fail(h, RVDD_ERR_ARG, "%s: H * W must be below 2^32 (the draws count a frame's pixels in 32 bits), got %d x %d", fn, H, W);
    if (n < 0) return fail(h, RVDD_ERR_ARG, "%s: n must be >= 0, got %d", fn, n);
    return RVDD_OK;
}

int rvdd_unprocess(rvdd_t* h, const uint8_t* srgb, int32_t n, int32_t H, int32_t W, double rgb_gain, double red_gain, double blue_gain,
                   int32_t iso, int32_t pattern, const float* dither, const float* normal, uint64_t seed, int64_t frame0, float* lin_f32,
                   uint16_t* lin_u16, float* gt_raw, float* noisy, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (iso != 3200 && iso != 12800) return fail(h, RVDD_ERR_ARG, "rvdd_unprocess: iso must be 3200 or 12800, got %d", iso);
    if (pattern < RVDD_BAYER_GBRG || pattern > RVDD_BAYER_BGGR)
        return fail(h, RVDD_ERR_ARG, "rvdd_unprocess: pattern %d is not an rvdd_bayer (0 GBRG, 1 GRBG, 2 RGGB, 3 BGGR)", pattern);
    RC(unprocess_shape(h, "rvdd_unprocess", n, H, W));
    if (n == 0) return RVDD_OK;
    if (!srgb) return fail(h, RVDD_ERR_ARG, "rvdd_unprocess: srgb is required");
    if (!(rgb_gain != 0.0) || !(red_gain != 0.0) || !(blue_gain != 0.0)) return fail(h, RVDD_ERR_ARG, "rvdd_unprocess: zero gain (rgb_gain, red_gain, blue_gain)");
    ENTER(h);
    // generate_raw_from_RGB.py:77: float32 tensors -- (1 / red_gain, 1, 1 / blue_gain) / rgb_gain, each quotient rounded to f32
    const float rgb = (float)rgb_gain;
    const float g[3] = {(1.0f / (float)red_gain) / rgb, 1.0f / rgb, (1.0f / (float)blue_gain) / rgb};
    HIPCHK(h, launch_unprocess(srgb, n, H / 2, W / 2, g, iso, pattern, dither, normal, seed, frame0, lin_f32, lin_u16, gt_raw, noisy,
                               static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_unprocess_draws(rvdd_t* h, uint64_t seed, int64_t frame0, int32_t n, int32_t H, int32_t W, float* dither, float* normal,
                         void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(unprocess_shape(h, "rvdd_unprocess_draws", n, H, W));
    if (n == 0) return RVDD_OK;
    ENTER(h);
    HIPCHK(h, launch_unprocess_draws(seed, frame0, n, H / 2, W / 2, dither, normal, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_video_push(rvdd_t* h, const void* frames, int32_t dtype, int32_t layout, int32_t bit_depth, const uint8_t* ctl, float* out_rgb,
                    uint8_t* valid, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (dtype != RVDD_RAW_U16 && dtype != RVDD_RAW_F32) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: dtype must be 0 (u16) or 1 (f32), got %d", dtype);
    if (layout != RVDD_RAW_MOSAIC && layout != RVDD_RAW_PACKED_HWC)
        return fail(h, RVDD_ERR_ARG, "rvdd_video_push: layout must be 0 (mosaic) or 1 (packed HWC), got %d", layout);
    if (bit_depth < 1 || bit_depth > 16) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: bit_depth must be 1..16, got %d", bit_depth);
    if (!frames || !out_rgb || !valid) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: frames, out_rgb and valid are required");
    if (!h->finalized) return fail(h, RVDD_ERR_STATE, "rvdd_video_push: weights not finalized");
    const int B = h->cfg.batch, hh = h->cfg.height / 2, ww = h->cfg.width / 2, fut = h->cfg.future;
    const size_t hw = (size_t)hh * ww;
    auto& st = h->st;
    for (int b = 0; b < B; ++b)
        if (ctl && ctl[b] > RVDD_PUSH_IDLE) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: ctl[%d] = %d is not 0 (NEXT), 1 (FIRST) or 2 (IDLE)", b, ctl[b]);
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!st.packed) {      // the first push
        if (B > 64) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: needs batch <= 64, as the partial reset marks of rvdd_reset_slots do (batch is %d)", B);
        if (!h->opt.no_warp && (hh < 16 || ww < 16 || !tvl1_size_ok(ww, hh)))
            return fail(h, RVDD_ERR_ARG, "rvdd_video_push: raw frames of %d x %d cells are not a size rvdd_tvl1flow_batch accepts (at least 16 x 16 and not too "
                        "skinny for the flow's pyramid); only option no_warp streams this size", ww, hh);
        const int depth = 2 + fut, nd = 1 + fut;
        st.count.assign((size_t)B, 0);
        st.was_idle.assign((size_t)B, 0);
        st.dgray_ok.assign((size_t)B, 0);
        float *pk = nullptr, *gr = nullptr;
        RC(dmalloc(h, reinterpret_cast<void**>(&gr), (size_t)depth * B * hw * sizeof(float)));
        RC(dmalloc(h, reinterpret_cast<void**>(&st.I0), (size_t)nd * B * hw * sizeof(float)));
        RC(dmalloc(h, reinterpret_cast<void**>(&st.I1), (size_t)nd * B * hw * sizeof(float)));
        RC(dmalloc(h, reinterpret_cast<void**>(&st.u), (size_t)nd * B * 2 * hw * sizeof(float)));
        RC(dmalloc(h, reinterpret_cast<void**>(&st.flows), (size_t)nd * B * 2 * hw * sizeof(float)));
        RC(dmalloc(h, reinterpret_cast<void**>(&pk), (size_t)depth * B * 4 * hw * sizeof(float)));
        st.gray = gr;
        st.depth = depth;
        st.pushes = 0;
        st.packed = pk;      // last: the mark of a complete allocation
    }
    // option "stream_flow_from_denoised": the gray planes of the outputs, allocated by the first push that has it on
    const bool from_den = h->opt.stream_flow_from_denoised && !h->opt.no_warp;
    if (from_den && !st.dgray) RC(dmalloc(h, reinterpret_cast<void**>(&st.dgray), (size_t)B * hw * sizeof(float)));
    // the whole ctl is judged before anything changes
    for (int b = 0; b < B; ++b)
        if ((ctl ? ctl[b] : RVDD_PUSH_NEXT) == RVDD_PUSH_NEXT && st.count[(size_t)b] == 0)
            return st.was_idle[(size_t)b]
                       ? fail(h, RVDD_ERR_STATE, "rvdd_video_push: slot %d was idle on the last push: it goes on with FIRST or IDLE, not NEXT", b)
                       : fail(h, RVDD_ERR_STATE, "rvdd_video_push: slot %d has no video yet: its first frame is pushed with FIRST", b);
    // ingest: one launch per run of slots that get a frame
    const int pos = (int)(st.pushes % (uint64_t)st.depth);
    const size_t esz = dtype == RVDD_RAW_U16 ? 2 : 4;
    for (int b = 0; b < B;) {
        if (ctl && ctl[b] == RVDD_PUSH_IDLE) { ++b; continue; }
        int e = b + 1;
        while (e < B && !(ctl && ctl[e] == RVDD_PUSH_IDLE)) ++e;
        HIPCHK(h, launch_ingest_raw(static_cast<const char*>(frames) + (size_t)b * 4 * hw * esz, dtype, layout, e - b, hh, ww, bit_depth,
                                    st.packed + ((size_t)pos * B + b) * 4 * hw, st.gray + ((size_t)pos * B + b) * hw, s));
        b = e;
    }
    std::vector<int> ready, fresh;
    uint64_t den_slots = 0;      // ready slots whose previous push gave an output of the same video, its gray plane in dgray
    for (int b = 0; b < B; ++b) {
        const int c = ctl ? ctl[b] : RVDD_PUSH_NEXT;
        int& n = st.count[(size_t)b];
        n = c == RVDD_PUSH_IDLE ? 0 : c == RVDD_PUSH_FIRST ? 1 : (n < (1 << 30) ? n + 1 : n);
        st.was_idle[(size_t)b] = c == RVDD_PUSH_IDLE;
        valid[b] = n >= st.depth;
        if (n >= st.depth) ready.push_back(b);
        if (n == st.depth || (h->opt.stream_reset_each && n >= st.depth)) fresh.push_back(b);
        if (from_den && n > st.depth && st.dgray_ok[(size_t)b]) den_slots |= 1ull << b;
        st.dgray_ok[(size_t)b] = 0;
    }
    st.pushes++;
    if (ready.empty()) return RVDD_OK;
    const int nready = (int)ready.size();
    // ring positions: with a future frame the centre is the frame of the push before
    const int pc = (pos + st.depth - fut) % st.depth, pp = (pc + st.depth - 1) % st.depth;
    auto packed_at = [&](int p) { return st.packed + (size_t)p * B * 4 * hw; };
    auto gray_at = [&](int p) { return st.gray + (size_t)p * B * hw; };
    const float *flow_prev = nullptr, *flow_next = nullptr;
    if (!h->opt.no_warp) {
        HIPCHK(h, launch_stream_gather(gray_at(pc), gray_at(pp), fut ? gray_at(pos) : nullptr, st.dgray, den_slots, st.I0, st.I1, ready.data(), nready, B,
                                       (int64_t)hw, s));
        float* u = nready == B ? st.flows : st.u;      // every slot ready: the batch writes the step's flows itself
        RC(tvl1flow_batch(h, st.I0, st.I1, u, nready * (1 + fut), ww, hh, nullptr, stream, true));
        if (nready != B) HIPCHK(h, launch_stream_scatter(st.u, st.flows, ready.data(), nready, 1 + fut, B, (int64_t)hw, s));
        flow_prev = st.flows;
        flow_next = fut ? st.flows + (size_t)B * 2 * hw : nullptr;
    }
    if (!fresh.empty()) {
        std::vector<uint8_t> mask((size_t)B, 0);
        for (int b : fresh) mask[(size_t)b] = 1;
        RC(rvdd_reset_slots(h, mask.data()));
    }
    RC(rvdd_step_strided(h, packed_at(pp), packed_at(pc), fut ? packed_at(pos) : nullptr, flow_prev, flow_next, 0, 0, out_rgb, stream));
    if (from_den) {
        // the plane is taken from the output (with "prev_noisy_frame" lastden holds the noisy demosaic) inside the push that wrote it:
        // the caller may overwrite out_rgb before the next one
        HIPCHK(h, launch_gray_of_rgb(out_rgb, B, hh, ww, h->opt.bayer, bit_depth, st.dgray, s));
        for (int b : ready) st.dgray_ok[(size_t)b] = 1;
    }
    return RVDD_OK;
}

int rvdd_profile_enable(rvdd_t* h, int32_t on) {
    if (!h) return RVDD_ERR_ARG;
    ENTER(h);
    RC(prof_flush(h));
    if (on) for (auto& p : h->prof) { p.seen = p.launches = 0; p.ms = p.flops = p.bytes = 0; }
    h->prof_on = on != 0;
    return RVDD_OK;
}

int rvdd_profile_select(rvdd_t* h, const char* kernel_class, int32_t stride) {
    if (!h || stride < 1) return fail(h, RVDD_ERR_ARG, "rvdd_profile_select: bad argument");
    h->prof_filter = kernel_class ? kernel_class : "";
    h->prof_stride = stride;
    return RVDD_OK;
}

int rvdd_profile_count(const rvdd_t* h) { return h ? (int)h->prof.size() : 0; }

int rvdd_profile_read(rvdd_t* h, int32_t idx, char* name, int32_t name_cap, int64_t* launches,
                      double* total_ms, double* flops, double* bytes) {
    if (!h || idx < 0 || idx >= (int)h->prof.size()) return fail(h, RVDD_ERR_ARG, "rvdd_profile_read: bad index");
    ENTER(h);
    RC(prof_flush(h));
    const ProfClass& p = h->prof[idx];
    if (name && name_cap > 0) {
        std::strncpy(name, p.name.c_str(), name_cap - 1);
        name[name_cap - 1] = 0;
    }
    if (launches) *launches = p.launches;
    if (total_ms) *total_ms = p.ms;
    if (flops) *flops = p.flops;
    if (bytes) *bytes = p.bytes;
    return RVDD_OK;
}

int rvdd_debug_conv_bench(rvdd_t* h, int32_t variant, int32_t level, int32_t iters, float* ms, void* stream) {
    if (!h || !ms || level < 0 || level > 3 || iters < 1) return fail(h, RVDD_ERR_ARG, "rvdd_debug_conv_bench: bad argument");
    ENTER(h);
    if (!h->finalized || h->is_next()) return fail(h, RVDD_ERR_STATE, "rvdd_debug_conv_bench: needs a finalized convunet handle");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool was = h->prof_on;
    const int was_conv = h->opt.conv;
    h->prof_on = false;
    const Conv3& L = h->cu[CU_ENC1_1];
    ConvCall c;
    // variant 3 = Winograd kernel, 4 = split-f16 kernel (the direct one where the layer has no split bank, never one by size),
    // 0..2 = direct kernel variants
    h->opt.conv = variant == 3 ? CONV_WINO : variant == 4 && L.wh[c.src] ? CONV_SPLIT16 : CONV_DIRECT;
    c.variant = variant >= 3 ? 0 : variant;
    c.in = h->lv[level].t[0]; c.out = h->lv[level].t[1]; c.H = h->lv[level].H; c.W = h->lv[level].W; c.epi = EPI_RELU;
    NetRun run;
    run.n = h->cfg.batch;
    const Sub all{0, run.n};
    int rc = run_conv(h, run, L, c, s, all);   // warm-up (also sets the function attribute)
    if (rc == RVDD_OK) {
        (void)hipEventRecord(h->t0, s);
        for (int i = 0; i < iters && rc == RVDD_OK; ++i) rc = run_conv(h, run, L, c, s, all);
        (void)hipEventRecord(h->t1, s);
        (void)hipEventSynchronize(h->t1);
        float t = 0.f;
        (void)hipEventElapsedTime(&t, h->t0, h->t1);
        *ms = t / iters;
    }
    h->prof_on = was;
    h->opt.conv = was_conv;
    return rc;
}

int rvdd_timer_start(rvdd_t* h, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    ENTER(h);
    HIPCHK(h, hipEventRecord(h->t0, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_timer_stop_ms(rvdd_t* h, void* stream, float* ms) {
    if (!h || !ms) return RVDD_ERR_ARG;
    ENTER(h);
    HIPCHK(h, hipEventRecord(h->t1, static_cast<hipStream_t>(stream)));
    HIPCHK(h, hipEventSynchronize(h->t1));
    HIPCHK(h, hipEventElapsedTime(ms, h->t0, h->t1));
    return RVDD_OK;
}

}  // extern "C"
