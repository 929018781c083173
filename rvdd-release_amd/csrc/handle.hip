// The handle: creation and destruction, device memory, the option table, weight staging and the reset marks.
#include "runtime_internal.h"

namespace {

thread_local std::string g_create_error;

#define CONV_KERNEL_RANGE "rvdd_set_option: conv_kernel must be 0 (default), 1 (direct f32), 2 (winograd f32) or 4 (f32 by size)"

// The one decoder of the conv selector: option "conv_kernel"'s integer (word == nullptr; -1: not a selector), or RVDD_CONV's
// word -- direct | winograd | f32, anything else = the default.
int conv_decode(const char* word, int32_t value) {
    static const struct { int sel; const char* word; } known[] = {
        {CONV_SPLIT16, nullptr}, {CONV_DIRECT, "direct"}, {CONV_WINO, "winograd"}, {CONV_F32, "f32"}};
    for (const auto& k : known)
        if (word ? (k.word && std::strcmp(word, k.word) == 0) : value == k.sel) return k.sel;
    return word ? CONV_SPLIT16 : -1;
}

void drop_graphs(rvdd_t* h) {
    for (auto& kv : h->graphs) {
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    }
    h->graphs.clear();
}

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

// One row per option: ABI name | environment variable read at rvdd_create (nullptr: none) | field of Options | accepted range
// lo .. hi | message of a value outside it (nullptr: a flag, any value counts as value != 0) | hook that does the storing itself
// (nullptr: plain store).  F is the first row, X every other: the table and the unknown-option message expand this one list.
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
    X("warp48_pairs", nullptr, warp48_pairs, 0, 1, nullptr, nullptr)                                                             \
    X("bayer_pattern", nullptr, bayer, RVDD_BAYER_GBRG, RVDD_BAYER_BGGR,                                                         \
      "rvdd_set_option: bayer_pattern must be 0 (GBRG), 1 (GRBG), 2 (RGGB) or 3 (BGGR)", nullptr)                                \
    X("stream_reset_each", nullptr, stream_reset_each, 0, 1, nullptr, nullptr)                                                   \
    X("stream_flow_from_denoised", nullptr, stream_flow_from_denoised, 0, 1, nullptr, nullptr)                                   \
    X("stream_all_frames", nullptr, stream_all_frames, 0, 1, nullptr, nullptr)                                                   \
    X("stream_container", nullptr, stream_container, 0, 2,                                                                       \
      "rvdd_set_option: stream_container must be 0 (one number per sample), 1 (MIPI CSI-2) or 2 (MSB first)", nullptr)
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

// range check, then the row's hook or a plain store
int set_option_row(rvdd_t* h, const OptRow& row, int32_t value) {
    if (!row.range_msg) value = value != 0;
    else if (value < row.lo || value > row.hi) return fail(h, RVDD_ERR_ARG, "%s", row.range_msg);
    if (row.hook) return row.hook(h, value);
    h->opt.*row.field = value;
    return RVDD_OK;
}

// ---- expected state_dict -------------------
struct KeySpec {
    std::string key;
    std::vector<int64_t> shape;
};

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

}  // namespace

int fail(rvdd_t* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

int dmalloc(rvdd_t* h, void** p, size_t bytes, bool zero) {
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

// rvdd_psnr_l1[_batch]: partial sums and results of every slice; rvdd_create allocates one slice's worth, more grows on demand
int ensure_loss_batch(rvdd_t* h, size_t doubles) {
    if (h->loss_batch_cap >= doubles) return RVDD_OK;
    if (h->loss_batch) {
        HIPCHK(h, hipDeviceSynchronize());
        HIPCHK(h, hipFree(h->loss_batch));
        h->loss_batch = nullptr;
        h->loss_batch_cap = 0;
    }
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&h->loss_batch), doubles * sizeof(double)));
    h->loss_batch_cap = doubles;
    return RVDD_OK;
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

std::vector<std::string> convunet_conv_names(bool feat) {
    std::vector<std::string> n;
    for (int i = feat ? 0 : 1; i < CU_COUNT; ++i) n.push_back(kCuNames[i]);
    return n;
}

int next_proj_cin(const rvdd_t* h, const std::string& blk) {
    const bool feat = h->has_feat();
    if (blk == "preprocessing_layer.blocks.0") return h->cin_real();
    if (blk == "encoder_convs.0.blocks.0") return feat ? 96 : h->cin_real();
    if (blk.rfind("decoder_convs.", 0) == 0 && blk.find(".blocks.0") != std::string::npos) return 96;
    return 0;
}

extern "C" {

const char* rvdd_version(void) { return "rvdd-hip 0.1 (gfx950)"; }

const char* rvdd_last_error(const rvdd_t* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

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
        if (!h->is_next()) A(&h->lv[l].part, n);      // the two-source convs and the composed first layer of the convunet
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
    if (rc == RVDD_OK) rc = ensure_loss_batch(h, 2 * 1024 + 2);      // one slice: a single-sequence caller never grows it
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
    stages_free(h);
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
    RC(h->is_next() ? finalize_convnext(h) : finalize_convunet(h));
    h->staged.clear();
    h->finalized = true;
    return RVDD_OK;
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
