// A frame-step of the recurrent denoise+demosaic path (models/recurrent_model.py:105-135 set_input, :161-349 forward, test
// branch): the stages in front of the net, the net, the graph cache, the recurrent state and its slots.
#include "runtime_internal.h"

namespace {

// The network-input stage in front of the net for sequences [sb.b0, sb.b0 + sb.nb): one launch covers them all -- the kernels take
// the caller's batch strides (channel slices of the reference's wider `n` / `flow` tensors are strided over the batch).
int prologue_netin(rvdd_t* h, NetRun& run, Sub sb, hipStream_t s) {
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
            return RVDD_OK;
        }
        // larger ones: the bound (and the zeroing) in its own small launch, the green plane and the network input tiled
        const bool tiled = !h->is_next() && !h->opt.prev_noisy && netin_tiled_applies(H / 2, W / 2, h->cfg.future != 0, h->opt.small_prestage);
        if (amax_netin) {
            // (block floating point) a bound of max |netin| from the raw frames and from the words PostConvs wrote last step;
            // with --prev_noisy_frame the "previous output" is a demosaicked frame whose raw data is gone: its own maximum
            const float* rp_ = in.raw_prev ? in.raw_prev + o * in.rawf : nullptr;
            HIPCHK(h, launch_netin_bound(rc_, rn_, rp_, n, H / 2, W / 2, (int64_t)in.rawf,
                                         latch == ~0ull ? nullptr : amax_words(h, run.amax.feat_in, o), amax_netin, s,
                                         zero_now ? zero_a : nullptr, zero_na, zero_now ? zero_b : nullptr, zero_nb, latch));
            if (h->opt.prev_noisy && latch != ~0ull)      // over the runs of sequences that continue a video (one run without a reset)
                RC(for_each_run(n, [&](int b) { return !((latch >> b) & 1ull); }, [&](int b, int e) -> int {
                    HIPCHK(h, launch_amax_reduce(h->lastden4 + (o + b) * img * 4, e - b, (int64_t)img * 4, amax_netin + (size_t)b * kAmaxSeqWords, s, 1));
                    return RVDD_OK;
                }));
        }
        // ConvNeXtUnet: the input's only reader is the 1x1 projection of the first ConvBlock, which rides in the same kernel
        const NextBlk* first = h->is_next() && h->opt.next_projfuse ? &h->nx[h->has_feat() ? NX_PRE : NX_ENC0_0] : nullptr;
        run.netin_proj = first != nullptr;
        if (tiled) {
            HIPCHK(h, launch_netin_small(rc_, nullptr, h->lastden4 + o * img * 4, fp_, netin, n, H / 2, W / 2, (int64_t)in.rawf, (int64_t)in.flowf,
                                         nullptr, nullptr, s, nullptr, 0, nullptr, 0, latch, h->opt.bayer));
            return RVDD_OK;
        }
        HIPCHK(h, launch_netin(rc_, green, h->lastden4 + o * img * 4, fp_, next4, fn_, netin, n, H / 2, W / 2, s, (int64_t)in.rawf,
                               (int64_t)in.flowf, first ? first->w.proj_w : nullptr, first ? first->w.proj_b : nullptr,
                               first ? h->lv[0].t[0] + o * img * kF : nullptr, h->opt.bayer));
    }
    return RVDD_OK;
}

// The feature warp of the same sequences (feature recurrence, unless --no_warp)
int prologue_features(rvdd_t* h, NetRun& run, Sub sb, hipStream_t s) {
    if (!h->has_feat() || h->opt.no_warp || run.zero_feat) return RVDD_OK;
    const int H = h->cfg.height, W = h->cfg.width, n = sb.nb;
    const size_t img = (size_t)H * W, o = (size_t)sb.b0;
    const StepInputs& in = *run.in;
    const float* fp_ = in.flow_prev ? in.flow_prev + o * in.flowf : nullptr;
    run.featw_proj = next_pf_pre(h);
    Scope sc(h, s, "warp48_kernel", run.featw_proj ? 2.0 * 48 * 48 * n * img : 0.0, (double)n * img * (384.0 + 2.0));
    if (run.featw_proj)
        HIPCHK(h, launch_warp48_proj(h->lastfeat + o * img * kF, fp_, h->featw + o * img * kF, n, H, W, h->nx[NX_ENC0_0].half[1].frag,
                                     h->nx[NX_ENC0_0].half[1].inv_e, h->nx[NX_ENC0_0].w.proj_b, s, (int64_t)in.flowf));
    else
        HIPCHK(h, launch_warp48(h->lastfeat + o * img * kF, fp_, h->featw + o * img * kF, n, H, W, s, (int64_t)in.flowf, h->opt.warp48_pairs));
    return RVDD_OK;
}

int run_net(rvdd_t* h, NetRun& run, const float* netin, const float* featw, float* feat_dst, float* out_nchw,
            float* out_nhwc4, hipStream_t s) {
    if (!h->is_next()) return run_convunet(h, run, netin, featw, feat_dst, out_nchw, out_nhwc4, s);
    if (run.in) RC(run_prologue(h, run, Sub{0, run.n}, s));
    return run_convnext(h, run, netin, featw, feat_dst, out_nchw, out_nhwc4, s);
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
    // every covered slot starts a video and the first layer is the composed one: the features are zero, and instead of a map of
    // zeros written, warped and convolved (a memset of 1.4 GB at 720p B = 8, warp48_kernel over it, the second pass of
    // EncoderConvs[0][0] over the result: +0 added to every partial sum) run_convunet applies the layer's ReLU to the partial sums
    run.zero_feat = init && !nw && pre5_fused(h);
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
        // (zero_feat: the features have no reader in this step, and PostConvs[0] writes the whole map at its end)
        if (h->has_feat() && !run.zero_feat) HIPCHK(h, hipMemsetAsync(h->lastfeat, 0, npix * kF * sizeof(float), s));
    } else if (pend) {
        // some sequences start a video (rvdd_reset_slots): the same latch for them alone -- the demosaic over each run of
        // them, then ONE launch that zeroes their features and their words in every set (the rotation of the sets by step_ctr
        // is harmless only because a latched sequence has all of them zeroed)
        const size_t img = (size_t)H * W;
        RC(for_each_run(B, [&](int b) { return (pend >> b) & 1u; }, [&](int b, int e) -> int {
            HIPCHK(h, launch_demosaic(raw_prev + b * in.rawf, h->green + b * img, h->lastden4 + b * img * 4, e - b, H / 2, W / 2,
                                      (int64_t)H * W * 4, 4, 1, s, (int64_t)in.rawf, h->opt.bayer));
            return RVDD_OK;
        }));
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

// What a frame-step does in front of the net, for the sequences of `sb`: run_convunet calls it per sequence when the
// full-resolution stages run depth first.
int run_prologue(rvdd_t* h, NetRun& run, Sub sb, hipStream_t s) {
    RC(prologue_netin(h, run, sb, s));
    return prologue_features(h, run, sb, s);
}

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

}  // extern "C"
