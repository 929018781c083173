// rvdd_video_push: raw frames in, denoised frames out -- ring, control, ingest, flows and the step of every slot that has its frames.  The
// stages between the ingest and the output are stages.hip's.
#include "runtime_internal.h"

extern "C" int rvdd_video_push(rvdd_t* h, const void* frames, int32_t dtype, int32_t layout, int32_t bit_depth, const uint8_t* ctl, float* out_rgb,
                    uint8_t* valid, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (dtype != RVDD_RAW_U16 && dtype != RVDD_RAW_F32) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: dtype must be 0 (u16) or 1 (f32), got %d", dtype);
    if (layout != RVDD_RAW_MOSAIC && layout != RVDD_RAW_PACKED_HWC)
        return fail(h, RVDD_ERR_ARG, "rvdd_video_push: layout must be 0 (mosaic) or 1 (packed HWC), got %d", layout);
    RC(need_bit_depth(h, "rvdd_video_push", bit_depth));
    if (!frames || !out_rgb || !valid) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: frames, out_rgb and valid are required");
    const int B = h->cfg.batch, hh = h->cfg.height / 2, ww = h->cfg.width / 2, fut = h->cfg.future;
    // option "stream_container": the frames are packed bits, order container - 1 of enum rvdd_bits_order
    const int container = h->opt.stream_container;
    if (container) {
        if (dtype != RVDD_RAW_U16) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with option stream_container dtype must be 0 (u16: the samples' type), got %d", dtype);
        if (layout != RVDD_RAW_MOSAIC) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with option stream_container layout must be 0 (mosaic), got %d", layout);
        if (bit_depth != 10 && bit_depth != 12 && bit_depth != 14)
            return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with option stream_container bit_depth must be 10, 12 or 14, got %d", bit_depth);
        if (container - 1 == RVDD_BITS_MIPI && bit_depth != 12 && (ww & 1))
            return fail(h, RVDD_ERR_ARG, "rvdd_video_push: ww must be even for MIPI RAW%d (groups of four pixels), got ww = %d", bit_depth, ww);
    }
    if (!h->finalized) return fail(h, RVDD_ERR_STATE, "rvdd_video_push: weights not finalized");
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
        st.head.assign((size_t)B, 0);
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
    RC(stages_fit(h, hh, ww));      // the stages between the ingest and the output (stages.hip): each fits these frames as it is set, or refuses them
    // the whole ctl is judged before anything changes
    for (int b = 0; b < B; ++b)
        if ((ctl ? ctl[b] : RVDD_PUSH_NEXT) == RVDD_PUSH_NEXT && st.count[(size_t)b] == 0)
            return st.was_idle[(size_t)b]
                       ? fail(h, RVDD_ERR_STATE, "rvdd_video_push: slot %d was idle on the last push: it goes on with FIRST or IDLE, not NEXT", b)
                       : fail(h, RVDD_ERR_STATE, "rvdd_video_push: slot %d has no video yet: its first frame is pushed with FIRST", b);
    // ingest: one launch per run of slots that get a frame
    const int pos = (int)(st.pushes % (uint64_t)st.depth);
    const size_t esz = dtype == RVDD_RAW_U16 ? 2 : 4;
    const size_t frame_bytes = container ? 2 * (size_t)hh * (size_t)bits_row_bytes(ww, bit_depth) : 0;
    RC(for_each_run(B, [&](int b) { return !(ctl && ctl[b] == RVDD_PUSH_IDLE); }, [&](int b, int e) -> int {
        float* ring_packed = st.packed + ((size_t)pos * B + b) * 4 * hw;
        float* ring_gray = st.gray + ((size_t)pos * B + b) * hw;
        float* packed = h->dpc.on ? h->dpc.in + (size_t)b * 4 * hw : ring_packed;      // rvdd_set_dpc corrects from beside the ring into it
        if (container)
            HIPCHK(h, launch_ingest_bits(static_cast<const uint8_t*>(frames) + (size_t)b * frame_bytes, container - 1, e - b, hh, ww, bit_depth,
                                         packed, ring_gray, s));
        else
            HIPCHK(h, launch_ingest_raw(static_cast<const char*>(frames) + (size_t)b * 4 * hw * esz, dtype, layout, e - b, hh, ww, bit_depth,
                                        packed, ring_gray, s));
        if (h->dmap.on && h->dmap.ncells)
            HIPCHK(h, launch_dpc_map_apply(packed, ring_gray, e - b, hh, ww, bit_depth, h->dmap.mask, h->dmap.cells, h->dmap.ncells, s));
        if (h->dpc.on) HIPCHK(h, launch_dpc(packed, ring_packed, ring_gray, e - b, hh, ww, bit_depth, h->dpc.p, h->dpc.counts + 2 * (size_t)b, s));
        if (h->cols.on) RC(run_cols_apply(h, ring_packed, ring_gray, h->cols.map, e - b, hh, ww, bit_depth, s));
        RC(rows_run(h, ring_packed, ring_gray, b, e, hh, ww, bit_depth, s));
        if (h->geq.on)
            RC(run_green_apply(h, ring_packed, ring_gray, h->geq.map, h->geq.gh, h->geq.gw, h->geq.black, e - b, hh, ww, bit_depth, h->opt.bayer, s));
        // the gray planes stay the sensor's: TV-L1 matches what it always matched
        if (h->match.on) HIPCHK(h, launch_match(ring_packed, ring_packed, (int64_t)(e - b) * 4 * (int64_t)hw, h->match.cfg.scale, h->match.cfg.offset, false, s));
        return RVDD_OK;
    }));
    // Per slot: which frame of its video this push outputs (centre; -1: none).  The plain rule is centre = n - 1 - future >= 1.  Option
    // "stream_all_frames" adds the HEAD, centre 0 -- frame 0 stands in for the missing previous frame, the flow towards it is zero by
    // definition -- and, with a future frame, the TAIL: an IDLE straight after the video's last frame outputs that frame, centre n - 1,
    // with itself as the next frame and a zero flow towards it.  The substituted frames lie in the slot's own ring positions (dup).
    const bool all_frames = h->opt.stream_all_frames;
    std::vector<int> ready, fresh, dup, centre((size_t)B, -1);
    std::vector<uint8_t> pairs, next_pairs;      // slot | direction << 6 of every TV-L1 pair: the pairs towards the previous frames first
    uint64_t den_slots = 0;      // slots whose pair towards the previous frame is matched against the previous output, its gray plane in dgray
    uint64_t tails = 0;
    for (int b = 0; b < B; ++b) {
        const int c = ctl ? ctl[b] : RVDD_PUSH_NEXT;
        int& n = st.count[(size_t)b];
        // a tail needs the frame in front of the centre in the ring: frame n - 2, or the copy a FIRST under the option left
        const bool tail = all_frames && fut && c == RVDD_PUSH_IDLE && n >= 1 && (n >= 2 || st.head[(size_t)b]);
        int& ctr = centre[(size_t)b];
        if (tail) {
            ctr = n - 1;
            tails |= 1ull << b;
            dup.push_back(b);
        } else {
            n = c == RVDD_PUSH_IDLE ? 0 : c == RVDD_PUSH_FIRST ? 1 : (n < (1 << 30) ? n + 1 : n);
            if (c == RVDD_PUSH_FIRST) {
                st.head[(size_t)b] = all_frames;
                if (all_frames) dup.push_back(b);
            }
            if (c != RVDD_PUSH_IDLE) ctr = n - 1 - fut;
            if (ctr < 0 || (ctr == 0 && !(all_frames && st.head[(size_t)b]))) ctr = -1;
        }
        st.was_idle[(size_t)b] = c == RVDD_PUSH_IDLE;
        valid[b] = ctr >= 0;
        if (ctr >= 0) {
            ready.push_back(b);
            if (ctr <= 1 || h->opt.stream_reset_each) fresh.push_back(b);
            if (ctr >= 1) pairs.push_back((uint8_t)b);
            if (fut && !tail) next_pairs.push_back((uint8_t)(64 | b));
            if (from_den && ctr >= 2 && st.dgray_ok[(size_t)b]) den_slots |= 1ull << b;
        }
        st.dgray_ok[(size_t)b] = 0;
        if (tail) n = 0;      // idle from here on, as after any IDLE
    }
    st.pushes++;
    auto packed_at = [&](int p) { return st.packed + (size_t)p * B * 4 * hw; };
    auto gray_at = [&](int p) { return st.gray + (size_t)p * B * hw; };
    if (!dup.empty())
        HIPCHK(h, launch_stream_dup(packed_at((pos + st.depth - 1) % st.depth), packed_at(pos), dup.data(), (int)dup.size(), tails, B, (int64_t)hw, s));
    if (ready.empty()) return RVDD_OK;
    // ring positions: with a future frame the centre is the frame of the push before
    const int pc = (pos + st.depth - fut) % st.depth, pp = (pc + st.depth - 1) % st.depth;
    const float *flow_prev = nullptr, *flow_next = nullptr;
    if (!h->opt.no_warp) {
        pairs.insert(pairs.end(), next_pairs.begin(), next_pairs.end());
        const int npairs = (int)pairs.size();
        const bool whole = npairs == B * (1 + fut);      // every slot has every pair: the batch writes the step's flows itself
        if (npairs) {
            HIPCHK(h, launch_stream_gather(gray_at(pc), gray_at(pp), fut ? gray_at(pos) : nullptr, st.dgray, den_slots, st.I0, st.I1, pairs.data(), npairs, B,
                                           (int64_t)hw, s));
            RC(tvl1flow_batch(h, st.I0, st.I1, whole ? st.flows : st.u, npairs, ww, hh, nullptr, stream, true));
        }
        if (!whole) HIPCHK(h, launch_stream_scatter(st.u, st.flows, pairs.data(), npairs, 1 + fut, B, (int64_t)hw, s));
        flow_prev = st.flows;
        flow_next = fut ? st.flows + (size_t)B * 2 * hw : nullptr;
    }
    if (!fresh.empty()) {
        std::vector<uint8_t> mask((size_t)B, 0);
        for (int b : fresh) mask[(size_t)b] = 1;
        RC(rvdd_reset_slots(h, mask.data()));
    }
    RC(rvdd_step_strided(h, packed_at(pp), packed_at(pc), fut ? packed_at(pos) : nullptr, flow_prev, flow_next, 0, 0, out_rgb, stream));
    // rvdd_set_resid: the centre frames as the step read them against the outputs as it wrote them, before the way back: with the match
    // on both are in the network's domain, whose unit is the 12-bit DN of the checkpoint's curve
    if (h->resid.on)
        RC(for_each_run(B, [&](int b) { return centre[(size_t)b] >= 0; }, [&](int b, int e) -> int {
            HIPCHK(h, launch_resid(packed_at(pc) + (size_t)b * 4 * hw, out_rgb + (size_t)b * 12 * hw, e - b, hh, ww, h->opt.bayer,
                                   h->match.on ? 12 : bit_depth, h->resid.acc + b, s));
            return RVDD_OK;
        }));
    // every slot, ready or not: one launch; the recurrent state stays in the network's own domain
    if (h->match.on) HIPCHK(h, launch_match(out_rgb, out_rgb, (int64_t)B * 12 * (int64_t)hw, h->match.cfg.scale, h->match.cfg.offset, true, s));
    if (from_den) {
        // the plane is taken from the output (with "prev_noisy_frame" lastden holds the noisy demosaic) inside the push that wrote it:
        // the caller may overwrite out_rgb before the next one
        HIPCHK(h, launch_gray_of_rgb(out_rgb, B, hh, ww, h->opt.bayer, bit_depth, st.dgray, s));
        for (int b : ready) st.dgray_ok[(size_t)b] = centre[(size_t)b] >= 1 && st.count[(size_t)b] > 0;      // not a head's, not a tail's
    }
    return RVDD_OK;
}
