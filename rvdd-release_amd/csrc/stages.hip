// The state of the stages of rvdd_video_push between its ingest and its output -- map, dpc, cols, rows, green, match, resid, in the push's
// order: their setters and readers, the launches that sit inside a profile class, and the push's one question whether its frames fit them.
#include "runtime_internal.h"

namespace {
// A device map the caller supplied from the host (dmap.mask, dmap.cells, cols.map, geq.map): the setter that replaces it synchronises
// first -- pushes in flight read the map they were enqueued with -- then drops the old copy, and uploads the new one if there is one.
template <class T>
int map_drop(rvdd_t* h, T*& dev) {
    if (dev) HIPCHK(h, hipFree(dev));
    dev = nullptr;
    return RVDD_OK;
}
template <class T>
int map_upload(rvdd_t* h, T*& dev, const T* host, size_t count) {
    HIPCHK(h, hipMalloc(reinterpret_cast<void**>(&dev), count * sizeof(T)));
    HIPCHK(h, hipMemcpy(dev, host, count * sizeof(T), hipMemcpyHostToDevice));
    return RVDD_OK;
}

// One accumulator per slot (rows.acc, resid.acc), allocated by the first push that has its stage on.  rvdd_set_rows / rvdd_set_resid behind
// their checks: the device synchronised -- pushes in flight keep what they were enqueued with, the accumulators must be at rest -- and a
// stage switched on starts from zero.
template <class Acc>
int acc_switch(rvdd_t* h, bool on, bool& stage_on, Acc* acc) {
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());
    if (on && !stage_on && acc) HIPCHK(h, hipMemset(acc, 0, (size_t)h->cfg.batch * sizeof(Acc)));
    stage_on = on;
    return RVDD_OK;
}
// rvdd_rows_read / rvdd_resid_read as `fn`: the slot's accumulator copied out and zeroed, in stream order; zeros where no push has run the stage
template <class Acc>
int acc_read(rvdd_t* h, const char* fn, Acc* acc, int32_t slot, Acc* host_out, void* stream) {
    RC(need_ptr(h, fn, host_out, "host_out"));
    if (slot < 0 || slot >= h->cfg.batch) return fail(h, RVDD_ERR_ARG, "%s: slot must be 0 .. %d, got %d", fn, h->cfg.batch - 1, slot);
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (acc) {
        HIPCHK(h, hipMemcpyAsync(host_out, acc + slot, sizeof(Acc), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemsetAsync(acc + slot, 0, sizeof(Acc), s));
    } else {
        std::memset(host_out, 0, sizeof(Acc));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    return RVDD_OK;
}
}  // namespace

void stages_free(rvdd_t* h) {
    for (void* p : {(void*)h->dmap.mask, (void*)h->dmap.cells, (void*)h->cols.map, (void*)h->geq.map})
        if (p) (void)hipFree(p);
}

// ---- map (rvdd_set_dpc_map): the frames just ingested are corrected by the static defect map in place, in front of rvdd_set_dpc's rule
extern "C" int rvdd_set_dpc_map(rvdd_t* h, const uint8_t* cellmask, int32_t hh, int32_t ww) {
    const char* fn = "rvdd_set_dpc_map";
    if (!h) return RVDD_ERR_ARG;
    std::vector<int> cells;
    if (cellmask) {
        RC(need_min(h, fn, "hh", hh, 3, "the second ring is reflected about the edge"));
        RC(need_min(h, fn, "ww", ww, 3, "the second ring is reflected about the edge"));
        if ((int64_t)hh * ww > 0x7fffffffll) return fail(h, RVDD_ERR_ARG, "rvdd_set_dpc_map: hh * ww = %d * %d must be below 2^31 (cell indices are 32-bit)", hh, ww);
        const size_t hw = (size_t)hh * ww;
        for (size_t i = 0; i < hw; ++i) {
            if (cellmask[i] & 0xf0u)
                return fail(h, RVDD_ERR_ARG, "rvdd_set_dpc_map: cellmask[%d][%d] = 0x%02x has a bit above the four planes' set", (int)(i / ww), (int)(i % ww),
                            cellmask[i]);
            if (cellmask[i]) cells.push_back((int)i);
        }
    }
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());
    auto& m = h->dmap;
    RC(map_drop(h, m.mask));
    RC(map_drop(h, m.cells));
    m.on = false;
    m.ncells = 0;
    if (!cellmask) return RVDD_OK;
    if (!cells.empty()) {                   // an empty map is valid and owns nothing
        RC(map_upload(h, m.mask, cellmask, (size_t)hh * ww));
        RC(map_upload<int>(h, m.cells, cells.data(), cells.size()));
    }
    m.hh = hh;
    m.ww = ww;
    m.ncells = (int64_t)cells.size();
    m.on = true;
    return RVDD_OK;
}

// ---- dpc (rvdd_set_dpc): the packed planes are ingested beside the ring (dpc.in) and corrected into it
extern "C" int rvdd_set_dpc(rvdd_t* h, const rvdd_dpc_cfg* cfg) {
    if (!h) return RVDD_ERR_ARG;
    DpcParams p{};
    if (cfg) RC(dpc_params(h, "rvdd_set_dpc", cfg, &p));
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());      // pushes in flight keep the parameters they were enqueued with anyway; the counters must be at rest
    auto& dpc = h->dpc;
    if (cfg && !dpc.on) {                   // switched on: the totals start again
        dpc.total.assign((size_t)h->cfg.batch * 2, 0);
        if (dpc.counts) HIPCHK(h, hipMemset(dpc.counts, 0, (size_t)h->cfg.batch * 2 * sizeof(unsigned)));
    }
    dpc.on = cfg != nullptr;
    if (cfg) dpc.p = p;
    return RVDD_OK;
}

// unlike the slot readers: what the device counted since the last call is folded into the totals, which are what the caller gets
extern "C" int rvdd_dpc_counts(rvdd_t* h, uint64_t* hot_dead, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_ptr(h, "rvdd_dpc_counts", hot_dead, "hot_dead"));
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto& dpc = h->dpc;
    const size_t n = (size_t)h->cfg.batch * 2;
    dpc.total.resize(n, 0);
    if (dpc.counts) {
        std::vector<unsigned> got(n, 0);
        HIPCHK(h, hipMemcpyAsync(got.data(), dpc.counts, n * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemsetAsync(dpc.counts, 0, n * sizeof(unsigned), s));
        HIPCHK(h, hipStreamSynchronize(s));
        for (size_t i = 0; i < n; ++i) dpc.total[i] += got[i];
    } else {
        HIPCHK(h, hipStreamSynchronize(s));
    }
    for (size_t i = 0; i < n; ++i) hot_dead[i] = dpc.total[i];
    return RVDD_OK;
}

// ---- cols (rvdd_set_cols): the static column offsets taken out of the ring's planes and gray planes in place; nothing is allocated by a push
extern "C" int rvdd_set_cols(rvdd_t* h, const float* map_host, int32_t ww) {
    if (!h) return RVDD_ERR_ARG;
    if (map_host) {
        RC(need_min(h, "rvdd_set_cols", "ww", ww, 5));
        for (int64_t i = 0; i < 2 * (int64_t)ww; ++i)
            if (!std::isfinite(map_host[i]))
                return fail(h, RVDD_ERR_ARG, "rvdd_set_cols: map_host[%d][%d] = %g is not finite", (int)(i / ww), (int)(i % ww), (double)map_host[i]);
    }
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());
    auto& c = h->cols;
    RC(map_drop(h, c.map));
    c.on = false;
    c.ww = 0;
    if (!map_host) return RVDD_OK;
    RC(map_upload(h, c.map, map_host, 2 * (size_t)ww));
    c.ww = ww;
    c.on = true;
    return RVDD_OK;
}

int run_cols_apply(rvdd_t* h, float* packed, float* gray, const float* map_dev, int n, int hh, int ww, int bit_depth, hipStream_t s) {
    const double cells = (double)n * 4.0 * hh * ww;
    Scope sc(h, s, "cols_apply_kernel", 0.0, cells * 8.0 + cells * 2.0);
    HIPCHK(h, launch_cols_apply(packed, gray, map_dev, n, hh, ww, bit_depth, s));
    return RVDD_OK;
}

// ---- rows (rvdd_set_rows): the row offsets of the (corrected) frames estimated and taken out of the ring's planes and gray planes in place
extern "C" int rvdd_set_rows(rvdd_t* h, const rvdd_rows_cfg* cfg) {
    if (!h) return RVDD_ERR_ARG;
    RowsParams p{};
    if (cfg) RC(rows_params(h, "rvdd_set_rows", cfg, &p));
    RC(acc_switch(h, cfg != nullptr, h->rows.on, h->rows.acc));
    if (cfg) h->rows.p = p;
    return RVDD_OK;
}

extern "C" int rvdd_rows_read(rvdd_t* h, int32_t slot, rvdd_rows_acc* host_out, void* stream) {
    return h ? acc_read(h, "rvdd_rows_read", h->rows.acc, slot, host_out, stream) : RVDD_ERR_ARG;
}

int rows_run(rvdd_t* h, float* packed, float* gray, int b, int e, int hh, int ww, int bit_depth, hipStream_t s) {
    const auto& rows = h->rows;
    if (!rows.on) return RVDD_OK;
    const double cells = (double)(e - b) * 4.0 * (double)hh * ww;
    float* offsets = rows.offsets + (size_t)b * 2 * hh;
    {
        Scope sc(h, s, "rows_estimate_kernel", 0.0, cells * 4.0);
        HIPCHK(h, launch_rows_estimate(packed, e - b, hh, ww, bit_depth, rows.p, offsets, rows.state + (size_t)b * 2 * hh, rows.acc + b, s));
    }
    Scope sc(h, s, "rows_apply_kernel", 0.0, cells * 8.0 + cells * 2.0);
    HIPCHK(h, launch_rows_apply(packed, gray, offsets, e - b, hh, ww, bit_depth, s));
    return RVDD_OK;
}

// ---- green (rvdd_set_green): the static map of green gains taken out of the ring's two green planes and gray planes in place; nothing is
// allocated by a push
extern "C" int rvdd_set_green(rvdd_t* h, const float* map_host, int32_t gh, int32_t gw, float black) {
    const char* fn = "rvdd_set_green";
    if (!h) return RVDD_ERR_ARG;
    if (map_host) {
        RC(need_min(h, fn, "gh", gh, 1));
        RC(need_min(h, fn, "gw", gw, 1));
        if (!std::isfinite(black)) return fail(h, RVDD_ERR_ARG, "rvdd_set_green: black must be finite, got %g", (double)black);
        for (int64_t i = 0; i < (int64_t)gh * gw; ++i)
            if (!std::isfinite(map_host[i]))
                return fail(h, RVDD_ERR_ARG, "rvdd_set_green: map_host[%d][%d] = %g is not finite", (int)(i / gw), (int)(i % gw), (double)map_host[i]);
    }
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());
    auto& g = h->geq;
    RC(map_drop(h, g.map));
    g.on = false;
    g.gh = g.gw = 0;
    if (!map_host) return RVDD_OK;
    RC(map_upload(h, g.map, map_host, (size_t)gh * (size_t)gw));
    g.gh = gh;
    g.gw = gw;
    g.black = black;
    g.on = true;
    return RVDD_OK;
}

int run_green_apply(rvdd_t* h, float* packed, float* gray, const float* map_dev, int gh, int gw, float black, int n, int hh, int ww, int bit_depth,
                    int bayer, hipStream_t s) {
    const double cells = (double)n * hh * ww;                       // two planes read and written, two read, the gray plane written
    Scope sc(h, s, "green_apply_kernel", 0.0, cells * 4.0 * (gray ? 7.0 : 4.0));
    HIPCHK(h, launch_green_apply(packed, gray, map_dev, gh, gw, black, n, hh, ww, bit_depth, bayer, s));
    return RVDD_OK;
}

// ---- match (rvdd_set_match): the ring's packed frames mapped in place behind the other stages, out_rgb mapped back.  The gray planes
// stay the sensor's: TV-L1 matches what it always matched
extern "C" int rvdd_set_match(rvdd_t* h, const rvdd_match_cfg* cfg) {
    if (!h) return RVDD_ERR_ARG;
    if (cfg) RC(match_params(h, "rvdd_set_match", cfg));
    ENTER(h);
    HIPCHK(h, hipDeviceSynchronize());      // as rvdd_set_dpc: pushes in flight keep the coefficients they were enqueued with
    h->match.on = cfg != nullptr;
    if (cfg) h->match.cfg = *cfg;
    return RVDD_OK;
}

// ---- resid (rvdd_set_resid): behind the step, the centre frames as it read them against the outputs as it wrote them, before the match's
// way back: with the match on both are in the network's domain, whose unit is the 12-bit DN of the checkpoint's curve
extern "C" int rvdd_set_resid(rvdd_t* h, int32_t on) {
    return h ? acc_switch(h, on != 0, h->resid.on, h->resid.acc) : RVDD_ERR_ARG;
}

extern "C" int rvdd_resid_read(rvdd_t* h, int32_t slot, rvdd_resid_acc* host_out, void* stream) {
    return h ? acc_read(h, "rvdd_resid_read", h->resid.acc, slot, host_out, stream) : RVDD_ERR_ARG;
}

// ---- the push: do frames of hh x ww cells fit every stage as it is set, and is the first-use storage of those that are on there
int stages_fit(rvdd_t* h, int hh, int ww) {
    const size_t B = (size_t)h->cfg.batch;
    auto& dpc = h->dpc;
    if (dpc.on && (hh < 2 || ww < 2)) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with rvdd_set_dpc hh and ww must be >= 2, got %d x %d cells", hh, ww);
    if (dpc.on && !dpc.in) {
        RC(dmalloc(h, reinterpret_cast<void**>(&dpc.counts), B * 2 * sizeof(unsigned)));
        RC(dmalloc(h, reinterpret_cast<void**>(&dpc.in), B * 4 * hh * ww * sizeof(float)));
    }
    const auto& dmap = h->dmap;
    if (dmap.on && (dmap.hh != hh || dmap.ww != ww))
        return fail(h, RVDD_ERR_ARG, "rvdd_video_push: the map of rvdd_set_dpc_map is one of %d x %d cells, the frames have %d x %d", dmap.hh, dmap.ww, hh, ww);
    auto& resid = h->resid;
    if (resid.on && !resid.acc) RC(dmalloc(h, reinterpret_cast<void**>(&resid.acc), B * sizeof(rvdd_resid_acc)));
    auto& rows = h->rows;
    if (rows.on && hh < 5) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with rvdd_set_rows hh must be >= 5, got %d cell rows", hh);
    if (rows.on && ww > rows_max_ww()) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with rvdd_set_rows ww must be <= %d, got %d cells", rows_max_ww(), ww);
    if (rows.on && !rows.acc) {
        RC(dmalloc(h, reinterpret_cast<void**>(&rows.offsets), B * 2 * hh * sizeof(float)));
        RC(dmalloc(h, reinterpret_cast<void**>(&rows.state), B * 2 * hh));
        RC(dmalloc(h, reinterpret_cast<void**>(&rows.acc), B * sizeof(rvdd_rows_acc)));      // last: the mark of a complete allocation
    }
    const auto& cols = h->cols;
    if (cols.on && cols.ww != ww)
        return fail(h, RVDD_ERR_ARG, "rvdd_video_push: the map of rvdd_set_cols is one of %d cell columns, the frames have %d", cols.ww, ww);
    const auto& green = h->geq;
    if (green.on) {
        if (hh < 2 || ww < 2) return fail(h, RVDD_ERR_ARG, "rvdd_video_push: with rvdd_set_green hh and ww must be >= 2, got %d x %d cells", hh, ww);
        int gh, gw;
        green_grid(hh, ww, &gh, &gw);
        if (!(green.gh == 1 && green.gw == 1) && (green.gh != gh || green.gw != gw))
            return fail(h, RVDD_ERR_ARG, "rvdd_video_push: the map of rvdd_set_green is one of %d x %d blocks, frames of %d x %d cells have %d x %d",
                        green.gh, green.gw, hh, ww, gh, gw);
    }
    return RVDD_OK;
}
