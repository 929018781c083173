// Measurement: per-class event brackets around launches (Scope), their read-out, and the handle's stopwatch.
#include "runtime_internal.h"

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

static int prof_flush(rvdd_t* h) {
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

extern "C" {

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
