// rvdd_noise_fit, rvdd_resid_fit, rvdd_cols_fit, rvdd_green_fit, rvdd_cut_score and rvdd_match_coeffs: the noise curve var(m) = a m - b from a host copy of rvdd_noise_hist's accumulator (the rule is in include/rvdd.h).
// Host code only, f64, no device and no handle; compiled -ffp-contract=off so that tests/noise_ref.py, which runs the same sums in
// the same order in Python doubles, gets the same numbers.
#include "runtime_internal.h"

namespace {

// the lower quartile of the rule's block variance on unit white Gaussian samples; tools/noise_cq.py (seed 20261019, 4194304 blocks):
//   "mean 1.000094  C_Q (lower quartile) 0.805112  C_MED (median) 0.972282  (standard error about 1.4e-04)"
constexpr double kCQ = 0.8051;
constexpr int kMinCount = 16, kMinBins = 4;

// the lower edge of variance sub-bin j
double noise_edge(int j) {
    const uint32_t bits = (uint32_t)(j + ((127 - 6) << 4)) << 19;
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return (double)f;
}

// the value at which the cumulative count of a histogram row of `count` > 0 blocks reaches q * count, linear inside its sub-bin
double noise_quantile(const uint32_t* row, uint64_t count, double q) {
    const double target = q * (double)count;
    uint64_t cum = 0;
    for (int j = 0; j < 512; ++j) {
        const uint64_t c = row[j];
        if (c > 0 && (double)(cum + c) >= target) {
            const double lo = noise_edge(j), hi = noise_edge(j + 1);
            return lo + ((target - (double)cum) / (double)c) * (hi - lo);
        }
        cum += c;
    }
    return noise_edge(512);      // not reached: the counts add up to `count`
}

// The pooled step rvdd_cols_fit and rvdd_green_fit share (the rule is in include/rvdd.h): the median o of the nf values v, tested against
// its own spread -- the median mad of |v - o| -- and clamped to +-limit.  f32, every operation rounded on its own, in the order written
// there.  v is sorted in place, a is scratch.  state: 0 unsupported (nf < need: nothing else is formed), 3 insignificant, 1 applied, 2
// applied and clamped; value: what the map gets; o: the median before the clamp; se: its standard error.  zero_is_nothing: a median of
// exactly zero is insignificant whatever its spread (the green rule; the column rule applies it with a map of zero)
struct Pooled {
    int state;
    float value, o, se;
};
Pooled pooled_median(std::vector<float>& v, std::vector<float>& a, int need, float k2, float limit, bool zero_is_nothing) {
    const int nf = (int)v.size();
    if (nf < need) return {0, 0.0f, 0.0f, 0.0f};
    std::sort(v.begin(), v.end());
    const float o = (v[(size_t)(nf - 1) / 2] + v[(size_t)nf / 2]) * 0.5f;
    a.resize((size_t)nf);
    for (int i = 0; i < nf; ++i) a[(size_t)i] = std::fabs(v[(size_t)i] - o);
    std::sort(a.begin(), a.end());
    const float mad = (a[(size_t)(nf - 1) / 2] + a[(size_t)nf / 2]) * 0.5f;
    const float se = ((1.2533f * 1.4826f) * mad) / std::sqrt((float)nf);
    if ((zero_is_nothing && o == 0.0f) || (o * o) * (float)nf < k2 * (3.4528f * (mad * mad))) return {3, 0.0f, o, se};
    const float oc = std::fmin(std::fmax(o, -limit), limit);
    return {oc != o ? 2 : 1, oc, o, se};
}

}  // namespace

extern "C" int rvdd_noise_fit(const rvdd_noise_acc* acc, int32_t bit_depth, rvdd_noise_curve* out) {
    if (!acc) return fail(nullptr, RVDD_ERR_ARG, "rvdd_noise_fit: acc_host is required");
    if (!out) return fail(nullptr, RVDD_ERR_ARG, "rvdd_noise_fit: out is required");
    if (bit_depth < 1 || bit_depth > 16) return fail(nullptr, RVDD_ERR_ARG, "rvdd_noise_fit: bit_depth must be 1..16, got %d", bit_depth);
    double ms[64], vs[64], ns[64];
    int bins = 0;
    uint64_t blocks = 0;
    for (int i = 0; i < 64; ++i) {
        uint64_t count = 0;
        for (int j = 0; j < 512; ++j) count += acc->hist[i][j];
        if (count < (uint64_t)kMinCount) continue;
        ms[bins] = (double)acc->msum[i] / 16.0 / (double)count;
        vs[bins] = noise_quantile(acc->hist[i], count, 0.25) / kCQ;
        ns[bins] = (double)count;
        blocks += count;
        ++bins;
    }
    if (bins < kMinBins)
        return fail(nullptr, RVDD_ERR_STATE, "rvdd_noise_fit: %d usable mean bins (of %d blocks or more), at least %d are needed: too few frames, or "
                    "footage that is clipped or constant almost everywhere (%llu blocks seen, %llu clipped, %llu constant)", bins, kMinCount,
                    kMinBins, (unsigned long long)acc->counters[0], (unsigned long long)acc->counters[1], (unsigned long long)acc->counters[2]);
    double m_min = ms[0], m_max = ms[0];
    for (int k = 1; k < bins; ++k) {
        m_min = ms[k] < m_min ? ms[k] : m_min;
        m_max = ms[k] > m_max ? ms[k] : m_max;
    }
    const double range = (double)(1u << bit_depth);
    if (m_max - m_min < range / 16.0)
        return fail(nullptr, RVDD_ERR_STATE, "rvdd_noise_fit: the footage has too little tonal range: the %d usable bin means span %.1f DN (%.1f .. "
                    "%.1f), a curve needs %.0f (1/16 of 2^%d)", bins, m_max - m_min, m_min, m_max, range / 16.0, bit_depth);
    double ws[64], sw = 0.0, swm = 0.0, swv = 0.0;
    for (int k = 0; k < bins; ++k) {
        ws[k] = ns[k] / (vs[k] * vs[k]);
        sw += ws[k];
        swm += ws[k] * ms[k];
        swv += ws[k] * vs[k];
    }
    const double mbar = swm / sw, vbar = swv / sw;      // centred: the normal equations lose no digits to the means' offset
    double smm = 0.0, smv = 0.0;
    for (int k = 0; k < bins; ++k) {
        smm += ws[k] * ((ms[k] - mbar) * (ms[k] - mbar));
        smv += ws[k] * ((ms[k] - mbar) * (vs[k] - vbar));
    }
    const double a = smv / smm, b = a * mbar - vbar;
    double sr = 0.0;
    for (int k = 0; k < bins; ++k) {
        const double r = (vs[k] - (a * ms[k] - b)) / vs[k];
        sr += ns[k] * (r * r);
    }
    *out = rvdd_noise_curve{a, b, m_min, m_max, std::sqrt(sr / (double)blocks), blocks, bins, 0};
    return RVDD_OK;
}

// rvdd_resid_fit: a host copy of rvdd_resid_stats' accumulator judged against the curve var(m) = a m - b (the rule is in include/rvdd.h).
// f64, each operation as written, sums over the bins in ascending order; the totals are exact integer sums converted once: the same
// formulas in Python floats and integers give the same numbers (tests/resid_ref.py).
extern "C" int rvdd_resid_fit(const rvdd_resid_acc* acc, int32_t bit_depth, double a, double b, rvdd_resid_report* out) {
    if (!acc) return fail(nullptr, RVDD_ERR_ARG, "rvdd_resid_fit: acc_host is required");
    if (!out) return fail(nullptr, RVDD_ERR_ARG, "rvdd_resid_fit: out is required");
    if (bit_depth < 1 || bit_depth > 16) return fail(nullptr, RVDD_ERR_ARG, "rvdd_resid_fit: bit_depth must be 1..16, got %d", bit_depth);
    if (!std::isfinite(a)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_resid_fit: a must be finite, got %g", a);
    if (!std::isfinite(b)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_resid_fit: b must be finite, got %g", b);
    constexpr uint64_t kMinSamples = 1024;
    const double S = bit_depth == 16 ? 0.5 : (double)(1u << (15 - bit_depth));
    double ms[64], vs[64], rs[64], ns[64];
    int bins = 0;
    uint64_t samples = 0;
    for (int j = 0; j < 64; ++j) {
        if (acc->n[j] < kMinSamples) continue;
        const double n = (double)acc->n[j];
        const double m = (double)acc->msum[j] / 16.0 / n;
        const double p = a * m - b;
        if (!(p > 0.0)) continue;
        const double u = (double)acc->s1[j] / n / S;
        const double v = (double)acc->s2[j] / n / (S * S) - u * u;
        ms[bins] = m;
        vs[bins] = v;
        rs[bins] = v / p;
        ns[bins] = n;
        samples += acc->n[j];
        ++bins;
    }
    if (bins < kMinBins)
        return fail(nullptr, RVDD_ERR_STATE, "rvdd_resid_fit: %d usable level bins (of %llu samples or more, where the curve a = %g, b = %g predicts "
                    "noise), at least %d are needed: too few frames, or a curve that predicts no noise at the footage's levels", bins,
                    (unsigned long long)kMinSamples, a, b, kMinBins);
    rvdd_resid_report r{};
    double sn = 0.0, snr = 0.0;
    for (int k = 0; k < bins; ++k) {
        sn += ns[k];
        snr += ns[k] * rs[k];
    }
    r.ratio = snr / sn;
    const double third = (double)samples / 3.0;
    for (int side = 0; side < 2; ++side) {      // the darkest third walking upwards, the brightest walking downwards
        double c = 0.0, sw = 0.0, swr = 0.0;
        for (int i = 0; i < bins; ++i) {
            const int k = side ? bins - 1 - i : i;
            const double rest = third - c;
            const double w = ns[k] < rest ? ns[k] : rest;
            if (!(w > 0.0)) break;
            sw += w;
            swr += w * rs[k];
            c += w;
        }
        (side ? r.ratio_hi : r.ratio_lo) = swr / sw;
    }
    __int128 t1 = 0, t11 = 0;
    unsigned __int128 tn = 0, t2 = 0, tn11 = 0;
    for (int j = 0; j < 64; ++j) {
        tn += acc->n[j];
        t1 += acc->s1[j];
        t2 += acc->s2[j];
        tn11 += acc->n11[j];
        t11 += acc->s11[j];
    }
    r.bias = (double)t1 / (double)tn / S;
    r.rho = tn11 && t2 ? ((double)t11 / (double)tn11) / ((double)t2 / (double)tn) : 0.0;
    // the curve the residual follows: rvdd_noise_fit's centred normal equations over the bins that have a variance
    double sw = 0.0, swm = 0.0, swv = 0.0;
    int fit = 0;
    for (int k = 0; k < bins; ++k) {
        if (!(vs[k] > 0.0)) continue;
        const double w = ns[k] / (vs[k] * vs[k]);
        sw += w;
        swm += w * ms[k];
        swv += w * vs[k];
        ++fit;
    }
    if (fit >= 2) {
        const double mbar = swm / sw, vbar = swv / sw;
        double smm = 0.0, smv = 0.0;
        for (int k = 0; k < bins; ++k) {
            if (!(vs[k] > 0.0)) continue;
            const double w = ns[k] / (vs[k] * vs[k]);
            smm += w * ((ms[k] - mbar) * (ms[k] - mbar));
            smv += w * ((ms[k] - mbar) * (vs[k] - vbar));
        }
        if (smm > 0.0) {
            r.a_fit = smv / smm;
            r.b_fit = r.a_fit * mbar - vbar;
        }
    }
    r.samples = samples;
    r.bins = bins;
    *out = r;
    return RVDD_OK;
}

// rvdd_cols_fit: the static column map from host copies of rvdd_cols_estimate's offsets and states of F frames (the rule is in
// include/rvdd.h).  f32, every operation rounded on its own, in the order written there; the floor's mean alone is summed in f64 over
// the columns in the order (parity, column): tests/cols_ref.py says the same in NumPy f32 and gets the same bits.
extern "C" int rvdd_cols_fit(const float* offsets, const uint8_t* state, int32_t F, int32_t ww, const rvdd_cols_fit_cfg* cfg, float* map,
                             uint8_t* mstate, rvdd_cols_stats* stats) {
    if (!offsets) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: offsets_host is required");
    if (!state) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: state_host is required");
    if (!cfg) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: fit_cfg is required");
    if (!map) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: map_host is required");
    if (!mstate) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: mstate_host is required");
    if (F < 1) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: F must be >= 1, got %d", F);
    if (ww < 1) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: ww must be >= 1, got %d", ww);
    if (!(cfg->k_sig >= 0.0f) || !std::isfinite(cfg->k_sig)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: k_sig must be finite and >= 0, got %g", cfg->k_sig);
    if (!(cfg->max_dn > 0.0f) || !std::isfinite(cfg->max_dn)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cols_fit: max_dn must be finite and > 0, got %g", cfg->max_dn);
    const int need = cfg->min_frames > 1 ? cfg->min_frames : 1;
    const float k2 = cfg->k_sig * cfg->k_sig;
    rvdd_cols_stats st{};
    double floor_sum = 0.0;
    uint64_t supported = 0;
    std::vector<float> v, a;
    for (int64_t jc = 0; jc < 2 * (int64_t)ww; ++jc) {
        v.clear();
        for (int i = 0; i < F; ++i)
            if (state[(int64_t)i * 2 * ww + jc] == 1) v.push_back(offsets[(int64_t)i * 2 * ww + jc]);
        const Pooled p = pooled_median(v, a, need, k2, cfg->max_dn, false);
        map[jc] = p.value;
        mstate[jc] = (uint8_t)p.state;
        st.counts[p.state] += 1;
        if (p.state == 0) continue;
        floor_sum += (double)p.se;
        ++supported;
        if (p.state == 3) continue;
        const long long q = (long long)(int)std::rint(16.0f * p.value);
        st.sum_q2 += q * q;
    }
    st.floor_dn = supported ? floor_sum / (double)supported : 0.0;
    if (stats) *stats = st;
    return RVDD_OK;
}

// rvdd_green_fit: the static map of green gains from host copies of rvdd_green_estimate's e, level and state of F frames (the rule is in
// include/rvdd.h).  f32, every operation rounded on its own; the pooled step is rvdd_cols_fit's (pooled_median); the floor's mean alone
// is summed in f64 over the blocks in their order: tests/green_ref.py says the same in NumPy f32 and gets the same bits.
extern "C" int rvdd_green_fit(const float* e, const float* level, const uint8_t* state, int32_t F, int32_t gh, int32_t gw, float black,
                              const rvdd_green_fit_cfg* cfg, float* map, uint8_t* mstate, rvdd_green_stats* stats) {
    const char* fn = "rvdd_green_fit";
    if (!e) return fail(nullptr, RVDD_ERR_ARG, "%s: e_host is required", fn);
    if (!level) return fail(nullptr, RVDD_ERR_ARG, "%s: level_host is required", fn);
    if (!state) return fail(nullptr, RVDD_ERR_ARG, "%s: state_host is required", fn);
    if (!cfg) return fail(nullptr, RVDD_ERR_ARG, "%s: fit_cfg is required", fn);
    if (!map) return fail(nullptr, RVDD_ERR_ARG, "%s: map_host is required", fn);
    if (!mstate) return fail(nullptr, RVDD_ERR_ARG, "%s: mstate_host is required", fn);
    if (F < 1) return fail(nullptr, RVDD_ERR_ARG, "%s: F must be >= 1, got %d", fn, F);
    if (gh < 1) return fail(nullptr, RVDD_ERR_ARG, "%s: gh must be >= 1, got %d", fn, gh);
    if (gw < 1) return fail(nullptr, RVDD_ERR_ARG, "%s: gw must be >= 1, got %d", fn, gw);
    if (!std::isfinite(black)) return fail(nullptr, RVDD_ERR_ARG, "%s: black must be finite, got %g", fn, (double)black);
    if (!(cfg->k_sig >= 0.0f) || !std::isfinite(cfg->k_sig)) return fail(nullptr, RVDD_ERR_ARG, "%s: k_sig must be finite and >= 0, got %g", fn, cfg->k_sig);
    if (!(cfg->max_gain > 0.0f) || !std::isfinite(cfg->max_gain)) return fail(nullptr, RVDD_ERR_ARG, "%s: max_gain must be finite and > 0, got %g", fn, cfg->max_gain);
    if (!(cfg->min_signal > 0.0f) || !std::isfinite(cfg->min_signal)) return fail(nullptr, RVDD_ERR_ARG, "%s: min_signal must be finite and > 0, got %g", fn, cfg->min_signal);
    const int need = cfg->min_frames > 1 ? cfg->min_frames : 1;
    const float k2 = cfg->k_sig * cfg->k_sig;
    const int64_t blocks = (int64_t)gh * gw;
    rvdd_green_stats st{};
    double floor_sum = 0.0;
    uint64_t supported = 0;
    std::vector<float> v, a, os;
    for (int64_t b = 0; b < blocks; ++b) {
        v.clear();
        for (int i = 0; i < F; ++i) {
            const int64_t at = (int64_t)i * blocks + b;
            const float signal = level[at] - black;
            if (state[at] == 1 && signal >= cfg->min_signal) v.push_back(e[at] / signal);
        }
        const Pooled p = pooled_median(v, a, need, k2, cfg->max_gain, true);
        map[b] = p.value;
        mstate[b] = (uint8_t)p.state;
        st.counts[p.state] += 1;
        if (p.state == 0) continue;
        floor_sum += (double)p.se;
        ++supported;
        os.push_back(p.o);
        if (p.state == 3) continue;
        const long long q = (long long)(int)std::rint(16384.0f * p.value);
        st.sum_q2 += q * q;
    }
    st.floor = supported ? floor_sum / (double)supported : 0.0;
    const Pooled flat = pooled_median(os, a, 1, k2, cfg->max_gain, true);      // the supported blocks' medians in the frames' place
    st.flat_gain = flat.value;
    st.flat_se = flat.se;
    st.flat_state = flat.state;
    if (stats) *stats = st;
    return RVDD_OK;
}

// rvdd_cut_score: the distance of two frame signatures (rvdd_frame_sigs; the rule is in include/rvdd.h).  Integer sums, each converted to
// f64 once, one division each: the same formulas on Python integers give the same bits (tests/cuts_ref.py).
extern "C" int rvdd_cut_score(const rvdd_frame_sig* a, const rvdd_frame_sig* b, int32_t hh, int32_t ww, double* out2) {
    if (!a) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: a is required");
    if (!b) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: b is required");
    if (!out2) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: out2 is required");
    if (hh < 16) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: hh must be >= 16, got %d", hh);
    if (ww < 16) return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: ww must be >= 16, got %d", ww);
    const uint64_t cells = (uint64_t)hh * (uint64_t)ww;
    uint64_t ha[64], hb[64], na = 0, nb = 0, dh = 0;
    for (int j = 0; j < 64; ++j) {
        ha[j] = hb[j] = 0;
        for (int band = 0; band < 16; ++band) {
            ha[j] += a->hist[band][j];
            hb[j] += b->hist[band][j];
        }
        na += ha[j];
        nb += hb[j];
        dh += ha[j] > hb[j] ? ha[j] - hb[j] : hb[j] - ha[j];
    }
    if (na != cells)
        return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: a counts %llu cells, a frame of hh x ww = %d x %d has %llu: a signature of another frame size",
                    (unsigned long long)na, hh, ww, (unsigned long long)cells);
    if (nb != cells)
        return fail(nullptr, RVDD_ERR_ARG, "rvdd_cut_score: b counts %llu cells, a frame of hh x ww = %d x %d has %llu: a signature of another frame size",
                    (unsigned long long)nb, hh, ww, (unsigned long long)cells);
    unsigned __int128 dg = 0, mg = 0;          // 256 sums of up to 2^62 cells x 2^18 each
    for (int band = 0; band < 16; ++band)
        for (int col = 0; col < 16; ++col) {
            const uint64_t sa = a->sum[band][col], sb = b->sum[band][col];
            dg += sa > sb ? sa - sb : sb - sa;
            mg += sa > sb ? sa : sb;
        }
    out2[0] = (double)dh / (double)(2 * (unsigned __int128)cells);
    out2[1] = (double)dg / (mg ? (double)mg : 1.0);
    return RVDD_OK;
}

// The affine map of the samples that takes the footage's curve onto the checkpoint's (the derivation is in include/rvdd.h): f64, each
// operation as written, so that the same formulas in Python doubles give the same numbers.
extern "C" int rvdd_match_coeffs(double a, double b, int32_t bit_depth, double a_ref, double b_ref, rvdd_match_cfg* out, double* s_t) {
    if (!out) return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: out is required");
    if (!(a > 0.0) || !std::isfinite(a)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: a must be finite and > 0, got %g", a);
    if (!std::isfinite(b)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: b must be finite, got %g", b);
    if (bit_depth < 1 || bit_depth > 16) return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: bit_depth must be 1..16, got %d", bit_depth);
    if (!(a_ref > 0.0) || !std::isfinite(a_ref)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: a_ref must be finite and > 0, got %g", a_ref);
    if (!std::isfinite(b_ref)) return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: b_ref must be finite, got %g", b_ref);
    const double k = 4095.0 / (double)((1u << bit_depth) - 1u);
    const double a12 = k * a, b12 = (k * k) * b;
    const double s = a_ref / a12;
    const double t = (b_ref - (s * s) * b12) / a_ref;
    const rvdd_match_cfg cfg = {(float)s, (float)((s - 1.0) + (2.0 * t) / 4095.0)};
    // a curve so far from the checkpoint's that the f32 coefficients leave the range rvdd_match_raw accepts
    if (!(cfg.scale > 0.0f) || !std::isfinite(cfg.scale) || !std::isfinite(cfg.offset))
        return fail(nullptr, RVDD_ERR_ARG, "rvdd_match_coeffs: a = %g, b = %g against a_ref = %g, b_ref = %g gives scale %g, offset %g, which no f32 "
                    "map can carry", a, b, a_ref, b_ref, (double)cfg.scale, (double)cfg.offset);
    *out = cfg;
    if (s_t) {
        s_t[0] = s;
        s_t[1] = t;
    }
    return RVDD_OK;
}
