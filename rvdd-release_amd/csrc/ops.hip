// The stand-alone operators of the ABI: each one validates, selects the handle's device and launches.
#include "runtime_internal.h"

namespace {
// rvdd_psnr_l1_batch as `fn`, the entry point the caller used (rvdd_psnr_l1: one slice)
int psnr_l1_n(rvdd_t* h, const char* fn, const float* den, const float* gt, int32_t n, int64_t count, float* out, void* stream) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !den || !gt || !out || n < 0 || count <= 0) return fail(h, RVDD_ERR_ARG, "%s: bad argument", fn);
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int nblk = (int)((count + 256 * 16 - 1) / (256 * 16));      // the partition of every slice
    if (nblk > 1024) nblk = 1024;
    RC(ensure_loss_batch(h, (size_t)n * (2 * nblk + 2)));
    double* res = h->loss_batch + (size_t)n * 2 * nblk;
    HIPCHK(h, launch_loss_reduce_batch(den, gt, n, count, h->loss_batch, nblk, res, s));
    std::vector<double> r((size_t)2 * n);
    HIPCHK(h, hipMemcpyAsync(r.data(), res, r.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (hipError_t e = tvl1_check(h->tvl1, s); e != hipSuccess)       // an asynchronous flow batch in front of the frames just measured
        return fail(h, RVDD_ERR_HIP, "%s: an asynchronous rvdd_tvl1flow_batch before this call failed: %s", fn, hipGetErrorString(e));
    for (int i = 0; i < n; ++i) {
        out[2 * i] = (float)(100.0 * r[2 * i] / (double)count);
        out[2 * i + 1] = (float)(10.0 * std::log10(4.0 / (r[2 * i + 1] / (double)count)));
    }
    return RVDD_OK;
}
}  // namespace

// the TV-L1 workspace of nx x ny images (rvdd_tvl1flow, tvl1flow_batch): the cached one, or a new one in its place
static int ensure_tvl1(rvdd_t* h, int nx, int ny, void* stream) {
    if (h->tvl1 && tvl1_ws_nx(h->tvl1) == nx && tvl1_ws_ny(h->tvl1) == ny) return RVDD_OK;
    HIPCHK(h, hipDeviceSynchronize());
    HIPCHK(h, tvl1_check(h->tvl1, static_cast<hipStream_t>(stream)));      // what an asynchronous batch on the old workspace left unread
    tvl1_free(h->tvl1);
    h->tvl1 = nullptr;
    HIPCHK(h, tvl1_alloc(&h->tvl1, nx, ny));
    return RVDD_OK;
}

// rvdd_tvl1flow_batch; `async`: without iteration counts the batch is enqueued and the call returns (option "tvl1_async")
int tvl1flow_batch(rvdd_t* h, const float* I0, const float* I1, float* u, int32_t n, int32_t nx, int32_t ny, int32_t* iterations,
                   void* stream, bool async) {
    if (h && n == 0) return RVDD_OK;
    if (!h || !I0 || !I1 || !u || n < 0 || nx < 16 || ny < 16)
        return fail(h, RVDD_ERR_ARG, "rvdd_tvl1flow_batch: bad argument (images must be >= 16x16)");
    ENTER(h);
    if (!tvl1_size_ok(nx, ny))
        return fail(h, RVDD_ERR_ARG, "rvdd_tvl1flow_batch: image too skinny for its pyramid (the reference reads out of bounds at this size)");
    RC(ensure_tvl1(h, nx, ny, stream));
    std::vector<int> it((size_t)n, 0);
    HIPCHK(h, tvl1_run_batch(h->tvl1, I0, I1, u, n, static_cast<hipStream_t>(stream), iterations ? it.data() : nullptr, async));
    if (iterations)
        for (int i = 0; i < n; ++i) iterations[i] = it[(size_t)i];
    return RVDD_OK;
}

int dpc_params(rvdd_t* h, const char* fn, const rvdd_dpc_cfg* cfg, DpcParams* out) {
    RC(need_ptr(h, fn, cfg, "cfg"));
    if (!(cfg->k_hot >= 0.0f) || !std::isfinite(cfg->k_hot)) return fail(h, RVDD_ERR_ARG, "%s: k_hot must be finite and >= 0 (0 = off), got %g", fn, cfg->k_hot);
    if (!(cfg->k_dead >= 0.0f) || !std::isfinite(cfg->k_dead)) return fail(h, RVDD_ERR_ARG, "%s: k_dead must be finite and >= 0 (0 = off), got %g", fn, cfg->k_dead);
    if (!std::isfinite(cfg->noise_a)) return fail(h, RVDD_ERR_ARG, "%s: noise_a must be finite, got %g", fn, cfg->noise_a);
    if (!std::isfinite(cfg->noise_b)) return fail(h, RVDD_ERR_ARG, "%s: noise_b must be finite, got %g", fn, cfg->noise_b);
    if (!(cfg->var_floor > 0.0f) || !std::isfinite(cfg->var_floor)) return fail(h, RVDD_ERR_ARG, "%s: var_floor must be finite and > 0, got %g", fn, cfg->var_floor);
    // the squares rounded to f32 once, here (1e18 squared is +inf: such a side can never flag)
    const float k2h = cfg->k_hot * cfg->k_hot, k2d = cfg->k_dead * cfg->k_dead;
    *out = DpcParams{cfg->k_hot, cfg->k_dead, k2h, k2d, cfg->noise_a, cfg->noise_b, cfg->var_floor, 0.0f};
    return RVDD_OK;
}

// the gate of rvdd_rows_cfg, rvdd_cols_cfg and rvdd_green_cfg (Cfg): the fields the three share, in their order; *out = the kernel's parameters without a clamp
template <class Cfg>
static int line_params(rvdd_t* h, const char* fn, const Cfg* cfg, RowsParams* out) {
    RC(need_ptr(h, fn, cfg, "cfg"));
    if (!(cfg->k_gate > 0.0f) || !std::isfinite(cfg->k_gate)) return fail(h, RVDD_ERR_ARG, "%s: k_gate must be finite and > 0, got %g", fn, cfg->k_gate);
    if (!std::isfinite(cfg->noise_a)) return fail(h, RVDD_ERR_ARG, "%s: noise_a must be finite, got %g", fn, cfg->noise_a);
    if (!std::isfinite(cfg->noise_b)) return fail(h, RVDD_ERR_ARG, "%s: noise_b must be finite, got %g", fn, cfg->noise_b);
    if (!(cfg->var_floor > 0.0f) || !std::isfinite(cfg->var_floor)) return fail(h, RVDD_ERR_ARG, "%s: var_floor must be finite and > 0, got %g", fn, cfg->var_floor);
    // the square rounded to f32 once, here (+inf for a huge gate: every finite sample is used)
    *out = RowsParams{cfg->k_gate * cfg->k_gate, cfg->noise_a, cfg->noise_b, cfg->var_floor, 0.0f, 0.0f};
    return RVDD_OK;
}

int rows_params(rvdd_t* h, const char* fn, const rvdd_rows_cfg* cfg, RowsParams* out) {
    RC(line_params(h, fn, cfg, out));
    if (!(cfg->max_dn > 0.0f) || !std::isfinite(cfg->max_dn)) return fail(h, RVDD_ERR_ARG, "%s: max_dn must be finite and > 0, got %g", fn, cfg->max_dn);
    out->max_dn = cfg->max_dn;
    return RVDD_OK;
}

// the shape checks of the row (rows = true) and column calls: the axis the eight neighbours lie along needs five, the other one
static int line_shape(rvdd_t* h, const char* fn, bool rows, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth) {
    RC(need_bit_depth(h, fn, bit_depth));
    if ((rows ? hh : ww) < 5) return fail(h, RVDD_ERR_ARG, "%s: %s must be >= 5 (four %s neighbours on either side, mirrored about the site), got %d", fn, rows ? "hh" : "ww", rows ? "vertical" : "horizontal", rows ? hh : ww);
    if ((rows ? ww : hh) < 1) return fail(h, RVDD_ERR_ARG, "%s: %s must be >= 1, got %d", fn, rows ? "ww" : "hh", rows ? ww : hh);
    if (rows && ww > rows_max_ww()) return fail(h, RVDD_ERR_ARG, "%s: ww must be <= %d (a workgroup holds the 2 ww samples of a row in registers), got %d", fn, rows_max_ww(), ww);
    RC(need_count(h, fn, n));
    return RVDD_OK;
}

int match_params(rvdd_t* h, const char* fn, const rvdd_match_cfg* cfg) {
    RC(need_ptr(h, fn, cfg, "cfg"));
    if (!(cfg->scale > 0.0f) || !std::isfinite(cfg->scale)) return fail(h, RVDD_ERR_ARG, "%s: scale must be finite and > 0, got %g", fn, cfg->scale);
    if (!std::isfinite(cfg->offset)) return fail(h, RVDD_ERR_ARG, "%s: offset must be finite, got %g", fn, cfg->offset);
    return RVDD_OK;
}

namespace {
// rvdd_match_raw (c = 4, inverse = false) and rvdd_unmatch_rgb (c = 3, inverse = true) as `fn`: [n][c][d0][d1] floats, `in_name` /
// `out_name` and `d0_name` / `d1_name` the caller's words for them
int match_call(rvdd_t* h, const char* fn, const char* in_name, const char* out_name, const char* d0_name, const char* d1_name, const float* in,
               float* out, int32_t n, int c, int32_t d0, int32_t d1, const rvdd_match_cfg* cfg, bool inverse, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(match_params(h, fn, cfg));
    RC(need_count(h, fn, n));
    if (d0 < 1) return fail(h, RVDD_ERR_ARG, "%s: %s must be >= 1, got %d", fn, d0_name, d0);
    if (d1 < 1) return fail(h, RVDD_ERR_ARG, "%s: %s must be >= 1, got %d", fn, d1_name, d1);
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, fn, {{in, in_name}, {out, out_name}}));
    const int64_t count = (int64_t)n * c * d0 * d1;      // below 2^63: three 31-bit factors and c <= 4
    if (match_blocks(count, match_wide(in, out, count)) < 0)
        return fail(h, RVDD_ERR_ARG, "%s: n * %s * %s = %d * %d * %d needs a launch of more than 2^31 - 1 blocks", fn, d0_name, d1_name, n, d0, d1);
    // a thread reads its own samples and then writes them: the same tensor is fine, a shifted one is a race
    const uintptr_t a = reinterpret_cast<uintptr_t>(in), b = reinterpret_cast<uintptr_t>(out);
    const uintptr_t bytes = (uintptr_t)count * sizeof(float);
    if (a != b && a < b + bytes && b < a + bytes)
        return fail(h, RVDD_ERR_ARG, "%s: %s must be %s itself (in place) or not overlap it (%d frames of %d x %d x %d floats each)", fn, out_name,
                    in_name, n, c, d0, d1);
    ENTER(h);
    HIPCHK(h, launch_match(in, out, count, cfg->scale, cfg->offset, inverse, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}
}  // namespace

extern "C" {

int rvdd_match_raw(rvdd_t* h, const float* packed_in, float* packed_out, int32_t n, int32_t hh, int32_t ww, const rvdd_match_cfg* cfg,
                   void* stream) {
    return match_call(h, "rvdd_match_raw", "packed_in", "packed_out", "hh", "ww", packed_in, packed_out, n, 4, hh, ww, cfg, false, stream);
}

int rvdd_unmatch_rgb(rvdd_t* h, const float* rgb_in, float* rgb_out, int32_t n, int32_t H, int32_t W, const rvdd_match_cfg* cfg, void* stream) {
    return match_call(h, "rvdd_unmatch_rgb", "rgb_in", "rgb_out", "H", "W", rgb_in, rgb_out, n, 3, H, W, cfg, true, stream);
}

int rvdd_psnr_l1(rvdd_t* h, const float* den, const float* gt, int64_t count, float* out2, void* stream) {
    return psnr_l1_n(h, "rvdd_psnr_l1", den, gt, 1, count, out2, stream);
}

int rvdd_psnr_l1_batch(rvdd_t* h, const float* den, const float* gt, int32_t n, int64_t count, float* out, void* stream) {
    return psnr_l1_n(h, "rvdd_psnr_l1_batch", den, gt, n, count, out, stream);
}

int rvdd_demosaic_ha_bayer(rvdd_t* h, const float* raw, int32_t n, int32_t hh, int32_t ww, int32_t pattern, float* rgb, void* stream) {
    if (h) RC(need_bayer(h, "rvdd_demosaic_ha_bayer", pattern));
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
    RC(ensure_tvl1(h, nx, ny, stream));
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

int rvdd_ycbcr(rvdd_t* h, const float* disp, int32_t n, int32_t H, int32_t W, int32_t depth, void* frames, void* stream) {
    const char* fn = "rvdd_ycbcr";
    if (!h) return RVDD_ERR_ARG;
    if (depth != 8 && depth != 10) return fail(h, RVDD_ERR_ARG, "%s: depth must be 8 or 10, got %d", fn, depth);
    if (H < 2 || (H & 1)) return fail(h, RVDD_ERR_ARG, "%s: H must be even and >= 2 (chroma is one sample per 2 x 2 quad), got %d", fn, H);
    if (W < 2 || (W & 1)) return fail(h, RVDD_ERR_ARG, "%s: W must be even and >= 2 (chroma is one sample per 2 x 2 quad), got %d", fn, W);
    RC(need_count(h, fn, n));
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, fn, {{disp, "disp"}, {frames, "frames"}}));
    RC(need_blocks(h, fn, ycbcr_blocks(n, H, W, ycbcr_wide(disp, W, frames)), "n * H * W", n, H, W));
    ENTER(h);
    HIPCHK(h, launch_ycbcr(disp, n, H, W, depth, frames, static_cast<hipStream_t>(stream)));
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
    RC(need_bit_depth(h, "rvdd_ingest_raw", bit_depth));
    if (n == 0) return RVDD_OK;
    if (!frames || n < 0 || hh < 1 || ww < 1) return fail(h, RVDD_ERR_ARG, "rvdd_ingest_raw: bad argument (frames, n >= 0, hh, ww >= 1)");
    ENTER(h);
    HIPCHK(h, launch_ingest_raw(frames, dtype, layout, n, hh, ww, bit_depth, packed, gray, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_gray_of_rgb(rvdd_t* h, const float* rgb, int32_t n, int32_t H, int32_t W, int32_t pattern, int32_t bit_depth, float* gray,
                     void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_bayer(h, "rvdd_gray_of_rgb", pattern));
    RC(need_bit_depth(h, "rvdd_gray_of_rgb", bit_depth));
    if (H < 2 || (H & 1)) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: H must be even and >= 2, got %d", H);
    if (W < 2 || (W & 1)) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: W must be even and >= 2, got %d", W);
    if (n == 0) return RVDD_OK;
    RC(need_count(h, "rvdd_gray_of_rgb", n));
    if (!rgb || !gray) return fail(h, RVDD_ERR_ARG, "rvdd_gray_of_rgb: rgb and gray are required");
    ENTER(h);
    HIPCHK(h, launch_gray_of_rgb(rgb, n, H / 2, W / 2, pattern, bit_depth, gray, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_egress(rvdd_t* h, const float* rgb, int32_t n, int32_t H, int32_t W, int32_t layout, int32_t dtype, int32_t bit_depth,
                int32_t pattern, void* out, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (layout < RVDD_OUT_RGB_HWC || layout > RVDD_OUT_PACKED_HWC)
        return fail(h, RVDD_ERR_ARG, "rvdd_egress: layout must be 0 (RGB HWC), 1 (mosaic) or 2 (packed HWC), got %d", layout);
    if (dtype != RVDD_RAW_U16 && dtype != RVDD_RAW_F32) return fail(h, RVDD_ERR_ARG, "rvdd_egress: dtype must be 0 (u16) or 1 (f32), got %d", dtype);
    RC(need_bit_depth(h, "rvdd_egress", bit_depth));
    const bool cfa = layout != RVDD_OUT_RGB_HWC;
    if (cfa) RC(need_bayer(h, "rvdd_egress", pattern));
    if (H < 1 || (cfa && (H & 1))) return fail(h, RVDD_ERR_ARG, "rvdd_egress: H must be >= 1, and even for the mosaic layouts, got %d", H);
    if (W < 1 || (cfa && (W & 1))) return fail(h, RVDD_ERR_ARG, "rvdd_egress: W must be >= 1, and even for the mosaic layouts, got %d", W);
    RC(need_count(h, "rvdd_egress", n));
    if (n == 0) return RVDD_OK;
    if (!rgb || !out) return fail(h, RVDD_ERR_ARG, "rvdd_egress: rgb and out are required");
    bool wide;
    RC(need_blocks(h, "rvdd_egress", egress_blocks(rgb, n, H, W, layout, dtype, out, &wide), "n * H * W", n, H, W));
    ENTER(h);
    HIPCHK(h, launch_egress(rgb, n, H, W, layout, dtype, bit_depth, pattern, out, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

// the checks rvdd_ingest_bits and rvdd_egress_bits share (ww in cells); 0 = fine
static int bits_args(rvdd_t* h, const char* fn, int32_t order, int32_t bit_depth, int32_t ww) {
    if (order != RVDD_BITS_MIPI && order != RVDD_BITS_MSB) return fail(h, RVDD_ERR_ARG, "%s: order must be 0 (MIPI CSI-2) or 1 (MSB first), got %d", fn, order);
    if (bit_depth != 10 && bit_depth != 12 && bit_depth != 14) return fail(h, RVDD_ERR_ARG, "%s: bit_depth must be 10, 12 or 14, got %d", fn, bit_depth);
    if (order == RVDD_BITS_MIPI && bit_depth != 12 && (ww & 1))
        return fail(h, RVDD_ERR_ARG, "%s: ww must be even for MIPI RAW%d (groups of four pixels), got ww = %d", fn, bit_depth, ww);
    return RVDD_OK;
}

int rvdd_ingest_bits(rvdd_t* h, const uint8_t* frames, int32_t order, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, float* packed,
                     float* gray, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_min(h, "rvdd_ingest_bits", "hh", hh, 1));
    RC(need_min(h, "rvdd_ingest_bits", "ww", ww, 1));
    RC(bits_args(h, "rvdd_ingest_bits", order, bit_depth, ww));
    RC(need_count(h, "rvdd_ingest_bits", n));
    if (n == 0) return RVDD_OK;
    RC(need_ptr(h, "rvdd_ingest_bits", frames, "frames"));
    RC(need_blocks(h, "rvdd_ingest_bits", bits_blocks(n, hh, ww, ingest_bits_fast(frames, ww, packed, gray)), "n * hh * ww", n, hh, ww));
    ENTER(h);
    HIPCHK(h, launch_ingest_bits(frames, order, n, hh, ww, bit_depth, packed, gray, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_egress_bits(rvdd_t* h, const float* rgb, int32_t n, int32_t H, int32_t W, int32_t order, int32_t bit_depth, int32_t pattern,
                     uint8_t* out, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (H < 2 || (H & 1)) return fail(h, RVDD_ERR_ARG, "rvdd_egress_bits: H must be even and >= 2, got %d", H);
    if (W < 2 || (W & 1)) return fail(h, RVDD_ERR_ARG, "rvdd_egress_bits: W must be even and >= 2, got %d", W);
    RC(bits_args(h, "rvdd_egress_bits", order, bit_depth, W / 2));
    RC(need_bayer(h, "rvdd_egress_bits", pattern));
    RC(need_count(h, "rvdd_egress_bits", n));
    if (n == 0) return RVDD_OK;
    if (!rgb || !out) return fail(h, RVDD_ERR_ARG, "rvdd_egress_bits: rgb and out are required");
    RC(need_blocks(h, "rvdd_egress_bits", bits_blocks(n, H / 2, W / 2, egress_bits_fast(rgb, W, out)), "n * H * W", n, H, W));
    ENTER(h);
    HIPCHK(h, launch_egress_bits(rgb, n, H, W, order, bit_depth, pattern, out, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_dpc(rvdd_t* h, const float* packed_in, float* packed_out, float* gray, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth,
             const rvdd_dpc_cfg* cfg, uint32_t* counts, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    DpcParams p;
    RC(dpc_params(h, "rvdd_dpc", cfg, &p));
    RC(need_bit_depth(h, "rvdd_dpc", bit_depth));
    RC(need_min(h, "rvdd_dpc", "hh", hh, 2, "the neighbours are mirrored about the site"));
    RC(need_min(h, "rvdd_dpc", "ww", ww, 2, "the neighbours are mirrored about the site"));
    RC(need_count(h, "rvdd_dpc", n));
    if (n == 0) return RVDD_OK;
    if (!packed_in || !packed_out) return fail(h, RVDD_ERR_ARG, "rvdd_dpc: packed_in and packed_out are required");
    RC(need_blocks(h, "rvdd_dpc", dpc_blocks(n, hh, ww, dpc_wide(packed_in, packed_out, gray, ww), nullptr), "n * hh * ww", n, hh, ww));
    // a thread reads the neighbours other threads write: in place is a race, and so is any other overlap
    const uintptr_t a = reinterpret_cast<uintptr_t>(packed_in), b = reinterpret_cast<uintptr_t>(packed_out);
    const uintptr_t bytes = (uintptr_t)n * 4 * (uintptr_t)hh * (uintptr_t)ww * sizeof(float);
    if (a < b + bytes && b < a + bytes) return fail(h, RVDD_ERR_ARG, "rvdd_dpc: packed_out must not overlap packed_in (%d frames of 4 x %d x %d floats each)", n, hh, ww);
    ENTER(h);
    HIPCHK(h, launch_dpc(packed_in, packed_out, gray, n, hh, ww, bit_depth, p, counts, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_dpc_detect(rvdd_t* h, const float* packed, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, const rvdd_dpc_detect_cfg* cfg,
                    uint32_t* hits, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_ptr(h, "rvdd_dpc_detect", cfg, "cfg"));
    DpcParams p;
    RC(dpc_params(h, "rvdd_dpc_detect", &cfg->rule, &p));
    if (cfg->tolerate < 0 || cfg->tolerate > 3) return fail(h, RVDD_ERR_ARG, "rvdd_dpc_detect: tolerate must be 0..3 (the median of eight bears three), got %d", cfg->tolerate);
    if (cfg->reserved != 0) return fail(h, RVDD_ERR_ARG, "rvdd_dpc_detect: reserved must be 0, got %d", cfg->reserved);
    RC(need_bit_depth(h, "rvdd_dpc_detect", bit_depth));
    RC(need_min(h, "rvdd_dpc_detect", "hh", hh, 2, "the neighbours are mirrored about the site"));
    RC(need_min(h, "rvdd_dpc_detect", "ww", ww, 2, "the neighbours are mirrored about the site"));
    RC(need_count(h, "rvdd_dpc_detect", n));
    RC(need_ptr(h, "rvdd_dpc_detect", hits, "hits"));
    if (reinterpret_cast<uintptr_t>(hits) & 3) return fail(h, RVDD_ERR_ARG, "rvdd_dpc_detect: hits must be 4-byte aligned (32-bit words)");
    if (n == 0) return RVDD_OK;
    RC(need_ptr(h, "rvdd_dpc_detect", packed, "packed"));
    if (dpc_detect_blocks(hh, ww, dpc_detect_wide(packed, hits, ww)) < 0)
        return fail(h, RVDD_ERR_ARG, "rvdd_dpc_detect: hh * ww = %d * %d needs a launch of more than 2^31 - 1 blocks", hh, ww);
    ENTER(h);
    HIPCHK(h, launch_dpc_detect(packed, n, hh, ww, bit_depth, p, cfg->tolerate, hits, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_dpc_map_stats(const uint8_t* cellmask, int32_t hh, int32_t ww, int64_t* out3) {
    if (!cellmask) return fail(nullptr, RVDD_ERR_ARG, "rvdd_dpc_map_stats: cellmask is required");
    if (!out3) return fail(nullptr, RVDD_ERR_ARG, "rvdd_dpc_map_stats: out3 is required");
    if (hh < 3) return fail(nullptr, RVDD_ERR_ARG, "rvdd_dpc_map_stats: hh must be >= 3 (the second ring is reflected about the edge), got %d", hh);
    if (ww < 3) return fail(nullptr, RVDD_ERR_ARG, "rvdd_dpc_map_stats: ww must be >= 3 (the second ring is reflected about the edge), got %d", ww);
    const auto reflect = [](int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; };
    int64_t samples = 0, cells = 0, unfixable = 0;
    for (int y = 0; y < hh; ++y)
        for (int x = 0; x < ww; ++x) {
            const unsigned bits = cellmask[(size_t)y * ww + x];
            if (bits & 0xf0u)
                return fail(nullptr, RVDD_ERR_ARG, "rvdd_dpc_map_stats: cellmask[%d][%d] = 0x%02x has a bit above the four planes' set", y, x, bits);
            if (!bits) continue;
            ++cells;
            for (int k = 0; k < 4; ++k) {
                if (!((bits >> k) & 1u)) continue;
                ++samples;
                bool good = false;      // a site of the 5 x 5 window, either ring, whose bit k is clear (the centre's is set)
                for (int dy = -2; dy <= 2 && !good; ++dy)
                    for (int dx = -2; dx <= 2 && !good; ++dx)
                        good = !((cellmask[(size_t)reflect(y + dy, hh) * ww + reflect(x + dx, ww)] >> k) & 1u);
                unfixable += !good;
            }
        }
    out3[0] = samples;
    out3[1] = cells;
    out3[2] = unfixable;
    return RVDD_OK;
}

int rvdd_dpc_map_apply(rvdd_t* h, float* packed, float* gray, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_bit_depth(h, "rvdd_dpc_map_apply", bit_depth));
    RC(need_min(h, "rvdd_dpc_map_apply", "hh", hh, 3, "the second ring is reflected about the edge"));
    RC(need_min(h, "rvdd_dpc_map_apply", "ww", ww, 3, "the second ring is reflected about the edge"));
    RC(need_count(h, "rvdd_dpc_map_apply", n));
    if (n > 0) RC(need_ptr(h, "rvdd_dpc_map_apply", packed, "packed"));
    const auto& m = h->dmap;
    if (!m.on) return fail(h, RVDD_ERR_STATE, "rvdd_dpc_map_apply: no map is set (rvdd_set_dpc_map)");
    if (m.hh != hh || m.ww != ww)
        return fail(h, RVDD_ERR_STATE, "rvdd_dpc_map_apply: the map is one of %d x %d cells, the frames have %d x %d", m.hh, m.ww, hh, ww);
    if (dpc_map_blocks(n, m.ncells) < 0)
        return fail(h, RVDD_ERR_ARG, "rvdd_dpc_map_apply: n = %d frames of %lld defective cells need a launch of more than 2^31 - 1 blocks", n, (long long)m.ncells);
    if (n == 0 || m.ncells == 0) return RVDD_OK;
    ENTER(h);
    HIPCHK(h, launch_dpc_map_apply(packed, gray, n, hh, ww, bit_depth, m.mask, m.cells, m.ncells, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_noise_hist(rvdd_t* h, const float* packed, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, rvdd_noise_acc* acc, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_ptr(h, "rvdd_noise_hist", acc, "acc"));
    if (reinterpret_cast<uintptr_t>(acc) & 7) return fail(h, RVDD_ERR_ARG, "rvdd_noise_hist: acc must be 8-byte aligned (its sums are 64-bit atomics)");
    RC(need_bit_depth(h, "rvdd_noise_hist", bit_depth));
    RC(need_count(h, "rvdd_noise_hist", n));
    RC(need_min(h, "rvdd_noise_hist", "hh", hh, 0));
    RC(need_min(h, "rvdd_noise_hist", "ww", ww, 0));
    const int64_t groups = noise_groups(n, hh, ww, nullptr);
    if (groups < 0)
        return fail(h, RVDD_ERR_ARG, "rvdd_noise_hist: n * hh * ww = %d * %d * %d needs a launch of more than 2^31 - 1 workgroups", n, hh, ww);
    if (groups == 0) return RVDD_OK;       // no frame, or frames smaller than one block
    RC(need_ptr(h, "rvdd_noise_hist", packed, "packed"));
    ENTER(h);
    HIPCHK(h, launch_noise_hist(packed, n, hh, ww, bit_depth, acc, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_frame_sigs(rvdd_t* h, const float* gray, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, rvdd_frame_sig* sig, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_bit_depth(h, "rvdd_frame_sigs", bit_depth));
    RC(need_min(h, "rvdd_frame_sigs", "hh", hh, 16, "16 bands of at least one row"));
    RC(need_min(h, "rvdd_frame_sigs", "ww", ww, 16, "16 columns of at least one cell"));
    RC(need_count(h, "rvdd_frame_sigs", n));
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, "rvdd_frame_sigs", {{gray, "gray"}, {sig, "sig"}}));
    if (reinterpret_cast<uintptr_t>(sig) & 7) return fail(h, RVDD_ERR_ARG, "rvdd_frame_sigs: sig must be 8-byte aligned (its sums are 64-bit words)");
    if (n > 0x7fffffff / 16) return fail(h, RVDD_ERR_ARG, "rvdd_frame_sigs: n = %d needs a launch of more than 2^31 - 1 blocks (16 per frame)", n);
    ENTER(h);
    HIPCHK(h, launch_frame_sigs(gray, n, hh, ww, bit_depth, sig, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_resid_stats(rvdd_t* h, const float* packed, const float* rgb, int32_t n, int32_t hh, int32_t ww, int32_t pattern, int32_t bit_depth,
                     rvdd_resid_acc* acc, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(need_bayer(h, "rvdd_resid_stats", pattern));
    RC(need_bit_depth(h, "rvdd_resid_stats", bit_depth));
    RC(need_min(h, "rvdd_resid_stats", "hh", hh, 1));
    RC(need_min(h, "rvdd_resid_stats", "ww", ww, 1));
    RC(need_count(h, "rvdd_resid_stats", n));
    if (reinterpret_cast<uintptr_t>(acc) & 7) return fail(h, RVDD_ERR_ARG, "rvdd_resid_stats: acc must be 8-byte aligned (its sums are 64-bit atomics)");
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, "rvdd_resid_stats", {{packed, "packed"}, {rgb, "rgb"}, {acc, "acc"}}));
    RC(need_blocks(h, "rvdd_resid_stats", resid_blocks(n, hh, ww, resid_wide(packed, rgb, ww), nullptr), "n * hh * ww", n, hh, ww));
    ENTER(h);
    HIPCHK(h, launch_resid(packed, rgb, n, hh, ww, pattern, bit_depth, acc, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_rows_estimate(rvdd_t* h, const float* packed, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, const rvdd_rows_cfg* cfg,
                       float* offsets, uint8_t* state, rvdd_rows_acc* acc, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RowsParams p;
    RC(rows_params(h, "rvdd_rows_estimate", cfg, &p));
    RC(line_shape(h, "rvdd_rows_estimate", true, n, hh, ww, bit_depth));
    if (reinterpret_cast<uintptr_t>(acc) & 7) return fail(h, RVDD_ERR_ARG, "rvdd_rows_estimate: acc must be 8-byte aligned (sum_q2 is a 64-bit atomic)");
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, "rvdd_rows_estimate", {{packed, "packed"}, {offsets, "offsets"}, {state, "state"}}));
    if (rows_estimate_blocks(n, hh) < 0)
        return fail(h, RVDD_ERR_ARG, "rvdd_rows_estimate: n * 2 * hh = %d * 2 * %d needs a launch of more than 2^31 - 1 blocks", n, hh);
    ENTER(h);
    HIPCHK(h, launch_rows_estimate(packed, n, hh, ww, bit_depth, p, offsets, state, acc, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_rows_apply(rvdd_t* h, float* packed, float* gray, const float* offsets, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    RC(line_shape(h, "rvdd_rows_apply", true, n, hh, ww, bit_depth));
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, "rvdd_rows_apply", {{packed, "packed"}, {offsets, "offsets"}}));
    RC(need_blocks(h, "rvdd_rows_apply", line_apply_blocks(n, hh, ww, line_apply_wide(ww, packed, gray), nullptr), "n * hh * ww", n, hh, ww));
    ENTER(h);
    HIPCHK(h, launch_rows_apply(packed, gray, offsets, n, hh, ww, bit_depth, static_cast<hipStream_t>(stream)));
    return RVDD_OK;
}

int rvdd_cols_estimate(rvdd_t* h, const float* packed, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, const rvdd_cols_cfg* cfg,
                       float* offsets, uint8_t* state, void* stream) {
    const char* fn = "rvdd_cols_estimate";
    if (!h) return RVDD_ERR_ARG;
    RowsParams p;
    RC(line_params(h, fn, cfg, &p));
    RC(line_shape(h, fn, false, n, hh, ww, bit_depth));
    if (hh > cols_max_hh())
        return fail(h, RVDD_ERR_ARG, "%s: hh must be <= %d (a workgroup holds the 2 hh keys of four columns in LDS), got %d", fn, cols_max_hh(), hh);
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, fn, {{packed, "packed"}, {offsets, "offsets"}, {state, "state"}}));
    if (cols_estimate_blocks(n, hh, ww) < 0)
        return fail(h, RVDD_ERR_ARG, "%s: n = %d frames of ww = %d columns need a launch of more than 2^31 - 1 blocks", fn, n, ww);
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(h, s, "cols_estimate_kernel", 0.0, (double)n * 4.0 * hh * ww * 4.0);
    HIPCHK(h, launch_cols_estimate(packed, n, hh, ww, bit_depth, p, offsets, state, s));
    return RVDD_OK;
}

int rvdd_cols_apply(rvdd_t* h, float* packed, float* gray, const float* map_dev, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, void* stream) {
    const char* fn = "rvdd_cols_apply";
    if (!h) return RVDD_ERR_ARG;
    RC(line_shape(h, fn, false, n, hh, ww, bit_depth));
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, fn, {{packed, "packed"}, {map_dev, "map_dev"}}));
    RC(need_blocks(h, fn, line_apply_blocks(n, hh, ww, line_apply_wide(ww, packed, gray, map_dev), nullptr), "n * hh * ww", n, hh, ww));
    ENTER(h);
    return run_cols_apply(h, packed, gray, map_dev, n, hh, ww, bit_depth, static_cast<hipStream_t>(stream));
}

// the shape and pattern checks of the two green calls
static int green_shape(rvdd_t* h, const char* fn, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, int32_t pattern) {
    RC(need_bit_depth(h, fn, bit_depth));
    RC(need_bayer(h, fn, pattern));
    RC(need_min(h, fn, "hh", hh, 2, "a sample's four neighbours lie in two cell rows"));
    RC(need_min(h, fn, "ww", ww, 2, "a sample's four neighbours lie in two cell columns"));
    RC(need_count(h, fn, n));
    return RVDD_OK;
}

int rvdd_green_estimate(rvdd_t* h, const float* packed, int32_t n, int32_t hh, int32_t ww, int32_t bit_depth, int32_t pattern,
                        const rvdd_green_cfg* cfg, float* e, float* level, uint8_t* state, void* stream) {
    const char* fn = "rvdd_green_estimate";
    if (!h) return RVDD_ERR_ARG;
    RowsParams p;
    RC(line_params(h, fn, cfg, &p));
    if (!std::isfinite(cfg->black)) return fail(h, RVDD_ERR_ARG, "%s: black must be finite, got %g", fn, cfg->black);
    RC(green_shape(h, fn, n, hh, ww, bit_depth, pattern));
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, fn, {{packed, "packed"}, {e, "e"}, {level, "level"}, {state, "state"}}));
    if (green_estimate_blocks(n, hh, ww) < 0)
        return fail(h, RVDD_ERR_ARG, "%s: n = %d frames of %d x %d cells need a launch of more than 2^31 - 1 blocks", fn, n, hh, ww);
    ENTER(h);
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(h, s, "green_estimate_kernel", 0.0, (double)n * 2.0 * hh * ww * 4.0);
    HIPCHK(h, launch_green_estimate(packed, n, hh, ww, bit_depth, pattern, p, e, level, state, s));
    return RVDD_OK;
}

int rvdd_green_apply(rvdd_t* h, float* packed, float* gray, const float* map_dev, int32_t gh, int32_t gw, float black, int32_t n, int32_t hh,
                     int32_t ww, int32_t bit_depth, int32_t pattern, void* stream) {
    const char* fn = "rvdd_green_apply";
    if (!h) return RVDD_ERR_ARG;
    RC(green_shape(h, fn, n, hh, ww, bit_depth, pattern));
    if (!std::isfinite(black)) return fail(h, RVDD_ERR_ARG, "%s: black must be finite, got %g", fn, (double)black);
    int fgh, fgw;
    green_grid(hh, ww, &fgh, &fgw);
    if (!(gh == 1 && gw == 1) && !(gh == fgh && gw == fgw))
        return fail(h, RVDD_ERR_ARG, "%s: the map's grid gh x gw = %d x %d is neither 1 x 1 nor the %d x %d blocks of frames of %d x %d cells", fn, gh, gw,
                    fgh, fgw, hh, ww);
    if (n == 0) return RVDD_OK;
    RC(need_ptrs(h, fn, {{packed, "packed"}, {map_dev, "map_dev"}}));
    RC(need_blocks(h, fn, line_apply_blocks(n, hh, ww, line_apply_wide(ww, packed, gray), nullptr), "n * hh * ww", n, hh, ww));
    ENTER(h);
    return run_green_apply(h, packed, gray, map_dev, gh, gw, black, n, hh, ww, bit_depth, pattern, static_cast<hipStream_t>(stream));
}

// the shape checks rvdd_unprocess and rvdd_unprocess_draws share; 0 = fine
static int unprocess_shape(rvdd_t* h, const char* fn, int32_t n, int32_t H, int32_t W) {
    if (H < 2 || (H & 1)) return fail(h, RVDD_ERR_ARG, "%s: H must be even and >= 2, got %d", fn, H);
    if (W < 2 || (W & 1)) return fail(h, RVDD_ERR_ARG, "%s: W must be even and >= 2, got %d", fn, W);
    if ((int64_t)H * W >= (1ll << 32)) return fail(h, RVDD_ERR_ARG, "%s: H * W must be below 2^32 (the draws count a frame's pixels in 32 bits), got %d x %d", fn, H, W);
    RC(need_count(h, fn, n));
    return RVDD_OK;
}

int rvdd_unprocess(rvdd_t* h, const uint8_t* srgb, int32_t n, int32_t H, int32_t W, double rgb_gain, double red_gain, double blue_gain,
                   int32_t iso, int32_t pattern, const float* dither, const float* normal, uint64_t seed, int64_t frame0, float* lin_f32,
                   uint16_t* lin_u16, float* gt_raw, float* noisy, void* stream) {
    if (!h) return RVDD_ERR_ARG;
    if (iso != 3200 && iso != 12800) return fail(h, RVDD_ERR_ARG, "rvdd_unprocess: iso must be 3200 or 12800, got %d", iso);
    RC(need_bayer(h, "rvdd_unprocess", pattern));
    RC(unprocess_shape(h, "rvdd_unprocess", n, H, W));
    if (n == 0) return RVDD_OK;
    RC(need_ptr(h, "rvdd_unprocess", srgb, "srgb"));
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

}  // extern "C"
