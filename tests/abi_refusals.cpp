// The refusals of librvdd_hip.so's entry points, made without a GPU: every `fail(` site of csrc/ops.hip, csrc/stream.hip and
// csrc/stages.hip that lies in front of ENTER(h), and the argument refusals of the host-only entry points (rvdd_dpc_map_stats and those of
// csrc/noise_fit.hip).  One line per case on stdout: function <TAB> case <TAB> return code <TAB> rvdd_last_error.
//
// How: the program hides every device from itself before its first HIP call, so ENTER(h) -- the first thing that touches the runtime --
// ends in RVDD_ERR_HIP "cannot select device".  A handle is a plain struct (runtime_internal.h): it is built by hand here, cfg set, finalized
// where the later checks of rvdd_video_push are wanted.  For each entry point one valid argument set is broken one argument at a time; the
// buffers are small host arrays that no refusing call dereferences (the setters and the host-only calls read their host maps: those are real).
// The expected outcome of every case is a refusal that names what was broken: a line that says "cannot select device" is a lost refusal.
// tests/test_abi_refusals_host.py compares the output with tests/golden/abi_refusals.txt, which tools/make_golden_abi_refusals.py recorded
// from the commit in front of the one that folded the checks.  Built by `make -C rvdd-release_amd/csrc abi_refusals` on a built tree.
//
// The sites BEHIND ENTER, which this program cannot reach, and what holds each:
//   rvdd_tvl1flow, rvdd_tvl1flow_batch "image too skinny for its pyramid"      tests/test_tvl1.py (match="skinny")
//   rvdd_ppipe "zero gain"                                                      by reading
//   rvdd_srgb_metrics "win_size exceeds image extent"                           by reading
//   psnr_l1_n "an asynchronous rvdd_tvl1flow_batch before this call failed"     by reading
//   rvdd_video_push, everything from the first-push block on:
//     "needs batch <= 64"                                                       by reading
//     "are not a size rvdd_tvl1flow_batch accepts"                              by reading
//     "with rvdd_set_dpc hh and ww must be >= 2"                                by reading
//     "the map of rvdd_set_dpc_map is one of"                                   by reading
//     "with rvdd_set_rows hh must be >= 5", "... ww must be <="                 by reading
//     "the map of rvdd_set_cols is one of"                                      tests/test_gpu_cols.py (match="rvdd_set_cols is one of 17 cell columns")
//     "with rvdd_set_green hh and ww must be >= 2"                              by reading
//     "the map of rvdd_set_green is one of"                                     tests/test_gpu_green.py (match="rvdd_set_green is one of 2 x 1 blocks")
//     "slot %d was idle on the last push", "slot %d has no video yet"           by reading
// Those lines stay textually as they were.
#include "runtime_internal.h"

#include <limits>

static rvdd_handle g_handle;
static rvdd_t* const H = &g_handle;
static int g_cases = 0;

static void report(const char* fn, const char* what, int rc, const char* err) {
    std::printf("%s\t%s\t%d\t%s\n", fn, what, rc, err ? err : "");
    ++g_cases;
}
// a call on the handle: its error string starts empty, so a code without a message shows as such
#define R(fn, what, ...)                                 \
    do {                                                 \
        H->err.clear();                                  \
        const int rc__ = fn(__VA_ARGS__);                \
        report(#fn, what, rc__, rvdd_last_error(H));     \
    } while (0)
// a call without a handle (host-only, or a null handle): the message is the thread's, which rvdd_create's own first refusal marks
// beforehand, so that a code without a message shows as such here too
#define R0(fn, what, ...)                                                                   \
    do {                                                                                    \
        (void)rvdd_create(nullptr, nullptr);                                                \
        const std::string mark__ = rvdd_last_error(nullptr);                                \
        const int rc__ = fn(__VA_ARGS__);                                                   \
        report(#fn, what, rc__, mark__ == rvdd_last_error(nullptr) ? "" : rvdd_last_error(nullptr)); \
    } while (0)

int main() {
    setenv("ROCR_VISIBLE_DEVICES", "", 1);
    setenv("HIP_VISIBLE_DEVICES", "", 1);
    // the buffers below are host arrays: where the hiding did not take, a lost refusal would become a launch on them -- make no call at all
    int ndev = -1;
    if (const hipError_t e = hipGetDeviceCount(&ndev); e != hipErrorNoDevice && !(e == hipSuccess && ndev == 0)) {
        std::fprintf(stderr, "abi_refusals: %d device(s) still visible (%s): nothing called\n", ndev, hipGetErrorString(e));
        return 2;
    }
    H->cfg = rvdd_cfg{RVDD_ARCH_CONVUNET_FEAT, 0, 2, 64, 96, 0};

    alignas(16) static float buf[8192];
    alignas(16) static uint8_t bytes[4096];
    float *const A = buf, *const B = buf + 4096, *const G = buf + 2048;      // two tensors 16 KiB apart, and a gray plane between them
    uint8_t* const U8 = bytes;
    int32_t its[4];
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const double dnan = std::numeric_limits<double>::quiet_NaN();
    const int32_t BIG = 0x7fffffff;

    // ---- ops.hip: losses, demosaic, warps, flows, the sRGB pipe
    float out2[4];
    R0(rvdd_psnr_l1, "h null", nullptr, A, B, 16, out2, nullptr);
    R(rvdd_psnr_l1, "den null", H, nullptr, B, 16, out2, nullptr);
    R(rvdd_psnr_l1, "gt null", H, A, nullptr, 16, out2, nullptr);
    R(rvdd_psnr_l1, "out null", H, A, B, 16, nullptr, nullptr);
    R(rvdd_psnr_l1, "count 0", H, A, B, 0, out2, nullptr);
    R0(rvdd_psnr_l1_batch, "h null", nullptr, A, B, 1, 16, out2, nullptr);
    R(rvdd_psnr_l1_batch, "den null", H, nullptr, B, 1, 16, out2, nullptr);
    R(rvdd_psnr_l1_batch, "gt null", H, A, nullptr, 1, 16, out2, nullptr);
    R(rvdd_psnr_l1_batch, "out null", H, A, B, 1, 16, nullptr, nullptr);
    R(rvdd_psnr_l1_batch, "n -1", H, A, B, -1, 16, out2, nullptr);
    R(rvdd_psnr_l1_batch, "count -1", H, A, B, 1, -1, out2, nullptr);

    R(rvdd_demosaic_ha_bayer, "pattern -1", H, A, 1, 8, 8, -1, B, nullptr);
    R(rvdd_demosaic_ha_bayer, "pattern 4", H, A, 1, 8, 8, 4, B, nullptr);
    R0(rvdd_demosaic_ha_bayer, "h null", nullptr, A, 1, 8, 8, 0, B, nullptr);
    R(rvdd_demosaic_ha_bayer, "raw null", H, nullptr, 1, 8, 8, 0, B, nullptr);
    R(rvdd_demosaic_ha_bayer, "rgb null", H, A, 1, 8, 8, 0, nullptr, nullptr);
    R(rvdd_demosaic_ha_bayer, "n -1", H, A, -1, 8, 8, 0, B, nullptr);
    R(rvdd_demosaic_ha_bayer, "hh 0", H, A, 1, 0, 8, 0, B, nullptr);
    R(rvdd_demosaic_ha_bayer, "ww 0", H, A, 1, 8, 0, 0, B, nullptr);
    R0(rvdd_demosaic_ha, "h null", nullptr, A, 1, 8, 8, B, nullptr);
    R(rvdd_demosaic_ha, "raw null", H, nullptr, 1, 8, 8, B, nullptr);
    R(rvdd_demosaic_ha, "ww 0", H, A, 1, 8, 0, B, nullptr);

    R0(rvdd_warp_bicubic, "h null", nullptr, A, G, 1, 3, 8, 8, B, nullptr);
    R(rvdd_warp_bicubic, "x null", H, nullptr, G, 1, 3, 8, 8, B, nullptr);
    R(rvdd_warp_bicubic, "flow null", H, A, nullptr, 1, 3, 8, 8, B, nullptr);
    R(rvdd_warp_bicubic, "y null", H, A, G, 1, 3, 8, 8, nullptr, nullptr);
    R(rvdd_warp_bicubic, "n -1", H, A, G, -1, 3, 8, 8, B, nullptr);
    R(rvdd_warp_bicubic, "c 0", H, A, G, 1, 0, 8, 8, B, nullptr);
    R(rvdd_warp_bicubic, "H 1", H, A, G, 1, 3, 1, 8, B, nullptr);
    R(rvdd_warp_bicubic, "W 1", H, A, G, 1, 3, 8, 1, B, nullptr);

    R0(rvdd_upsample_factor_2, "h null", nullptr, A, 1, 2, 8, 8, 2.0f, B, nullptr);
    R(rvdd_upsample_factor_2, "t null", H, nullptr, 1, 2, 8, 8, 2.0f, B, nullptr);
    R(rvdd_upsample_factor_2, "out null", H, A, 1, 2, 8, 8, 2.0f, nullptr, nullptr);
    R(rvdd_upsample_factor_2, "n -1", H, A, -1, 2, 8, 8, 2.0f, B, nullptr);
    R(rvdd_upsample_factor_2, "c 0", H, A, 1, 0, 8, 8, 2.0f, B, nullptr);
    R(rvdd_upsample_factor_2, "hh 0", H, A, 1, 2, 0, 8, 2.0f, B, nullptr);
    R(rvdd_upsample_factor_2, "ww 0", H, A, 1, 2, 8, 0, 2.0f, B, nullptr);

    R0(rvdd_tvl1flow, "h null", nullptr, A, B, G, 16, 16, its, nullptr);
    R(rvdd_tvl1flow, "I0 null", H, nullptr, B, G, 16, 16, its, nullptr);
    R(rvdd_tvl1flow, "I1 null", H, A, nullptr, G, 16, 16, its, nullptr);
    R(rvdd_tvl1flow, "u null", H, A, B, nullptr, 16, 16, its, nullptr);
    R(rvdd_tvl1flow, "nx 15", H, A, B, G, 15, 16, its, nullptr);
    R(rvdd_tvl1flow, "ny 15", H, A, B, G, 16, 15, its, nullptr);
    R0(rvdd_tvl1flow_batch, "h null", nullptr, A, B, G, 1, 16, 16, its, nullptr);
    R(rvdd_tvl1flow_batch, "I0 null", H, nullptr, B, G, 1, 16, 16, its, nullptr);
    R(rvdd_tvl1flow_batch, "I1 null", H, A, nullptr, G, 1, 16, 16, its, nullptr);
    R(rvdd_tvl1flow_batch, "u null", H, A, B, nullptr, 1, 16, 16, its, nullptr);
    R(rvdd_tvl1flow_batch, "n -1", H, A, B, G, -1, 16, 16, its, nullptr);
    R(rvdd_tvl1flow_batch, "nx 15", H, A, B, G, 1, 15, 16, its, nullptr);
    R(rvdd_tvl1flow_batch, "ny 15", H, A, B, G, 1, 16, 15, its, nullptr);

    R0(rvdd_ppipe, "h null", nullptr, A, 1, 8, 8, 192, 64, 8, 1, 12, 1.0, 1.0, 1.0, 3200, U8, B, nullptr);
    R(rvdd_ppipe, "img null", H, nullptr, 1, 8, 8, 192, 64, 8, 1, 12, 1.0, 1.0, 1.0, 3200, U8, B, nullptr);
    R(rvdd_ppipe, "out_u8 null", H, A, 1, 8, 8, 192, 64, 8, 1, 12, 1.0, 1.0, 1.0, 3200, nullptr, B, nullptr);
    R(rvdd_ppipe, "n -1", H, A, -1, 8, 8, 192, 64, 8, 1, 12, 1.0, 1.0, 1.0, 3200, U8, B, nullptr);
    R(rvdd_ppipe, "H 0", H, A, 1, 0, 8, 192, 64, 8, 1, 12, 1.0, 1.0, 1.0, 3200, U8, B, nullptr);
    R(rvdd_ppipe, "W 0", H, A, 1, 8, 0, 192, 64, 8, 1, 12, 1.0, 1.0, 1.0, 3200, U8, B, nullptr);

    double ps[2], ss[2];
    R0(rvdd_srgb_metrics, "h null", nullptr, U8, U8 + 2048, 1, 8, 8, ps, ss, nullptr);
    R(rvdd_srgb_metrics, "a null", H, nullptr, U8 + 2048, 1, 8, 8, ps, ss, nullptr);
    R(rvdd_srgb_metrics, "b null", H, U8, nullptr, 1, 8, 8, ps, ss, nullptr);
    R(rvdd_srgb_metrics, "n 0", H, U8, U8 + 2048, 0, 8, 8, ps, ss, nullptr);

    // ---- ops.hip: frames in and out
    R0(rvdd_ingest_raw, "h null", nullptr, U8, 0, 0, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "dtype 2", H, U8, 2, 0, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "dtype -1", H, U8, -1, 0, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "layout 2", H, U8, 0, 2, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "bit_depth 0", H, U8, 0, 0, 1, 8, 8, 0, A, G, nullptr);
    R(rvdd_ingest_raw, "bit_depth 17", H, U8, 0, 0, 1, 8, 8, 17, A, G, nullptr);
    R(rvdd_ingest_raw, "frames null", H, nullptr, 0, 0, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "n -1", H, U8, 0, 0, -1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "hh 0", H, U8, 0, 0, 1, 0, 8, 12, A, G, nullptr);
    R(rvdd_ingest_raw, "ww 0", H, U8, 0, 0, 1, 8, 0, 12, A, G, nullptr);

    R0(rvdd_gray_of_rgb, "h null", nullptr, A, 1, 8, 8, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "pattern 4", H, A, 1, 8, 8, 4, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "pattern -1", H, A, 1, 8, 8, -1, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "bit_depth 0", H, A, 1, 8, 8, 0, 0, G, nullptr);
    R(rvdd_gray_of_rgb, "bit_depth 17", H, A, 1, 8, 8, 0, 17, G, nullptr);
    R(rvdd_gray_of_rgb, "H 0", H, A, 1, 0, 8, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "H odd", H, A, 1, 7, 8, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "W 0", H, A, 1, 8, 0, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "W odd", H, A, 1, 8, 7, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "n -1", H, A, -1, 8, 8, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "rgb null", H, nullptr, 1, 8, 8, 0, 12, G, nullptr);
    R(rvdd_gray_of_rgb, "gray null", H, A, 1, 8, 8, 0, 12, nullptr, nullptr);

    R0(rvdd_egress, "h null", nullptr, A, 1, 8, 8, 1, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "layout 3", H, A, 1, 8, 8, 3, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "layout -1", H, A, 1, 8, 8, -1, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "dtype 2", H, A, 1, 8, 8, 1, 2, 12, 0, B, nullptr);
    R(rvdd_egress, "bit_depth 0", H, A, 1, 8, 8, 1, 0, 0, 0, B, nullptr);
    R(rvdd_egress, "bit_depth 17", H, A, 1, 8, 8, 1, 0, 17, 0, B, nullptr);
    R(rvdd_egress, "mosaic pattern 4", H, A, 1, 8, 8, 1, 0, 12, 4, B, nullptr);
    R(rvdd_egress, "packed pattern -1", H, A, 1, 8, 8, 2, 0, 12, -1, B, nullptr);
    R(rvdd_egress, "H 0", H, A, 1, 0, 8, 0, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "mosaic H odd", H, A, 1, 7, 8, 1, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "W 0", H, A, 1, 8, 0, 0, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "mosaic W odd", H, A, 1, 8, 7, 1, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "n -1", H, A, -1, 8, 8, 1, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "rgb null", H, nullptr, 1, 8, 8, 1, 0, 12, 0, B, nullptr);
    R(rvdd_egress, "out null", H, A, 1, 8, 8, 1, 0, 12, 0, nullptr, nullptr);
    R(rvdd_egress, "blocks", H, A, BIG, 8192, 8192, 1, 0, 12, 0, B, nullptr);

    R0(rvdd_ingest_bits, "h null", nullptr, U8, 0, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_bits, "hh 0", H, U8, 0, 1, 0, 8, 12, A, G, nullptr);
    R(rvdd_ingest_bits, "ww 0", H, U8, 0, 1, 8, 0, 12, A, G, nullptr);
    R(rvdd_ingest_bits, "order 2", H, U8, 2, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_bits, "bit_depth 11", H, U8, 0, 1, 8, 8, 11, A, G, nullptr);
    R(rvdd_ingest_bits, "bit_depth 16", H, U8, 1, 1, 8, 8, 16, A, G, nullptr);
    R(rvdd_ingest_bits, "MIPI 10 odd ww", H, U8, 0, 1, 8, 7, 10, A, G, nullptr);
    R(rvdd_ingest_bits, "MIPI 14 odd ww", H, U8, 0, 1, 8, 7, 14, A, G, nullptr);
    R(rvdd_ingest_bits, "n -1", H, U8, 0, -1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_bits, "frames null", H, nullptr, 0, 1, 8, 8, 12, A, G, nullptr);
    R(rvdd_ingest_bits, "blocks", H, U8, 0, BIG, 4096, 4096, 12, A, G, nullptr);

    R0(rvdd_egress_bits, "h null", nullptr, A, 1, 8, 8, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "H 0", H, A, 1, 0, 8, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "H odd", H, A, 1, 7, 8, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "W 0", H, A, 1, 8, 0, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "W odd", H, A, 1, 8, 7, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "order -1", H, A, 1, 8, 8, -1, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "bit_depth 8", H, A, 1, 8, 8, 0, 8, 0, U8, nullptr);
    R(rvdd_egress_bits, "MIPI 10 odd ww", H, A, 1, 8, 14, 0, 10, 0, U8, nullptr);
    R(rvdd_egress_bits, "pattern 4", H, A, 1, 8, 8, 0, 12, 4, U8, nullptr);
    R(rvdd_egress_bits, "pattern -1", H, A, 1, 8, 8, 0, 12, -1, U8, nullptr);
    R(rvdd_egress_bits, "n -1", H, A, -1, 8, 8, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "rgb null", H, nullptr, 1, 8, 8, 0, 12, 0, U8, nullptr);
    R(rvdd_egress_bits, "out null", H, A, 1, 8, 8, 0, 12, 0, nullptr, nullptr);
    R(rvdd_egress_bits, "blocks", H, A, BIG, 8192, 8192, 0, 12, 0, U8, nullptr);

    // ---- ops.hip: defective pixels
    const rvdd_dpc_cfg dpc{4.0f, 4.0f, 1.0f, 0.0f, 1.0f};
    uint32_t* const CNT = reinterpret_cast<uint32_t*>(G);
    auto dpc_with = [&](int field, float v) {
        rvdd_dpc_cfg c = dpc;
        (&c.k_hot)[field] = v;
        return c;
    };
    rvdd_dpc_cfg dc;
    R0(rvdd_dpc, "h null", nullptr, A, B, G, 1, 8, 8, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "cfg null", H, A, B, G, 1, 8, 8, 12, nullptr, CNT, nullptr);
    dc = dpc_with(0, -1.0f);
    R(rvdd_dpc, "k_hot -1", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    dc = dpc_with(0, inf);
    R(rvdd_dpc, "k_hot inf", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    dc = dpc_with(1, nan);
    R(rvdd_dpc, "k_dead nan", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    dc = dpc_with(2, inf);
    R(rvdd_dpc, "noise_a inf", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    dc = dpc_with(3, nan);
    R(rvdd_dpc, "noise_b nan", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    dc = dpc_with(4, 0.0f);
    R(rvdd_dpc, "var_floor 0", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    dc = dpc_with(4, inf);
    R(rvdd_dpc, "var_floor inf", H, A, B, G, 1, 8, 8, 12, &dc, CNT, nullptr);
    R(rvdd_dpc, "bit_depth 0", H, A, B, G, 1, 8, 8, 0, &dpc, CNT, nullptr);
    R(rvdd_dpc, "bit_depth 17", H, A, B, G, 1, 8, 8, 17, &dpc, CNT, nullptr);
    R(rvdd_dpc, "hh 1", H, A, B, G, 1, 1, 8, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "ww 1", H, A, B, G, 1, 8, 1, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "n -1", H, A, B, G, -1, 8, 8, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "packed_in null", H, nullptr, B, G, 1, 8, 8, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "packed_out null", H, A, nullptr, G, 1, 8, 8, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "blocks", H, A, B, G, BIG, 4096, 4096, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "in place", H, A, A, G, 1, 8, 8, 12, &dpc, CNT, nullptr);
    R(rvdd_dpc, "overlap", H, A, A + 16, G, 1, 8, 8, 12, &dpc, CNT, nullptr);

    const rvdd_dpc_detect_cfg det{dpc, 1, 0};
    rvdd_dpc_detect_cfg dt;
    R0(rvdd_dpc_detect, "h null", nullptr, A, 1, 8, 8, 12, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "cfg null", H, A, 1, 8, 8, 12, nullptr, CNT, nullptr);
    dt = det, dt.rule.k_hot = nan;
    R(rvdd_dpc_detect, "rule.k_hot nan", H, A, 1, 8, 8, 12, &dt, CNT, nullptr);
    dt = det, dt.rule.var_floor = -1.0f;
    R(rvdd_dpc_detect, "rule.var_floor -1", H, A, 1, 8, 8, 12, &dt, CNT, nullptr);
    dt = det, dt.tolerate = 4;
    R(rvdd_dpc_detect, "tolerate 4", H, A, 1, 8, 8, 12, &dt, CNT, nullptr);
    dt = det, dt.tolerate = -1;
    R(rvdd_dpc_detect, "tolerate -1", H, A, 1, 8, 8, 12, &dt, CNT, nullptr);
    dt = det, dt.reserved = 1;
    R(rvdd_dpc_detect, "reserved 1", H, A, 1, 8, 8, 12, &dt, CNT, nullptr);
    R(rvdd_dpc_detect, "bit_depth 0", H, A, 1, 8, 8, 0, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "bit_depth 17", H, A, 1, 8, 8, 17, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "hh 1", H, A, 1, 1, 8, 12, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "ww 1", H, A, 1, 8, 1, 12, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "n -1", H, A, -1, 8, 8, 12, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "hits null", H, A, 1, 8, 8, 12, &det, nullptr, nullptr);
    R(rvdd_dpc_detect, "hits unaligned", H, A, 1, 8, 8, 12, &det, reinterpret_cast<uint32_t*>(U8 + 2), nullptr);
    R(rvdd_dpc_detect, "packed null", H, nullptr, 1, 8, 8, 12, &det, CNT, nullptr);
    R(rvdd_dpc_detect, "blocks", H, A, 1, BIG, BIG, 12, &det, CNT, nullptr);

    int64_t out3[3];
    static uint8_t mask[16];      // 4 x 4 cells, clean
    R0(rvdd_dpc_map_stats, "cellmask null", nullptr, 4, 4, out3);
    R0(rvdd_dpc_map_stats, "out3 null", mask, 4, 4, nullptr);
    R0(rvdd_dpc_map_stats, "hh 2", mask, 2, 4, out3);
    R0(rvdd_dpc_map_stats, "ww 2", mask, 4, 2, out3);
    mask[6] = 0x13;
    R0(rvdd_dpc_map_stats, "bit 4 set", mask, 4, 4, out3);

    R0(rvdd_dpc_map_apply, "h null", nullptr, A, G, 1, 8, 8, 12, nullptr);
    R(rvdd_dpc_map_apply, "bit_depth 0", H, A, G, 1, 8, 8, 0, nullptr);
    R(rvdd_dpc_map_apply, "bit_depth 17", H, A, G, 1, 8, 8, 17, nullptr);
    R(rvdd_dpc_map_apply, "hh 2", H, A, G, 1, 2, 8, 12, nullptr);
    R(rvdd_dpc_map_apply, "ww 2", H, A, G, 1, 8, 2, 12, nullptr);
    R(rvdd_dpc_map_apply, "n -1", H, A, G, -1, 8, 8, 12, nullptr);
    R(rvdd_dpc_map_apply, "packed null", H, nullptr, G, 1, 8, 8, 12, nullptr);
    R(rvdd_dpc_map_apply, "no map", H, A, G, 1, 8, 8, 12, nullptr);
    H->dmap.on = true, H->dmap.hh = 8, H->dmap.ww = 8, H->dmap.ncells = 1ll << 40;      // a map by hand: only its size is read
    R(rvdd_dpc_map_apply, "map of another hh", H, A, G, 1, 9, 8, 12, nullptr);
    R(rvdd_dpc_map_apply, "map of another ww", H, A, G, 1, 8, 9, 12, nullptr);
    R(rvdd_dpc_map_apply, "blocks", H, A, G, BIG, 8, 8, 12, nullptr);
    H->dmap = {};

    // ---- ops.hip: noise curve, scene cuts, residual
    rvdd_noise_acc* const NACC = reinterpret_cast<rvdd_noise_acc*>(B);
    R0(rvdd_noise_hist, "h null", nullptr, A, 1, 64, 64, 12, NACC, nullptr);
    R(rvdd_noise_hist, "acc null", H, A, 1, 64, 64, 12, nullptr, nullptr);
    R(rvdd_noise_hist, "acc unaligned", H, A, 1, 64, 64, 12, reinterpret_cast<rvdd_noise_acc*>(buf + 1), nullptr);
    R(rvdd_noise_hist, "bit_depth 0", H, A, 1, 64, 64, 0, NACC, nullptr);
    R(rvdd_noise_hist, "bit_depth 17", H, A, 1, 64, 64, 17, NACC, nullptr);
    R(rvdd_noise_hist, "n -1", H, A, -1, 64, 64, 12, NACC, nullptr);
    R(rvdd_noise_hist, "hh -1", H, A, 1, -1, 64, 12, NACC, nullptr);
    R(rvdd_noise_hist, "ww -1", H, A, 1, 64, -1, 12, NACC, nullptr);
    R(rvdd_noise_hist, "workgroups", H, A, BIG, 8192, 8192, 12, NACC, nullptr);
    R(rvdd_noise_hist, "packed null", H, nullptr, 1, 64, 64, 12, NACC, nullptr);

    rvdd_frame_sig* const SIG = reinterpret_cast<rvdd_frame_sig*>(B);
    R0(rvdd_frame_sigs, "h null", nullptr, A, 1, 16, 16, 12, SIG, nullptr);
    R(rvdd_frame_sigs, "bit_depth 0", H, A, 1, 16, 16, 0, SIG, nullptr);
    R(rvdd_frame_sigs, "bit_depth 17", H, A, 1, 16, 16, 17, SIG, nullptr);
    R(rvdd_frame_sigs, "hh 15", H, A, 1, 15, 16, 12, SIG, nullptr);
    R(rvdd_frame_sigs, "ww 15", H, A, 1, 16, 15, 12, SIG, nullptr);
    R(rvdd_frame_sigs, "n -1", H, A, -1, 16, 16, 12, SIG, nullptr);
    R(rvdd_frame_sigs, "gray null", H, nullptr, 1, 16, 16, 12, SIG, nullptr);
    R(rvdd_frame_sigs, "sig null", H, A, 1, 16, 16, 12, nullptr, nullptr);
    R(rvdd_frame_sigs, "sig unaligned", H, A, 1, 16, 16, 12, reinterpret_cast<rvdd_frame_sig*>(buf + 1), nullptr);
    R(rvdd_frame_sigs, "blocks", H, A, BIG / 16 + 1, 16, 16, 12, SIG, nullptr);

    rvdd_resid_acc* const RACC = reinterpret_cast<rvdd_resid_acc*>(G);
    R0(rvdd_resid_stats, "h null", nullptr, A, B, 1, 8, 8, 0, 12, RACC, nullptr);
    R(rvdd_resid_stats, "pattern 4", H, A, B, 1, 8, 8, 4, 12, RACC, nullptr);
    R(rvdd_resid_stats, "pattern -1", H, A, B, 1, 8, 8, -1, 12, RACC, nullptr);
    R(rvdd_resid_stats, "bit_depth 0", H, A, B, 1, 8, 8, 0, 0, RACC, nullptr);
    R(rvdd_resid_stats, "bit_depth 17", H, A, B, 1, 8, 8, 0, 17, RACC, nullptr);
    R(rvdd_resid_stats, "hh 0", H, A, B, 1, 0, 8, 0, 12, RACC, nullptr);
    R(rvdd_resid_stats, "ww 0", H, A, B, 1, 8, 0, 0, 12, RACC, nullptr);
    R(rvdd_resid_stats, "n -1", H, A, B, -1, 8, 8, 0, 12, RACC, nullptr);
    R(rvdd_resid_stats, "acc unaligned", H, A, B, 1, 8, 8, 0, 12, reinterpret_cast<rvdd_resid_acc*>(buf + 1), nullptr);
    R(rvdd_resid_stats, "packed null", H, nullptr, B, 1, 8, 8, 0, 12, RACC, nullptr);
    R(rvdd_resid_stats, "rgb null", H, A, nullptr, 1, 8, 8, 0, 12, RACC, nullptr);
    R(rvdd_resid_stats, "acc null", H, A, B, 1, 8, 8, 0, 12, nullptr, nullptr);
    R(rvdd_resid_stats, "blocks", H, A, B, BIG, 4096, 4096, 0, 12, RACC, nullptr);

    // ---- ops.hip: the map onto the checkpoint's curve
    const rvdd_match_cfg mc{1.5f, 0.01f};
    rvdd_match_cfg mb;
    R0(rvdd_match_raw, "h null", nullptr, A, B, 1, 8, 8, &mc, nullptr);
    R(rvdd_match_raw, "cfg null", H, A, B, 1, 8, 8, nullptr, nullptr);
    mb = {0.0f, 0.0f};
    R(rvdd_match_raw, "scale 0", H, A, B, 1, 8, 8, &mb, nullptr);
    mb = {inf, 0.0f};
    R(rvdd_match_raw, "scale inf", H, A, B, 1, 8, 8, &mb, nullptr);
    mb = {1.0f, nan};
    R(rvdd_match_raw, "offset nan", H, A, B, 1, 8, 8, &mb, nullptr);
    R(rvdd_match_raw, "n -1", H, A, B, -1, 8, 8, &mc, nullptr);
    R(rvdd_match_raw, "hh 0", H, A, B, 1, 0, 8, &mc, nullptr);
    R(rvdd_match_raw, "ww 0", H, A, B, 1, 8, 0, &mc, nullptr);
    R(rvdd_match_raw, "packed_in null", H, nullptr, B, 1, 8, 8, &mc, nullptr);
    R(rvdd_match_raw, "packed_out null", H, A, nullptr, 1, 8, 8, &mc, nullptr);
    R(rvdd_match_raw, "blocks", H, A, B, BIG, 8192, 8192, &mc, nullptr);
    R(rvdd_match_raw, "overlap", H, A, A + 4, 1, 8, 8, &mc, nullptr);
    R0(rvdd_unmatch_rgb, "h null", nullptr, A, B, 1, 8, 8, &mc, nullptr);
    R(rvdd_unmatch_rgb, "cfg null", H, A, B, 1, 8, 8, nullptr, nullptr);
    mb = {-1.0f, 0.0f};
    R(rvdd_unmatch_rgb, "scale -1", H, A, B, 1, 8, 8, &mb, nullptr);
    mb = {1.0f, inf};
    R(rvdd_unmatch_rgb, "offset inf", H, A, B, 1, 8, 8, &mb, nullptr);
    R(rvdd_unmatch_rgb, "n -1", H, A, B, -1, 8, 8, &mc, nullptr);
    R(rvdd_unmatch_rgb, "H 0", H, A, B, 1, 0, 8, &mc, nullptr);
    R(rvdd_unmatch_rgb, "W 0", H, A, B, 1, 8, 0, &mc, nullptr);
    R(rvdd_unmatch_rgb, "rgb_in null", H, nullptr, B, 1, 8, 8, &mc, nullptr);
    R(rvdd_unmatch_rgb, "rgb_out null", H, A, nullptr, 1, 8, 8, &mc, nullptr);
    R(rvdd_unmatch_rgb, "blocks", H, A, B, BIG, 8192, 8192, &mc, nullptr);
    R(rvdd_unmatch_rgb, "overlap", H, A, A + 4, 1, 8, 8, &mc, nullptr);

    // ---- ops.hip: row and column noise
    const rvdd_rows_cfg rows{3.0f, 1.0f, 0.0f, 1.0f, 8.0f};
    auto rows_with = [&](int field, float v) {
        rvdd_rows_cfg c = rows;
        (&c.k_gate)[field] = v;
        return c;
    };
    rvdd_rows_cfg rc;
    uint8_t* const ST = U8;
    rvdd_rows_acc* const WACC = reinterpret_cast<rvdd_rows_acc*>(bytes + 1024);
    R0(rvdd_rows_estimate, "h null", nullptr, A, 1, 8, 8, 12, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "cfg null", H, A, 1, 8, 8, 12, nullptr, B, ST, WACC, nullptr);
    rc = rows_with(0, 0.0f);
    R(rvdd_rows_estimate, "k_gate 0", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    rc = rows_with(0, inf);
    R(rvdd_rows_estimate, "k_gate inf", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    rc = rows_with(1, nan);
    R(rvdd_rows_estimate, "noise_a nan", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    rc = rows_with(2, inf);
    R(rvdd_rows_estimate, "noise_b inf", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    rc = rows_with(3, 0.0f);
    R(rvdd_rows_estimate, "var_floor 0", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    rc = rows_with(4, 0.0f);
    R(rvdd_rows_estimate, "max_dn 0", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    rc = rows_with(4, nan);
    R(rvdd_rows_estimate, "max_dn nan", H, A, 1, 8, 8, 12, &rc, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "bit_depth 0", H, A, 1, 8, 8, 0, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "bit_depth 17", H, A, 1, 8, 8, 17, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "hh 4", H, A, 1, 4, 8, 12, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "ww 0", H, A, 1, 8, 0, 12, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "ww too wide", H, A, 1, 8, rows_max_ww() + 1, 12, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "n -1", H, A, -1, 8, 8, 12, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "acc unaligned", H, A, 1, 8, 8, 12, &rows, B, ST, reinterpret_cast<rvdd_rows_acc*>(bytes + 1028), nullptr);
    R(rvdd_rows_estimate, "packed null", H, nullptr, 1, 8, 8, 12, &rows, B, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "offsets null", H, A, 1, 8, 8, 12, &rows, nullptr, ST, WACC, nullptr);
    R(rvdd_rows_estimate, "state null", H, A, 1, 8, 8, 12, &rows, B, nullptr, WACC, nullptr);
    R(rvdd_rows_estimate, "blocks", H, A, BIG, 8, 8, 12, &rows, B, ST, WACC, nullptr);

    R0(rvdd_rows_apply, "h null", nullptr, A, G, B, 1, 8, 8, 12, nullptr);
    R(rvdd_rows_apply, "bit_depth 0", H, A, G, B, 1, 8, 8, 0, nullptr);
    R(rvdd_rows_apply, "bit_depth 17", H, A, G, B, 1, 8, 8, 17, nullptr);
    R(rvdd_rows_apply, "hh 4", H, A, G, B, 1, 4, 8, 12, nullptr);
    R(rvdd_rows_apply, "ww 0", H, A, G, B, 1, 8, 0, 12, nullptr);
    R(rvdd_rows_apply, "ww too wide", H, A, G, B, 1, 8, rows_max_ww() + 1, 12, nullptr);
    R(rvdd_rows_apply, "n -1", H, A, G, B, -1, 8, 8, 12, nullptr);
    R(rvdd_rows_apply, "packed null", H, nullptr, G, B, 1, 8, 8, 12, nullptr);
    R(rvdd_rows_apply, "offsets null", H, A, G, nullptr, 1, 8, 8, 12, nullptr);
    R(rvdd_rows_apply, "blocks", H, A, G, B, BIG, 1 << 20, 64, 12, nullptr);

    const rvdd_cols_cfg cols{3.0f, 1.0f, 0.0f, 1.0f};
    rvdd_cols_cfg cc;
    R0(rvdd_cols_estimate, "h null", nullptr, A, 1, 8, 8, 12, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "cfg null", H, A, 1, 8, 8, 12, nullptr, B, ST, nullptr);
    cc = cols, cc.k_gate = -1.0f;
    R(rvdd_cols_estimate, "k_gate -1", H, A, 1, 8, 8, 12, &cc, B, ST, nullptr);
    cc = cols, cc.noise_a = inf;
    R(rvdd_cols_estimate, "noise_a inf", H, A, 1, 8, 8, 12, &cc, B, ST, nullptr);
    cc = cols, cc.noise_b = nan;
    R(rvdd_cols_estimate, "noise_b nan", H, A, 1, 8, 8, 12, &cc, B, ST, nullptr);
    cc = cols, cc.var_floor = nan;
    R(rvdd_cols_estimate, "var_floor nan", H, A, 1, 8, 8, 12, &cc, B, ST, nullptr);
    R(rvdd_cols_estimate, "bit_depth 0", H, A, 1, 8, 8, 0, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "bit_depth 17", H, A, 1, 8, 8, 17, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "ww 4", H, A, 1, 8, 4, 12, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "hh 0", H, A, 1, 0, 8, 12, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "n -1", H, A, -1, 8, 8, 12, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "hh too tall", H, A, 1, cols_max_hh() + 1, 8, 12, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "packed null", H, nullptr, 1, 8, 8, 12, &cols, B, ST, nullptr);
    R(rvdd_cols_estimate, "offsets null", H, A, 1, 8, 8, 12, &cols, nullptr, ST, nullptr);
    R(rvdd_cols_estimate, "state null", H, A, 1, 8, 8, 12, &cols, B, nullptr, nullptr);
    R(rvdd_cols_estimate, "blocks", H, A, BIG, 8, 1 << 20, 12, &cols, B, ST, nullptr);

    R0(rvdd_cols_apply, "h null", nullptr, A, G, B, 1, 8, 8, 12, nullptr);
    R(rvdd_cols_apply, "bit_depth 0", H, A, G, B, 1, 8, 8, 0, nullptr);
    R(rvdd_cols_apply, "bit_depth 17", H, A, G, B, 1, 8, 8, 17, nullptr);
    R(rvdd_cols_apply, "ww 4", H, A, G, B, 1, 8, 4, 12, nullptr);
    R(rvdd_cols_apply, "hh 0", H, A, G, B, 1, 0, 8, 12, nullptr);
    R(rvdd_cols_apply, "n -1", H, A, G, B, -1, 8, 8, 12, nullptr);
    R(rvdd_cols_apply, "packed null", H, nullptr, G, B, 1, 8, 8, 12, nullptr);
    R(rvdd_cols_apply, "map_dev null", H, A, G, nullptr, 1, 8, 8, 12, nullptr);
    R(rvdd_cols_apply, "blocks", H, A, G, B, BIG, 4096, 4096, 12, nullptr);

    // ---- ops.hip: green imbalance
    const rvdd_green_cfg green{3.0f, 1.0f, 0.0f, 1.0f, 64.0f};
    rvdd_green_cfg gc;
    float* const LV = buf + 1024;
    R0(rvdd_green_estimate, "h null", nullptr, A, 1, 8, 8, 12, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "cfg null", H, A, 1, 8, 8, 12, 0, nullptr, B, LV, ST, nullptr);
    gc = green, gc.k_gate = nan;
    R(rvdd_green_estimate, "k_gate nan", H, A, 1, 8, 8, 12, 0, &gc, B, LV, ST, nullptr);
    gc = green, gc.noise_a = nan;
    R(rvdd_green_estimate, "noise_a nan", H, A, 1, 8, 8, 12, 0, &gc, B, LV, ST, nullptr);
    gc = green, gc.noise_b = inf;
    R(rvdd_green_estimate, "noise_b inf", H, A, 1, 8, 8, 12, 0, &gc, B, LV, ST, nullptr);
    gc = green, gc.var_floor = -1.0f;
    R(rvdd_green_estimate, "var_floor -1", H, A, 1, 8, 8, 12, 0, &gc, B, LV, ST, nullptr);
    gc = green, gc.black = inf;
    R(rvdd_green_estimate, "black inf", H, A, 1, 8, 8, 12, 0, &gc, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "bit_depth 0", H, A, 1, 8, 8, 0, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "bit_depth 17", H, A, 1, 8, 8, 17, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "pattern 4", H, A, 1, 8, 8, 12, 4, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "pattern -1", H, A, 1, 8, 8, 12, -1, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "hh 1", H, A, 1, 1, 8, 12, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "ww 1", H, A, 1, 8, 1, 12, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "n -1", H, A, -1, 8, 8, 12, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "packed null", H, nullptr, 1, 8, 8, 12, 0, &green, B, LV, ST, nullptr);
    R(rvdd_green_estimate, "e null", H, A, 1, 8, 8, 12, 0, &green, nullptr, LV, ST, nullptr);
    R(rvdd_green_estimate, "level null", H, A, 1, 8, 8, 12, 0, &green, B, nullptr, ST, nullptr);
    R(rvdd_green_estimate, "state null", H, A, 1, 8, 8, 12, 0, &green, B, LV, nullptr, nullptr);
    R(rvdd_green_estimate, "blocks", H, A, BIG, 8192, 8192, 12, 0, &green, B, LV, ST, nullptr);

    R0(rvdd_green_apply, "h null", nullptr, A, G, B, 1, 1, 64.0f, 1, 8, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "bit_depth 0", H, A, G, B, 1, 1, 64.0f, 1, 8, 8, 0, 0, nullptr);
    R(rvdd_green_apply, "bit_depth 17", H, A, G, B, 1, 1, 64.0f, 1, 8, 8, 17, 0, nullptr);
    R(rvdd_green_apply, "pattern 4", H, A, G, B, 1, 1, 64.0f, 1, 8, 8, 12, 4, nullptr);
    R(rvdd_green_apply, "hh 1", H, A, G, B, 1, 1, 64.0f, 1, 1, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "ww 1", H, A, G, B, 1, 1, 64.0f, 1, 8, 1, 12, 0, nullptr);
    R(rvdd_green_apply, "n -1", H, A, G, B, 1, 1, 64.0f, -1, 8, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "black nan", H, A, G, B, 1, 1, nan, 1, 8, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "grid 2 x 1 of a 1 x 1 frame", H, A, G, B, 2, 1, 64.0f, 1, 8, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "grid 2 x 2 of a 2 x 3 frame", H, A, G, B, 2, 2, 64.0f, 1, 40, 70, 12, 0, nullptr);
    R(rvdd_green_apply, "packed null", H, nullptr, G, B, 1, 1, 64.0f, 1, 8, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "map_dev null", H, A, G, nullptr, 1, 1, 64.0f, 1, 8, 8, 12, 0, nullptr);
    R(rvdd_green_apply, "blocks", H, A, G, B, 1, 1, 64.0f, BIG, 4096, 4096, 12, 0, nullptr);

    // ---- ops.hip: raw datasets from sRGB video
    uint16_t* const U16 = reinterpret_cast<uint16_t*>(bytes + 2048);
    R0(rvdd_unprocess, "h null", nullptr, U8, 1, 8, 8, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "iso 100", H, U8, 1, 8, 8, 1.0, 1.0, 1.0, 100, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "pattern 4", H, U8, 1, 8, 8, 1.0, 1.0, 1.0, 3200, 4, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "pattern -1", H, U8, 1, 8, 8, 1.0, 1.0, 1.0, 12800, -1, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "H odd", H, U8, 1, 7, 8, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "H 0", H, U8, 1, 0, 8, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "W odd", H, U8, 1, 8, 7, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "H * W 2^32", H, U8, 1, 65536, 65536, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "n -1", H, U8, -1, 8, 8, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "srgb null", H, nullptr, 1, 8, 8, 1.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "rgb_gain 0", H, U8, 1, 8, 8, 0.0, 1.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "red_gain 0", H, U8, 1, 8, 8, 1.0, 0.0, 1.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R(rvdd_unprocess, "blue_gain 0", H, U8, 1, 8, 8, 1.0, 1.0, 0.0, 3200, 0, nullptr, nullptr, 1, 0, A, U16, B, G, nullptr);
    R0(rvdd_unprocess_draws, "h null", nullptr, 1, 0, 1, 8, 8, A, B, nullptr);
    R(rvdd_unprocess_draws, "H odd", H, 1, 0, 1, 7, 8, A, B, nullptr);
    R(rvdd_unprocess_draws, "W 0", H, 1, 0, 1, 8, 0, A, B, nullptr);
    R(rvdd_unprocess_draws, "H * W 2^32", H, 1, 0, 1, 65536, 65536, A, B, nullptr);
    R(rvdd_unprocess_draws, "n -1", H, 1, 0, -1, 8, 8, A, B, nullptr);

    // ---- stages.hip: the setters and readers of the push's stages
    R0(rvdd_set_dpc, "h null", nullptr, &dpc);
    dc = dpc_with(0, nan);
    R(rvdd_set_dpc, "k_hot nan", H, &dc);
    dc = dpc_with(1, -1.0f);
    R(rvdd_set_dpc, "k_dead -1", H, &dc);
    dc = dpc_with(2, nan);
    R(rvdd_set_dpc, "noise_a nan", H, &dc);
    dc = dpc_with(3, inf);
    R(rvdd_set_dpc, "noise_b inf", H, &dc);
    dc = dpc_with(4, 0.0f);
    R(rvdd_set_dpc, "var_floor 0", H, &dc);

    static uint8_t cellmask[16];
    R0(rvdd_set_dpc_map, "h null", nullptr, cellmask, 4, 4);
    R(rvdd_set_dpc_map, "hh 2", H, cellmask, 2, 4);
    R(rvdd_set_dpc_map, "ww 2", H, cellmask, 4, 2);
    R(rvdd_set_dpc_map, "hh * ww 2^31", H, cellmask, 65536, 32768);
    cellmask[9] = 0x80;
    R(rvdd_set_dpc_map, "bit 7 set", H, cellmask, 4, 4);

    R0(rvdd_set_match, "h null", nullptr, &mc);
    mb = {0.0f, 0.0f};
    R(rvdd_set_match, "scale 0", H, &mb);
    mb = {nan, 0.0f};
    R(rvdd_set_match, "scale nan", H, &mb);
    mb = {1.0f, inf};
    R(rvdd_set_match, "offset inf", H, &mb);

    float colmap[16] = {};
    R0(rvdd_set_cols, "h null", nullptr, colmap, 8);
    R(rvdd_set_cols, "ww 4", H, colmap, 4);
    colmap[11] = nan;
    R(rvdd_set_cols, "map[1][3] nan", H, colmap, 8);

    float gmap[6] = {};
    R0(rvdd_set_green, "h null", nullptr, gmap, 2, 3, 64.0f);
    R(rvdd_set_green, "gh 0", H, gmap, 0, 3, 64.0f);
    R(rvdd_set_green, "gw 0", H, gmap, 2, 0, 64.0f);
    R(rvdd_set_green, "black nan", H, gmap, 2, 3, nan);
    gmap[4] = inf;
    R(rvdd_set_green, "map[1][1] inf", H, gmap, 2, 3, 64.0f);

    R0(rvdd_set_rows, "h null", nullptr, &rows);
    rc = rows_with(0, nan);
    R(rvdd_set_rows, "k_gate nan", H, &rc);
    rc = rows_with(1, inf);
    R(rvdd_set_rows, "noise_a inf", H, &rc);
    rc = rows_with(2, nan);
    R(rvdd_set_rows, "noise_b nan", H, &rc);
    rc = rows_with(3, -1.0f);
    R(rvdd_set_rows, "var_floor -1", H, &rc);
    rc = rows_with(4, inf);
    R(rvdd_set_rows, "max_dn inf", H, &rc);

    rvdd_rows_acc racc;
    R0(rvdd_rows_read, "h null", nullptr, 0, &racc, nullptr);
    R(rvdd_rows_read, "host_out null", H, 0, nullptr, nullptr);
    R(rvdd_rows_read, "slot -1", H, -1, &racc, nullptr);
    R(rvdd_rows_read, "slot 2 of 2", H, 2, &racc, nullptr);
    R0(rvdd_set_resid, "h null", nullptr, 1);
    static rvdd_resid_acc sacc;
    R0(rvdd_resid_read, "h null", nullptr, 0, &sacc, nullptr);
    R(rvdd_resid_read, "host_out null", H, 0, nullptr, nullptr);
    R(rvdd_resid_read, "slot -1", H, -1, &sacc, nullptr);
    R(rvdd_resid_read, "slot 2 of 2", H, 2, &sacc, nullptr);
    uint64_t hd[4];
    R0(rvdd_dpc_counts, "h null", nullptr, hd, nullptr);
    R(rvdd_dpc_counts, "hot_dead null", H, nullptr, nullptr);

    // ---- stream.hip: the push, up to ENTER
    uint8_t ctl[2] = {RVDD_PUSH_FIRST, RVDD_PUSH_FIRST}, valid[2];
    R0(rvdd_video_push, "h null", nullptr, U8, 0, 0, 12, ctl, A, valid, nullptr);
    R(rvdd_video_push, "dtype 2", H, U8, 2, 0, 12, ctl, A, valid, nullptr);
    R(rvdd_video_push, "layout 2", H, U8, 0, 2, 12, ctl, A, valid, nullptr);
    R(rvdd_video_push, "bit_depth 0", H, U8, 0, 0, 0, ctl, A, valid, nullptr);
    R(rvdd_video_push, "bit_depth 17", H, U8, 0, 0, 17, ctl, A, valid, nullptr);
    R(rvdd_video_push, "frames null", H, nullptr, 0, 0, 12, ctl, A, valid, nullptr);
    R(rvdd_video_push, "out_rgb null", H, U8, 0, 0, 12, ctl, nullptr, valid, nullptr);
    R(rvdd_video_push, "valid null", H, U8, 0, 0, 12, ctl, A, nullptr, nullptr);
    R(rvdd_video_push, "not finalized", H, U8, 0, 0, 12, ctl, A, valid, nullptr);
    H->finalized = true;
    ctl[1] = 3;
    R(rvdd_video_push, "ctl[1] 3", H, U8, 0, 0, 12, ctl, A, valid, nullptr);
    ctl[1] = RVDD_PUSH_FIRST;
    H->opt.stream_container = 1 + RVDD_BITS_MIPI;
    R(rvdd_video_push, "container dtype f32", H, U8, 1, 0, 12, ctl, A, valid, nullptr);
    R(rvdd_video_push, "container layout packed", H, U8, 0, 1, 12, ctl, A, valid, nullptr);
    R(rvdd_video_push, "container bit_depth 16", H, U8, 0, 0, 16, ctl, A, valid, nullptr);
    H->cfg.width = 34;
    R(rvdd_video_push, "container MIPI 10 odd ww", H, U8, 0, 0, 10, ctl, A, valid, nullptr);
    H->opt.stream_container = 1 + RVDD_BITS_MSB;
    H->finalized = false;
    R(rvdd_video_push, "container MSB 10 odd ww not finalized", H, U8, 0, 0, 10, ctl, A, valid, nullptr);
    H->cfg.width = 96;
    H->opt.stream_container = 0;

    // ---- noise_fit.hip: the fits on the host
    static rvdd_noise_acc nacc;
    rvdd_noise_curve curve;
    R0(rvdd_noise_fit, "acc null", nullptr, 12, &curve);
    R0(rvdd_noise_fit, "out null", &nacc, 12, nullptr);
    R0(rvdd_noise_fit, "bit_depth 0", &nacc, 0, &curve);
    R0(rvdd_noise_fit, "bit_depth 17", &nacc, 17, &curve);
    R0(rvdd_noise_fit, "no blocks", &nacc, 12, &curve);
    rvdd_resid_report rep;
    R0(rvdd_resid_fit, "acc null", nullptr, 12, 1.0, 0.0, &rep);
    R0(rvdd_resid_fit, "out null", &sacc, 12, 1.0, 0.0, nullptr);
    R0(rvdd_resid_fit, "bit_depth 0", &sacc, 0, 1.0, 0.0, &rep);
    R0(rvdd_resid_fit, "bit_depth 17", &sacc, 17, 1.0, 0.0, &rep);
    R0(rvdd_resid_fit, "a nan", &sacc, 12, dnan, 0.0, &rep);
    R0(rvdd_resid_fit, "b nan", &sacc, 12, 1.0, dnan, &rep);
    R0(rvdd_resid_fit, "no samples", &sacc, 12, 1.0, 0.0, &rep);

    const rvdd_cols_fit_cfg cfit{2, 3.0f, 8.0f};
    rvdd_cols_fit_cfg cf;
    float fmap[16];
    uint8_t fstate[16] = {}, mstate[16];
    R0(rvdd_cols_fit, "offsets null", nullptr, fstate, 1, 8, &cfit, fmap, mstate, nullptr);
    R0(rvdd_cols_fit, "state null", colmap, nullptr, 1, 8, &cfit, fmap, mstate, nullptr);
    R0(rvdd_cols_fit, "fit_cfg null", colmap, fstate, 1, 8, nullptr, fmap, mstate, nullptr);
    R0(rvdd_cols_fit, "map null", colmap, fstate, 1, 8, &cfit, nullptr, mstate, nullptr);
    R0(rvdd_cols_fit, "mstate null", colmap, fstate, 1, 8, &cfit, fmap, nullptr, nullptr);
    R0(rvdd_cols_fit, "F 0", colmap, fstate, 0, 8, &cfit, fmap, mstate, nullptr);
    R0(rvdd_cols_fit, "ww 0", colmap, fstate, 1, 0, &cfit, fmap, mstate, nullptr);
    cf = cfit, cf.k_sig = -1.0f;
    R0(rvdd_cols_fit, "k_sig -1", colmap, fstate, 1, 8, &cf, fmap, mstate, nullptr);
    cf = cfit, cf.max_dn = 0.0f;
    R0(rvdd_cols_fit, "max_dn 0", colmap, fstate, 1, 8, &cf, fmap, mstate, nullptr);

    const rvdd_green_fit_cfg gfit{2, 3.0f, 0.1f, 16.0f};
    rvdd_green_fit_cfg gf;
    float ge[6] = {}, gl[6] = {};
    R0(rvdd_green_fit, "e null", nullptr, gl, fstate, 1, 2, 3, 64.0f, &gfit, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "level null", ge, nullptr, fstate, 1, 2, 3, 64.0f, &gfit, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "state null", ge, gl, nullptr, 1, 2, 3, 64.0f, &gfit, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "fit_cfg null", ge, gl, fstate, 1, 2, 3, 64.0f, nullptr, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "map null", ge, gl, fstate, 1, 2, 3, 64.0f, &gfit, nullptr, mstate, nullptr);
    R0(rvdd_green_fit, "mstate null", ge, gl, fstate, 1, 2, 3, 64.0f, &gfit, fmap, nullptr, nullptr);
    R0(rvdd_green_fit, "F 0", ge, gl, fstate, 0, 2, 3, 64.0f, &gfit, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "gh 0", ge, gl, fstate, 1, 0, 3, 64.0f, &gfit, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "gw 0", ge, gl, fstate, 1, 2, 0, 64.0f, &gfit, fmap, mstate, nullptr);
    R0(rvdd_green_fit, "black nan", ge, gl, fstate, 1, 2, 3, nan, &gfit, fmap, mstate, nullptr);
    gf = gfit, gf.k_sig = nan;
    R0(rvdd_green_fit, "k_sig nan", ge, gl, fstate, 1, 2, 3, 64.0f, &gf, fmap, mstate, nullptr);
    gf = gfit, gf.max_gain = 0.0f;
    R0(rvdd_green_fit, "max_gain 0", ge, gl, fstate, 1, 2, 3, 64.0f, &gf, fmap, mstate, nullptr);
    gf = gfit, gf.min_signal = inf;
    R0(rvdd_green_fit, "min_signal inf", ge, gl, fstate, 1, 2, 3, 64.0f, &gf, fmap, mstate, nullptr);

    static rvdd_frame_sig sa, sb;
    double d2[2];
    R0(rvdd_cut_score, "a null", nullptr, &sb, 16, 16, d2);
    R0(rvdd_cut_score, "b null", &sa, nullptr, 16, 16, d2);
    R0(rvdd_cut_score, "out2 null", &sa, &sb, 16, 16, nullptr);
    R0(rvdd_cut_score, "hh 15", &sa, &sb, 15, 16, d2);
    R0(rvdd_cut_score, "ww 15", &sa, &sb, 16, 15, d2);
    R0(rvdd_cut_score, "a of no frame", &sa, &sb, 16, 16, d2);

    rvdd_match_cfg mo;
    double st[2];
    R0(rvdd_match_coeffs, "out null", 1.0, 0.0, 12, 1.0, 0.0, nullptr, st);
    R0(rvdd_match_coeffs, "a 0", 0.0, 0.0, 12, 1.0, 0.0, &mo, st);
    R0(rvdd_match_coeffs, "a nan", dnan, 0.0, 12, 1.0, 0.0, &mo, st);
    R0(rvdd_match_coeffs, "b nan", 1.0, dnan, 12, 1.0, 0.0, &mo, st);
    R0(rvdd_match_coeffs, "bit_depth 0", 1.0, 0.0, 0, 1.0, 0.0, &mo, st);
    R0(rvdd_match_coeffs, "bit_depth 17", 1.0, 0.0, 17, 1.0, 0.0, &mo, st);
    R0(rvdd_match_coeffs, "a_ref -1", 1.0, 0.0, 12, -1.0, 0.0, &mo, st);
    R0(rvdd_match_coeffs, "b_ref nan", 1.0, 0.0, 12, 1.0, dnan, &mo, st);
    R0(rvdd_match_coeffs, "no f32 holds it", 1e-300, 0.0, 12, 1e300, 0.0, &mo, st);

    std::fprintf(stderr, "%d cases\n", g_cases);
    return 0;
}
