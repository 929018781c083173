#!/usr/bin/env python3
"""What the green equilibration's kernels cost.

    python tools/green_bench.py [SIZE CONTENT]    rvdd_green_estimate and rvdd_green_apply beside rvdd_cols_estimate and rvdd_cols_apply in
                                                  one process, LAUNCHES (200) launches after 20 each, at 1280x720 with n = 16 and at
                                                  3840x2160 with n = 4, on a "scene" (a ramp over 10 .. 85 % of the range with the noise of
                                                  the ISO 3200 curve and 3 % of green imbalance) and on a "flat" frame (every sample the same
                                                  value: every d equal, every gain zero -- the apply then leaves its cells after the map's
                                                  loads).  SIZE (720 or 2160) and CONTENT (scene or flat) run that one case alone, for a
                                                  `rocprofv3 --kernel-trace --stats -- python tools/green_bench.py 720 scene` whose
                                                  per-kernel averages then are that case's; rvdd_timer_start / rvdd_timer_stop_ms time the
                                                  launches either way.

Prints its lines and appends them to profiles/green_kernel.txt (or the file named by GREEN_BENCH_OUT)."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20


def main(argv):
    import torch
    import kernel_resources
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import cols_cfg, cols_fit, dpc_iso_curve, green_cfg, green_fit
    from rvdd_release_amd.util._ops import ops_runtime
    assert torch.cuda.is_available(), "green_bench needs a GPU"
    only = (int(argv[0]), argv[1]) if len(argv) == 2 else None
    rt = ops_runtime(0)
    table = {r["name"]: r for r in kernel_resources.kernel_table(_lib.LIB_PATH)}
    a, b = dpc_iso_curve(3200, 12)
    black = b / a
    gen = torch.Generator(device="cuda").manual_seed(1)
    rule, cols = green_cfg(3.0, a, b, 1.0), cols_cfg(3.0, a, b, 1.0)
    lines = ["green_bench: %d launches after %d; %s" % (LAUNCHES, WARMUP, "; ".join(
        "%s: %d vgpr, %d sgpr, %d B scratch, %d B static LDS" % (k, r.get("vgpr_count", 0), r.get("sgpr_count", 0), r.get("private_segment_fixed_size", 0),
                                                                 r.get("group_segment_fixed_size", 0)) for k, r in sorted(table.items()) if k.startswith("green_")))]
    for N, H, W in ((16, 720, 1280), (4, 2160, 3840)):
        hh, ww = H // 2, W // 2
        for content in ("scene", "flat"):
            if only is not None and only != (H, content):
                continue
            if content == "scene":
                m = (0.10 + 0.75 * torch.linspace(0, 1, W, device="cuda"))[None, None, :].expand(N, H, W) * 4095
                m = m.clone()
                m[:, 0::2, 0::2] += 0.015 * (m[:, 0::2, 0::2] - black)      # GBRG: plane A up, plane B down by half of 3 %
                m[:, 1::2, 1::2] -= 0.015 * (m[:, 1::2, 1::2] - black)
                dn = (m + (a * m - b).clamp(min=0).sqrt() * torch.randn(N, H, W, device="cuda", generator=gen)).round().clamp(0, 4095)
            else:
                dn = torch.full((N, H, W), 1824.0, device="cuda")
            mosaic = dn.to(torch.int16)
            packed, gray = rt.ingest_raw(mosaic, 12, "mosaic")
            e, level, state = rt.green_estimate(packed, rule, 12, "gbrg")
            gmap_host, mstate, stats = green_fit(e, level, state, black, (N + 1) // 2, 0.0, 0.10, 4095.0 / 64.0)      # k_sig = 0: every supported block
            gmap = torch.from_numpy(gmap_host).cuda()
            offsets, cstate = rt.cols_estimate(packed, cols, 12)
            cmap = torch.from_numpy(cols_fit(offsets, cstate, (N + 1) // 2, 0.0, 4095.0 / 64.0)[0]).cuda()
            work, work_gray = packed.clone(), gray.clone()
            gh, gw = gmap_host.shape

            def timed(fn):
                for _ in range(WARMUP):
                    fn()
                rt.timer_start()
                for _ in range(LAUNCHES):
                    fn()
                return rt.timer_stop_ms() * 1e3 / LAUNCHES        # us per launch

            def ok(rc):
                assert rc == 0, rt.lib.rvdd_last_error(rt.h)

            def g_estimate():
                ok(rt.lib.rvdd_green_estimate(rt.h, packed.data_ptr(), N, hh, ww, 12, 0, ctypes.byref(rule), e.data_ptr(), level.data_ptr(),
                                              state.data_ptr(), rt._stream()))

            def g_apply():                                        # in place, the same map again and again: the same traffic each time
                ok(rt.lib.rvdd_green_apply(rt.h, work.data_ptr(), work_gray.data_ptr(), gmap.data_ptr(), gh, gw, black, N, hh, ww, 12, 0, rt._stream()))

            def c_estimate():
                ok(rt.lib.rvdd_cols_estimate(rt.h, packed.data_ptr(), N, hh, ww, 12, ctypes.byref(cols), offsets.data_ptr(), cstate.data_ptr(), rt._stream()))

            def c_apply():
                ok(rt.lib.rvdd_cols_apply(rt.h, work.data_ptr(), work_gray.data_ptr(), cmap.data_ptr(), N, hh, ww, 12, rt._stream()))

            for name, fn, cell_bytes in (("rvdd_cols_estimate (packed -> offsets)", c_estimate, 16), ("rvdd_green_estimate (two planes -> e, level)", g_estimate, 8),
                                         ("rvdd_cols_apply (packed, gray in place)", c_apply, 40), ("rvdd_green_apply (two planes, gray in place)", g_apply, 28)):
                runs = [timed(fn) for _ in range(3)]              # three timings: the spread beside the figure
                us = sorted(runs)[1]
                lines.append("%dx%d n=%-2d %-6s %-46s %8.2f us/frame  %8.1f us/launch (three runs: %s)  %7.1f GB/s of %d B/cell"
                             % (W, H, N, content, name, us / N, us, " / ".join("%.1f" % r for r in runs), N * hh * ww * cell_bytes / us / 1e3, cell_bytes))
            torch.cuda.synchronize()
            lines.append("%dx%d n=%-2d %-6s last frame: %d applied, %d skipped of %d blocks; the map: %d blocks with a gain, rms %.5f, flat estimate %.5f"
                         % (W, H, N, content, int(state[N - 1].eq(1).sum()), int(state[N - 1].eq(0).sum()), gh * gw, int((gmap_host != 0).sum()),
                            float((gmap_host.astype("float64") ** 2).mean() ** 0.5), stats["flat_gain"]))
    path = os.environ.get("GREEN_BENCH_OUT", os.path.join(REPO, "profiles", "green_kernel.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


if __name__ == '__main__':
    main(sys.argv[1:])
