#!/usr/bin/env python3
"""What the residual report costs.

    python tools/resid_bench.py              the kernel: rvdd_resid_stats beside rvdd_unmatch_rgb (the other pass over out_rgb a push may
                                             make) in one process, rvdd_timer_start / rvdd_timer_stop_ms over LAUNCHES (200) launches after
                                             20, at 1280x720 with n = 16 and at 3840x2160 with n = 4, on a "scene" (outputs that ramp over
                                             10 .. 85 % of the range, the noise of the ISO 3200 curve in the noisy frames: some fifty level
                                             bins) and on a "flat" frame (every output the same value: ONE bin, the case equal bins contend in)
    python tools/resid_bench.py --denoise    `denoise` end to end on a tree of two 1280x720 videos of 24 frames written to a temporary
                                             directory: without --report and with --report FILE --report_noise iso3200, alternating ROUNDS
                                             (3) times, each run a fresh process of this tree

Prints its lines and appends them to profiles/resid_kernel.txt / profiles/resid_denoise.txt (or the file named by RESID_BENCH_OUT)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20
ROUNDS = int(os.environ.get("ROUNDS", "3"))


def emit(lines, name):
    path = os.environ.get("RESID_BENCH_OUT", os.path.join(REPO, "profiles", name))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


def kernel():
    import torch
    import kernel_resources
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import dpc_iso_curve, match_cfg, resid_acc_arrays
    from rvdd_release_amd.util._ops import ops_runtime
    assert torch.cuda.is_available(), "resid_bench needs a GPU"
    rt = ops_runtime(0)
    rows = {r["name"]: r for r in kernel_resources.kernel_table(_lib.LIB_PATH)}
    a, b = dpc_iso_curve(3200, 12)
    gen = torch.Generator(device="cuda").manual_seed(1)
    cfg = match_cfg(0.5, 0.1)
    lines = ["resid_bench: %d launches after %d; %s" % (LAUNCHES, WARMUP, "; ".join(
        "%s: %d vgpr, %d sgpr, %d B scratch, %d B LDS" % (k, r.get("vgpr_count", 0), r.get("sgpr_count", 0), r.get("private_segment_fixed_size", 0),
                                                          r.get("group_segment_fixed_size", 0)) for k, r in rows.items() if k.startswith("resid_kernel")))]
    for N, H, W in ((16, 720, 1280), (4, 2160, 3840)):
        hh, ww = H // 2, W // 2
        for content in ("scene", "flat"):
            if content == "scene":
                level = (0.10 + 0.75 * torch.linspace(0, 1, H, device="cuda"))[None, None, :, None].expand(N, 3, H, W)
            else:
                level = torch.full((N, 3, H, W), 0.4453, device="cuda")
            rgb = (2 * level - 1).contiguous()
            mosaic = torch.stack([rgb[:, (1, 2, 0, 1)[k], (k >> 1)::2, (k & 1)::2] for k in range(4)], 1)      # GBRG
            packed = mosaic.clone()
            if content == "scene":
                m = (mosaic + 1) * 0.5 * 4095
                packed = 2 * ((m + (a * m - b).clamp(min=0).sqrt() * torch.randn(m.shape, device="cuda", generator=gen)) / 4095) - 1
            packed = packed.contiguous()
            acc = torch.zeros(N, 384, dtype=torch.int64, device="cuda")
            back = torch.empty_like(rgb)

            def timed(fn):
                for _ in range(WARMUP):
                    fn()
                rt.timer_start()
                for _ in range(LAUNCHES):
                    fn()
                return rt.timer_stop_ms() * 1e3 / LAUNCHES        # us per launch

            def resid():
                rc = rt.lib.rvdd_resid_stats(rt.h, packed.data_ptr(), rgb.data_ptr(), N, hh, ww, 0, 12, acc.data_ptr(), rt._stream())
                assert rc == 0, rt.lib.rvdd_last_error(rt.h)

            def unmatch():
                rc = rt.lib.rvdd_unmatch_rgb(rt.h, rgb.data_ptr(), back.data_ptr(), N, H, W, ctypes.byref(cfg), rt._stream())
                assert rc == 0, rt.lib.rvdd_last_error(rt.h)

            for name, fn, cell_bytes in (("rvdd_unmatch_rgb (out_rgb -> out_rgb)", unmatch, 96), ("rvdd_resid_stats (noisy, out_rgb -> sums)", resid, 64)):
                runs = [timed(fn) for _ in range(3)]              # three timings: the spread beside the figure
                us = sorted(runs)[1]
                lines.append("%dx%d n=%-2d %-6s %-42s %8.2f us/frame  %8.1f us/launch (three runs: %s)  %7.1f GB/s of %d B/cell"
                             % (W, H, N, content, name, us / N, us, " / ".join("%.1f" % r for r in runs), N * hh * ww * cell_bytes / us / 1e3, cell_bytes))
            torch.cuda.synchronize()
            arrays = resid_acc_arrays(acc)
            launches = 3 * (WARMUP + LAUNCHES)
            assert int(arrays["n"][N - 1].sum()) == launches * 4 * hh * ww
            lines.append("%dx%d n=%-2d %-6s %d level bins in use in the last frame" % (W, H, N, content, int((arrays["n"][N - 1] > 0).sum())))
    emit(lines, "resid_kernel.txt")


def denoise():
    from cuts_bench import write_tree
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(REPO, "weights", "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--nFolder", "noisy", "--batch_size", "2", "--all_frames"]
    lines = ["resid_bench --denoise: 2 videos of 24 frames of 1280x720, uint16 mosaic TIFFs, recurrent-convunet+feat-iso3200, batch 2, --all_frames, "
             "f32 output files; each run a fresh process of this tree; alternating, %d rounds" % ROUNDS]
    fps = {}
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp)
        runs = [("no flag ", []), ("--report", ["--report", os.path.join(tmp, "report.jsonl"), "--report_noise", "iso3200"])]
        for r in range(ROUNDS):
            for k, (name, more) in enumerate(runs):
                res = os.path.join(tmp, "res_%d_%d" % (r, k))
                p = subprocess.run([sys.executable, "-m", "rvdd_release_amd.denoise", "--dataroot", tmp, "--results_dir", res] + flags + more,
                                   cwd=REPO, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, p.stderr[-2000:]
                told = re.search(r"\(denoise, (\d+) frames, ([0-9.]+) s, ([0-9.]+) frames/s\)", p.stdout)
                fps.setdefault(name, []).append(float(told.group(3)))
                extra = "  ".join(ln for ln in p.stdout.splitlines() if ln.startswith("report:"))
                lines.append("%s: %s frames, %s s streaming, %s frames/s  %s" % (name, told.group(1), told.group(2), told.group(3), extra))
        lines.append("first video's line: " + open(os.path.join(tmp, "report.jsonl")).readline().strip())
    for name, v in fps.items():
        lines.append("%s: %.2f .. %.2f frames/s over %d runs, median %.2f" % (name, min(v), max(v), len(v), sorted(v)[len(v) // 2]))
    emit(lines, "resid_denoise.txt")


if __name__ == "__main__":
    denoise() if "--denoise" in sys.argv else kernel()
