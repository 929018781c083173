#!/usr/bin/env python3
"""What scene-cut detection costs.

    python tools/cuts_bench.py                    the kernel: rvdd_frame_sigs beside rvdd_ingest_raw (a u16 mosaic in, gray out) in one
                                                  process, rvdd_timer_start / rvdd_timer_stop_ms over LAUNCHES (200) launches after 20, at
                                                  1280x720 with n = 16 and at 3840x2160 with n = 4, on a "scene" (a ramp over 10 .. 85 % of
                                                  the range with the noise of the ISO 3200 curve: some fifty level bins) and on a "flat"
                                                  frame (every cell the same value: one level bin, the case equal keys would contend in)
    python tools/cuts_bench.py --denoise [OTHER]  `denoise` end to end on a tree of two 1280x720 videos of 24 frames, two shots each, written
                                                  to a temporary directory: without --cuts and with --cuts auto, alternating ROUNDS (3)
                                                  times, each run a fresh process; OTHER: the root of another checkout (the parent commit's,
                                                  built) whose `denoise` without the flag runs in every round as well

Prints its lines and appends them to profiles/cuts_kernel.txt / profiles/cuts_denoise.txt (or the file named by CUTS_BENCH_OUT)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20
ROUNDS = int(os.environ.get("ROUNDS", "3"))


def emit(lines, name):
    path = os.environ.get("CUTS_BENCH_OUT", os.path.join(REPO, "profiles", name))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


def kernel():
    import torch
    import kernel_resources
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import FRAME_SIG_BYTES, dpc_iso_curve, frame_sig_arrays
    from rvdd_release_amd.util._ops import ops_runtime
    assert torch.cuda.is_available(), "cuts_bench needs a GPU"
    rt = ops_runtime(0)
    rows = {r["name"]: r for r in kernel_resources.kernel_table(_lib.LIB_PATH)}
    a, b = dpc_iso_curve(3200, 12)
    gen = torch.Generator(device="cuda").manual_seed(1)
    lines = ["cuts_bench: %d launches after %d; %s" % (LAUNCHES, WARMUP, "; ".join(
        "%s: %d vgpr, %d sgpr, %d B scratch, %d B LDS" % (k, r.get("vgpr_count", 0), r.get("sgpr_count", 0), r.get("private_segment_fixed_size", 0),
                                                          r.get("group_segment_fixed_size", 0)) for k, r in rows.items() if k.startswith("frame_sig_kernel")))]
    for N, H, W in ((16, 720, 1280), (4, 2160, 3840)):
        hh, ww = H // 2, W // 2
        ramp = (0.10 + 0.75 * torch.linspace(0, 1, H, device="cuda"))[None, :, None].expand(N, H, W)
        for content in ("scene", "flat"):
            if content == "scene":
                m = ramp * 4095
                dn = (m + (a * m - b).clamp(min=0).sqrt() * torch.randn(N, H, W, device="cuda", generator=gen)).round().clamp(0, 4095)
            else:
                dn = torch.full((N, H, W), 1824.0, device="cuda")
            mosaic = dn.to(torch.int16)
            _, gray = rt.ingest_raw(mosaic, 12, "mosaic", want_packed=False)
            sig = torch.empty(N, FRAME_SIG_BYTES, dtype=torch.uint8, device="cuda")

            def timed(fn):
                for _ in range(WARMUP):
                    fn()
                rt.timer_start()
                for _ in range(LAUNCHES):
                    fn()
                return rt.timer_stop_ms() * 1e3 / LAUNCHES        # us per launch

            def ingest():
                rc = rt.lib.rvdd_ingest_raw(rt.h, mosaic.data_ptr(), _lib.RAW_U16, _lib.RAW_MOSAIC, N, hh, ww, 12, None, gray.data_ptr(), rt._stream())
                assert rc == 0, rt.lib.rvdd_last_error(rt.h)

            def sigs():
                rc = rt.lib.rvdd_frame_sigs(rt.h, gray.data_ptr(), N, hh, ww, 12, sig.data_ptr(), rt._stream())
                assert rc == 0, rt.lib.rvdd_last_error(rt.h)

            for name, fn, cell_bytes in (("rvdd_ingest_raw (u16 mosaic -> gray)", ingest, 8 + 4), ("rvdd_frame_sigs (gray -> signatures)", sigs, 4)):
                runs = [timed(fn) for _ in range(3)]              # three timings: the spread beside the figure
                us = sorted(runs)[1]
                lines.append("%dx%d n=%-2d %-6s %-38s %8.2f us/frame  %8.1f us/launch (three runs: %s)  %7.1f GB/s of %d B/cell"
                             % (W, H, N, content, name, us / N, us, " / ".join("%.1f" % r for r in runs), N * hh * ww * cell_bytes / us / 1e3, cell_bytes))
            torch.cuda.synchronize()
            arrays = frame_sig_arrays(sig)
            assert int(arrays["hist"][N - 1].sum()) == hh * ww
            lines.append("%dx%d n=%-2d %-6s %d level bins in use in the last frame, %d cells per band"
                         % (W, H, N, content, int((arrays["hist"][N - 1].sum(axis=0) > 0).sum()), hh * ww // 16))
    emit(lines, "cuts_kernel.txt")


def write_tree(root, videos=2, shots=2, frames=12, H=720, W=1280):
    """<root>/noisy/<video>/<frame>.tif: uint16 mosaics, every video `shots` shots of `frames` frames -- a level, two ramps and a slow wave
    that drifts 3 pixels per frame, the noise of the ISO 3200 curve; the levels of neighbouring shots lie far apart"""
    from rvdd_release_amd import tiffio
    from rvdd_release_amd.runtime import dpc_iso_curve
    a, b = dpc_iso_curve(3200, 12)
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for v in range(videos):
        os.makedirs(os.path.join(root, "noisy", "%03d" % v))
        for s in range(shots):
            level, tilt = (0.18, 0.25) if (s + v) % 2 == 0 else (0.55, -0.2)
            for t in range(frames):
                m = (level + tilt * (y / H - 0.5) * 0.4 + 0.05 * x / W + 0.04 * np.sin((x + 3 * t) * (2 * np.pi / 400) + s)) * 4095
                dn = np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0)) * rng.standard_normal(m.shape, dtype=np.float32)), 0, 4095)
                tiffio.write(os.path.join(root, "noisy", "%03d" % v, "%08d.tif" % (s * frames + t)), dn.astype(np.uint16))


def denoise(other):
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(REPO, "weights", "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--nFolder", "noisy", "--batch_size", "2", "--all_frames"]
    lines = ["cuts_bench --denoise: 2 videos of 24 frames of 1280x720 (two shots of 12 each), uint16 mosaic TIFFs, recurrent-convunet+feat-iso3200, "
             "batch 2, --all_frames, f32 output files; each run a fresh process; alternating, %d rounds" % ROUNDS]
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp)
        runs = ([("parent, no flag      ", other, [])] if other else []) + [("this tree, no flag   ", REPO, []), ("this tree, --cuts auto", REPO, ["--cuts", "auto"])]
        for r in range(ROUNDS):
            for k, (name, repo, more) in enumerate(runs):
                res = os.path.join(tmp, "res_%d_%d" % (r, k))
                p = subprocess.run([sys.executable, "-m", "rvdd_release_amd.denoise", "--dataroot", tmp, "--results_dir", res] + flags + more,
                                   cwd=repo, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, p.stderr[-2000:]
                told = re.search(r"\(denoise, (\d+) frames, ([0-9.]+) s, ([0-9.]+) frames/s\)", p.stdout)
                extra = "  ".join(ln for ln in p.stdout.splitlines() if ln.startswith("cuts:"))
                lines.append("%s: %s frames, %s s streaming, %s frames/s  %s" % (name, told.group(1), told.group(2), told.group(3), extra))
    emit(lines, "cuts_denoise.txt")


if __name__ == "__main__":
    if "--denoise" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--denoise"]
        denoise(os.path.abspath(rest[0]) if rest else None)
    else:
        kernel()
