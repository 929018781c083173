#!/usr/bin/env python3
"""What the column-noise correction costs.

    python tools/cols_bench.py                    the kernels: rvdd_cols_estimate and rvdd_cols_apply beside rvdd_rows_estimate,
                                                  rvdd_rows_apply and rvdd_ingest_raw in one process, rvdd_timer_start /
                                                  rvdd_timer_stop_ms over LAUNCHES (200) launches after 20, at 1280x720 with n = 16 and at
                                                  3840x2160 with n = 4, on a "scene" (a ramp over 10 .. 85 % of the range with the noise of
                                                  the ISO 3200 curve, a static Gaussian offset of 15 DN per column and one of 15 DN per row
                                                  and frame) and on a "flat" frame (every sample the same value: every d equal, every
                                                  offset zero -- both apply kernels then leave their cells after the offsets' loads)
    python tools/cols_bench.py --denoise [OTHER]  `denoise` end to end on a tree of two 1280x720 videos of 24 frames written to a temporary
                                                  directory: without the flag, with --col_noise auto --col_noise_curve iso3200 and with
                                                  --col_noise FILE (the same map, written by the col_noise command first: the stage without
                                                  the pre-pass, which takes the process's first use of the device out of the timed stream),
                                                  alternating ROUNDS (3) times, each run a fresh process; OTHER: the root of another checkout
                                                  (the parent commit's, built) whose `denoise` without the flag runs in every round as well

Prints its lines and appends them to profiles/cols_kernel.txt / profiles/cols_denoise.txt (or the file named by COLS_BENCH_OUT)."""
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
    path = os.environ.get("COLS_BENCH_OUT", os.path.join(REPO, "profiles", name))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


def kernel():
    import torch
    import kernel_resources
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import cols_cfg, cols_fit, dpc_iso_curve, rows_cfg
    from rvdd_release_amd.util._ops import ops_runtime
    assert torch.cuda.is_available(), "cols_bench needs a GPU"
    rt = ops_runtime(0)
    table = {r["name"]: r for r in kernel_resources.kernel_table(_lib.LIB_PATH)}
    a, b = dpc_iso_curve(3200, 12)
    gen = torch.Generator(device="cuda").manual_seed(1)
    rule, rows = cols_cfg(3.0, a, b, 1.0), rows_cfg(3.0, a, b, 1.0, 4095.0 / 64.0)
    lines = ["cols_bench: %d launches after %d; %s" % (LAUNCHES, WARMUP, "; ".join(
        "%s: %d vgpr, %d sgpr, %d B scratch, %d B static LDS" % (k, r.get("vgpr_count", 0), r.get("sgpr_count", 0), r.get("private_segment_fixed_size", 0),
                                                                 r.get("group_segment_fixed_size", 0)) for k, r in sorted(table.items()) if k.startswith("cols_")))]
    for N, H, W in ((16, 720, 1280), (4, 2160, 3840)):
        hh, ww = H // 2, W // 2
        ramp = (0.10 + 0.75 * torch.linspace(0, 1, W, device="cuda"))[None, None, :].expand(N, H, W)
        for content in ("scene", "flat"):
            if content == "scene":
                m = ramp * 4095
                dn = m + (a * m - b).clamp(min=0).sqrt() * torch.randn(N, H, W, device="cuda", generator=gen)
                dn = dn + 15.0 * torch.randn(1, 1, W, device="cuda", generator=gen)
                dn = (dn + 15.0 * torch.randn(N, H, 1, device="cuda", generator=gen)).round().clamp(0, 4095)
            else:
                dn = torch.full((N, H, W), 1824.0, device="cuda")
            mosaic = dn.to(torch.int16)
            packed, gray = rt.ingest_raw(mosaic, 12, "mosaic")
            fixed = torch.empty_like(packed)
            offsets, state = rt.cols_estimate(packed, rule, 12)
            cmap_host, mstate, stats = cols_fit(offsets, state, (N + 1) // 2, 0.0, 4095.0 / 64.0)      # k_sig = 0: every supported column
            cmap = torch.from_numpy(cmap_host).cuda()
            r_offsets, r_state, r_acc = rt.rows_estimate(packed, rows, 12)
            work, work_gray = packed.clone(), gray.clone()

            def timed(fn):
                for _ in range(WARMUP):
                    fn()
                rt.timer_start()
                for _ in range(LAUNCHES):
                    fn()
                return rt.timer_stop_ms() * 1e3 / LAUNCHES        # us per launch

            def ok(rc):
                assert rc == 0, rt.lib.rvdd_last_error(rt.h)

            def ingest():
                ok(rt.lib.rvdd_ingest_raw(rt.h, mosaic.data_ptr(), _lib.RAW_U16, _lib.RAW_MOSAIC, N, hh, ww, 12, fixed.data_ptr(), work_gray.data_ptr(),
                                          rt._stream()))

            def c_estimate():
                ok(rt.lib.rvdd_cols_estimate(rt.h, packed.data_ptr(), N, hh, ww, 12, ctypes.byref(rule), offsets.data_ptr(), state.data_ptr(), rt._stream()))

            def c_apply():                                        # in place, the same map again and again: the same traffic each time
                ok(rt.lib.rvdd_cols_apply(rt.h, work.data_ptr(), work_gray.data_ptr(), cmap.data_ptr(), N, hh, ww, 12, rt._stream()))

            def r_estimate():
                ok(rt.lib.rvdd_rows_estimate(rt.h, packed.data_ptr(), N, hh, ww, 12, ctypes.byref(rows), r_offsets.data_ptr(), r_state.data_ptr(),
                                             r_acc.data_ptr(), rt._stream()))

            def r_apply():
                ok(rt.lib.rvdd_rows_apply(rt.h, work.data_ptr(), work_gray.data_ptr(), r_offsets.data_ptr(), N, hh, ww, 12, rt._stream()))

            for name, fn, cell_bytes in (("rvdd_ingest_raw (u16 mosaic -> packed, gray)", ingest, 8 + 20),
                                         ("rvdd_rows_estimate (packed -> offsets)", r_estimate, 16), ("rvdd_cols_estimate (packed -> offsets)", c_estimate, 16),
                                         ("rvdd_rows_apply (packed, gray in place)", r_apply, 40), ("rvdd_cols_apply (packed, gray in place)", c_apply, 40)):
                runs = [timed(fn) for _ in range(3)]              # three timings: the spread beside the figure
                us = sorted(runs)[1]
                lines.append("%dx%d n=%-2d %-6s %-46s %8.2f us/frame  %8.1f us/launch (three runs: %s)  %7.1f GB/s of %d B/cell"
                             % (W, H, N, content, name, us / N, us, " / ".join("%.1f" % r for r in runs), N * hh * ww * cell_bytes / us / 1e3, cell_bytes))
            torch.cuda.synchronize()
            lines.append("%dx%d n=%-2d %-6s last frame: %d applied, %d skipped columns per call; the map: %d columns with a non-zero offset of %d, "
                         "%d rows with a non-zero offset" % (W, H, N, content, int(state[N - 1].eq(1).sum()), int(state[N - 1].eq(0).sum()),
                                                            int((cmap_host != 0).sum()), cmap_host.size, int(r_offsets[N - 1].ne(0).sum())))
    emit(lines, "cols_kernel.txt")


def write_tree(root, videos=2, frames=24, H=720, W=1280, sigma_col=15.0):
    """rows_bench's tree with a static Gaussian offset of sigma_col DN per mosaic column, the same in every frame of every video"""
    import numpy as np
    from rvdd_release_amd import tiffio
    from rvdd_release_amd.runtime import dpc_iso_curve
    a, b = dpc_iso_curve(3200, 12)
    rng = np.random.default_rng(7)
    cols = sigma_col * rng.standard_normal((1, W), dtype=np.float32)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for v in range(videos):
        os.makedirs(os.path.join(root, "noisy", "%03d" % v))
        for t in range(frames):
            m = (0.3 + 0.1 * v + 0.25 * (y / H - 0.5) * 0.4 + 0.05 * x / W + 0.04 * np.sin((x + 3 * t) * (2 * np.pi / 400))) * 4095
            dn = m + np.sqrt(np.maximum(a * m - b, 0)) * rng.standard_normal(m.shape, dtype=np.float32)
            tiffio.write(os.path.join(root, "noisy", "%03d" % v, "%08d.tif" % t), np.clip(np.rint(dn + cols), 0, 4095).astype(np.uint16))


def denoise(other):
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(REPO, "weights", "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--nFolder", "noisy", "--batch_size", "2", "--all_frames"]
    lines = ["cols_bench --denoise: 2 videos of 24 frames of 1280x720 with 15 DN of static column noise, uint16 mosaic TIFFs, "
             "recurrent-convunet+feat-iso3200, batch 2, --all_frames, f32 output files; each run a fresh process; alternating, %d rounds" % ROUNDS]
    fps = {}
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp)
        made = os.path.join(tmp, "cols.tif")                   # the same map as a FILE: the stage without the pre-pass in the process
        p = subprocess.run([sys.executable, "-m", "rvdd_release_amd.col_noise", "--dataroot", tmp, "--nFolder", "noisy", "--bit_depth", "12",
                            "--col_noise_curve", "iso3200", "--out", made], cwd=REPO, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append("col_noise: " + p.stdout.strip().splitlines()[-1])
        runs = ([("parent, no flag           ", other, [])] if other else []) + [
            ("this tree, no flag        ", REPO, []), ("this tree, --col_noise auto", REPO, ["--col_noise", "auto", "--col_noise_curve", "iso3200"]),
            ("this tree, --col_noise FILE", REPO, ["--col_noise", made])]
        for r in range(ROUNDS):
            for k, (name, repo, more) in enumerate(runs):
                res = os.path.join(tmp, "res_%d_%d" % (r, k))
                p = subprocess.run([sys.executable, "-m", "rvdd_release_amd.denoise", "--dataroot", tmp, "--results_dir", res] + flags + more,
                                   cwd=repo, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, p.stderr[-2000:]
                told = re.search(r"\(denoise, (\d+) frames, ([0-9.]+) s, ([0-9.]+) frames/s\)", p.stdout)
                fps.setdefault(name, []).append(float(told.group(3)))
                extra = "  ".join(ln for ln in p.stdout.splitlines() if ln.startswith("cols:"))[:260]
                lines.append("%s: %s frames, %s s streaming, %s frames/s  %s" % (name, told.group(1), told.group(2), told.group(3), extra))
    for name, v in fps.items():
        lines.append("%s: %.2f .. %.2f frames/s over %d runs, median %.2f" % (name, min(v), max(v), len(v), sorted(v)[len(v) // 2]))
    emit(lines, "cols_denoise.txt")


if __name__ == "__main__":
    if "--denoise" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--denoise"]
        denoise(os.path.abspath(rest[0]) if rest else None)
    else:
        kernel()
