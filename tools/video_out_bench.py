#!/usr/bin/env python3
"""What the Y4M output costs (rvdd_ycbcr, denoise --video_out), measured on the GPU, in the manner of tools/egress_bench.py.

    python tools/video_out_bench.py                    the kernels: rvdd_ycbcr at 8 and 10 bits beside rvdd_ppipe (network output in, as
                                                       `denoise` calls it: with the float image; and the uint8 image alone) in one
                                                       process, HIP events over LAUNCHES (200) launches after 20, at 1280x720 with
                                                       n = 8 and at 3840x2160 with n = 8.  Per line: microseconds per frame, the bytes
                                                       per pixel the result needs, and that byte rate.  Every launch reads the same
                                                       input again.  At 720p a launch moves 95 to 190 MiB, inside the 256 MiB Infinity
                                                       Cache: those are cache-served rates.  At 2160p it moves 854 MiB and more, so a
                                                       line is evicted before the next launch comes back to it: those stream from HBM.
    python tools/video_out_bench.py --denoise [OTHER]  `denoise` end to end, files included, on a tree of two 1280x720 videos of 24
                                                       frames written to a temporary directory: --out_format none --video_out y4m8,
                                                       --out_format f32, and --out_format f32 --srgb, alternating ROUNDS (3) times, each
                                                       run a fresh process; OTHER: the root of another checkout (the parent commit's,
                                                       built) whose --out_format f32 runs in every round as well

Prints its lines and appends them to profiles/video_out_kernel.txt / profiles/video_out_denoise.txt (or the file named by VIDEO_OUT_BENCH_OUT)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20
ROUNDS = int(os.environ.get("ROUNDS", "3"))
RENDER = "3200,1.3,1.9,1.5"


def emit(lines, name, echo=True):
    path = os.environ.get("VIDEO_OUT_BENCH_OUT") or os.path.join(REPO, "profiles", name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            if echo:
                print(ln)
            f.write(ln + "\n")


def kernel():
    import torch
    from rvdd_release_amd import _lib
    from rvdd_release_amd.util._ops import ops_runtime
    assert torch.cuda.is_available(), "video_out_bench needs a GPU"
    rt = ops_runtime(0)
    lib, h, stream = rt.lib, rt.h, rt._stream()

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / LAUNCHES            # us per launch

    lines = ["video_out_bench: HIP events over %d launches after %d, one process; bytes per pixel are what the result needs" % (LAUNCHES, WARMUP)]
    for n, H, W in ((8, 720, 1280), (8, 2160, 3840)):
        px = n * H * W
        rng = np.random.default_rng(1)
        x = torch.from_numpy(rng.uniform(-1, 1, (n, 3, H, W)).astype(np.float32)).cuda()
        u8 = torch.empty(n, H, W, 3, dtype=torch.uint8, device="cuda")
        disp = torch.empty(n, H, W, 3, device="cuda")
        y8 = torch.empty(n, H * W * 3 // 2, dtype=torch.uint8, device="cuda")
        y10 = torch.empty(n, H * W * 3 // 2, dtype=torch.int16, device="cuda")

        def ppipe(f32):
            rc = lib.rvdd_ppipe(h, x.data_ptr(), n, H, W, 3 * H * W, H * W, W, 1, _lib.PPIPE_FROM_NET, 1.0 / 1.3, 1.9, 1.5, 3200, u8.data_ptr(),
                                disp.data_ptr() if f32 else None, stream)
            assert rc == 0, lib.rvdd_last_error(h)

        def ycbcr(depth, out):
            rc = lib.rvdd_ycbcr(h, disp.data_ptr(), n, H, W, depth, out.data_ptr(), stream)
            assert rc == 0, lib.rvdd_last_error(h)

        for name, fn, bpp in (("rvdd_ppipe, uint8 and float image (as --video_out calls it)", lambda: ppipe(True), 12 + 3 + 12),
                              ("rvdd_ppipe, uint8 image alone (as --srgb calls it)", lambda: ppipe(False), 12 + 3),
                              ("rvdd_ycbcr, 8 bits", lambda: ycbcr(8, y8), 12 + 1.5), ("rvdd_ycbcr, 10 bits", lambda: ycbcr(10, y10), 12 + 3)):
            us = timed(fn)
            lines.append("%dx%d, n = %d: %-62s %8.2f us/frame  %5.1f B/px  %7.1f GB/s  (%.0f MiB per launch: %s)"
                         % (W, H, n, name, us / n, bpp, px * bpp / us / 1e3, px * bpp / 2 ** 20,
                            "inside the 256 MiB Infinity Cache, a cache-served rate" if px * bpp <= 256 * 2 ** 20 else "streams from HBM"))
    emit(lines, "video_out_kernel.txt")


def write_tree(root, videos=2, T=24, H=720, W=1280):
    """uint16 mosaic TIFFs of a smooth scene that moves, with the noise of the ISO 3200 curve"""
    from rvdd_release_amd import tiffio
    a, b = 2.5, 600.0
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    for v in range(videos):
        os.makedirs(os.path.join(root, "noisy", "%03d" % v))
        rng = np.random.default_rng(40 + v)
        for t in range(T):
            m = (0.3 + 0.1 * v + 0.25 * (y / H - 0.5) * 0.4 + 0.05 * x / W + 0.04 * np.sin((x + 3 * t) * (2 * np.pi / 400))) * 4095
            dn = np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0)) * rng.standard_normal(m.shape, dtype=np.float32)), 0, 4095)
            tiffio.write(os.path.join(root, "noisy", "%03d" % v, "%08d.tif" % t), dn.astype(np.uint16))


def tree_bytes(path):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, files in os.walk(path) for f in files)


def denoise(other):
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(REPO, "weights", "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--nFolder", "noisy", "--batch_size", "2"]
    lines = ["video_out_bench --denoise: 2 videos of 24 frames of 1280x720, uint16 mosaic TIFFs, recurrent-convunet+feat-iso3200, batch 2; results in a "
             "temporary directory; each run a fresh process; alternating, %d rounds" % ROUNDS]
    runs = ([("parent, --out_format f32                   ", other, ["--out_format", "f32"])] if other else []) + [
        ("this tree, --out_format f32                ", REPO, ["--out_format", "f32"]),
        ("this tree, --out_format f32 --srgb         ", REPO, ["--out_format", "f32", "--srgb", RENDER]),
        ("this tree, --out_format none --video_out y4m8", REPO, ["--out_format", "none", "--video_out", "y4m8", "--video_render", RENDER])]
    fps = {}
    print(lines[0], flush=True)                      # every line as it comes: a run takes a while
    with tempfile.TemporaryDirectory() as tmp:
        write_tree(tmp)
        for r in range(ROUNDS):
            for k, (name, repo, more) in enumerate(runs):
                res = os.path.join(tmp, "res_%d_%d" % (r, k))
                p = subprocess.run([sys.executable, "-m", "rvdd_release_amd.denoise", "--dataroot", tmp, "--results_dir", res] + flags + more,
                                   cwd=repo, capture_output=True, text=True, timeout=600)
                assert p.returncode == 0, p.stderr[-2000:]
                told = re.search(r"\(denoise, (\d+) frames, ([0-9.]+) s, ([0-9.]+) frames/s\)", p.stdout)
                fps.setdefault(name, []).append(float(told.group(3)))
                lines.append("%s: %s frames, %s s, %s frames/s, %.1f MiB written" % (name, told.group(1), told.group(2), told.group(3), tree_bytes(res) / 2 ** 20))
                print(lines[-1], flush=True)
    for name, v in fps.items():
        lines.append("%s: %.2f .. %.2f frames/s over %d runs, median %.2f" % (name, min(v), max(v), len(v), sorted(v)[len(v) // 2]))
        print(lines[-1], flush=True)
    emit(lines, "video_out_denoise.txt", echo=False)


if __name__ == "__main__":
    if "--denoise" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--denoise"]
        denoise(os.path.abspath(rest[0]) if rest else None)
    else:
        kernel()
