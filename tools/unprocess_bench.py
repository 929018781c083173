#!/usr/bin/env python3
"""Raw-dataset synthesis throughput (rvdd_unprocess) on 1280x720 frames, n = 8, all four outputs: once with the draws made in
the kernel and once with both planes supplied.  HIP events over LAUNCHES launches after warm-up.  Two JSON lines, appended to
profiles/unprocess_bench.jsonl.

Per line: microseconds per frame; the algorithmic bytes over that time (per pixel 3 B sRGB in, 12 B lin_f32 + 6 B lin_u16 +
4 B gt_raw + 4 B noisy out = 29 B with generated draws; + 12 B dither + 4 B normal in = 45 B supplied); and the two lower
bounds of the launch -- bytes over 8 TB/s, and the kernel's vector instructions over the chip's issue rate (a wave's VALU
instruction occupies its SIMD for two cycles: 256 CUs x 4 SIMDs x 32 lanes per cycle at 2.4 GHz) -- with the name of the larger.
The instruction count is the STATIC count of `v_` instructions of the wide kernel (both forms of the draws are in it, and a
transcendental costs more than one issue slot), read from the assembly hipcc writes for csrc/unprocess.hip: an estimate of what
a thread executes, named as such in the output; null where hipcc is not available."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rvdd_release_amd.ppipe import find_gains  # noqa: E402
from rvdd_release_amd.util._ops import ops_runtime  # noqa: E402

N, H, W = int(os.environ.get("BATCH", "8")), 720, 1280
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20
HBM_BYTES_PER_S = 8.0e12
VALU_LANES_PER_S = 256 * 4 * 32 * 2.4e9


def static_valu_per_thread():
    """`v_` instructions of unprocess_kernel<2> in the assembly of csrc/unprocess.hip (a thread of the wide form owns 8 pixels)."""
    src = os.path.join(REPO, "rvdd-release_amd", "csrc", "unprocess.hip")
    try:
        with tempfile.TemporaryDirectory() as tmp:
            asm = os.path.join(tmp, "unprocess.s")
            subprocess.run([os.environ.get("HIPCC", "hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                            "--cuda-device-only", "-S", src, "-o", asm], check=True, capture_output=True, timeout=300)
            text = open(asm).read()
    except (OSError, subprocess.SubprocessError):
        return None
    m = re.search(r"^(\S*unprocess_kernelILi2E\S*):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
    if not m:
        return None
    return sum(1 for line in m.group(2).splitlines() if line.startswith("\t") and line.split()[0].startswith("v_"))


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


def main():
    assert torch.cuda.is_available(), "unprocess_bench needs a GPU"
    rt = ops_runtime(0)
    lib, h = rt.lib, rt.h
    srgb = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (N, H, W, 3)).astype(np.uint8)).cuda()
    n_gain, red, blue = find_gains(7, 3200)
    dither, normal = rt.unprocess_draws(5, 0, N, H, W)
    out = rt.unprocess(srgb, 1 / n_gain, red, blue, 3200, seed=5)
    ptr = {k: v.data_ptr() for k, v in out.items()}
    stream = rt._stream()

    def launch(d, z):
        rc = lib.rvdd_unprocess(h, srgb.data_ptr(), N, H, W, 1 / n_gain, red, blue, 3200, 0, d, z, 5, 0, ptr["lin_f32"], ptr["lin_u16"],
                                ptr["gt_raw"], ptr["noisy"], stream)
        assert rc == 0, lib.rvdd_last_error(h)

    valu = static_valu_per_thread()
    px = N * H * W
    lines = []
    for mode, d, z, bpp in (("generated", None, None, 29), ("supplied", dither.data_ptr(), normal.data_ptr(), 45)):
        us = timed(lambda: launch(d, z))
        t_hbm = px * bpp / HBM_BYTES_PER_S * 1e6
        t_valu = None if valu is None else (px / 8) * valu / VALU_LANES_PER_S * 1e6      # threads x instructions = lane-instructions
        bound = "hbm" if t_valu is None or t_hbm >= t_valu else "valu"
        floor = t_hbm if bound == "hbm" else t_valu
        lines.append({"metric": "rvdd_unprocess us/frame, 1280x720, all four outputs", "draws": mode, "batch": N, "launches": LAUNCHES,
                      "us_per_frame": round(us / N, 3), "us_per_launch": round(us, 2), "frames_per_s": round(N / us * 1e6, 1),
                      "bytes_per_pixel": bpp, "achieved_GBps": round(px * bpp / us / 1e3, 1),
                      "static_valu_instructions_per_thread_of_8_pixels": valu,
                      "bound_us_per_launch": {"hbm_8TBps": round(t_hbm, 2), "valu_issue_static": None if t_valu is None else round(t_valu, 2)},
                      "bound": bound if valu is not None else "hbm (instruction count not available)",
                      "frac_of_bound": round(floor / us, 4)})
    # the outputs of the two modes are the same bits (the supplied planes are the kernel's own draws)
    again = rt.unprocess(srgb, 1 / n_gain, red, blue, 3200, dither=dither, normal=normal)
    for k in ("lin_f32", "gt_raw", "noisy"):
        assert torch.equal(out[k], again[k]), k
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "unprocess_bench.jsonl"), "a") as f:
        for line in lines:
            print(json.dumps(line))
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
