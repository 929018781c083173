#!/usr/bin/env python3
"""Time of rvdd_match_raw and rvdd_unmatch_rgb alone on 1280x720 frames (640 x 360 cells, the wide form), n = 8, in place and out of
place, beside rvdd_ingest_raw (a u16 mosaic in, both outputs) in the same process.  rvdd_timer_start / rvdd_timer_stop_ms over
LAUNCHES launches after a warm-up.  Prints one line per kernel and appends them to profiles/match_kernel.txt (or the file named by
MATCH_BENCH_OUT).

Per line: microseconds per frame, and the bytes per raw cell over that time: the map reads 16 and writes 16, the way back reads
48 and writes 48 (three planes of four sites per cell), the ingest reads 8 and writes 20."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_resources  # noqa: E402
from rvdd_release_amd import _lib  # noqa: E402
from rvdd_release_amd.runtime import match_coeffs  # noqa: E402
from rvdd_release_amd.util._ops import ops_runtime  # noqa: E402

N, H, W = int(os.environ.get("BATCH", "8")), 720, 1280
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20


def main():
    assert torch.cuda.is_available(), "match_bench needs a GPU"
    rt = ops_runtime(0)
    hh, ww = H // 2, W // 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    cfg, s, _ = match_coeffs(60.0, 60.0 * 256 - 100, 12, 3200)
    vgpr = {r["name"]: r.get("vgpr_count", 0) for r in kernel_resources.kernel_table(_lib.LIB_PATH)}
    mosaic = torch.randint(256, 4096, (N, H, W), device="cuda", generator=gen).to(torch.int16)
    packed, gray = rt.ingest_raw(mosaic, 12, "mosaic")
    mapped = torch.empty_like(packed)
    rgb = torch.rand(N, 3, H, W, device="cuda", generator=gen) * 2 - 1
    back = torch.empty_like(rgb)

    def timed(fn):
        for _ in range(WARMUP):
            fn()
        rt.timer_start()
        for _ in range(LAUNCHES):
            fn()
        return rt.timer_stop_ms() * 1e3 / LAUNCHES        # us per launch

    def ingest():
        rc = rt.lib.rvdd_ingest_raw(rt.h, mosaic.data_ptr(), _lib.RAW_U16, _lib.RAW_MOSAIC, N, hh, ww, 12, packed.data_ptr(), gray.data_ptr(), rt._stream())
        assert rc == 0, rt.lib.rvdd_last_error(rt.h)

    def match(dst):
        def fn():
            rc = rt.lib.rvdd_match_raw(rt.h, packed.data_ptr(), dst.data_ptr(), N, hh, ww, cfg, rt._stream())
            assert rc == 0, rt.lib.rvdd_last_error(rt.h)
        return fn

    def unmatch(dst):
        def fn():
            rc = rt.lib.rvdd_unmatch_rgb(rt.h, rgb.data_ptr(), dst.data_ptr(), N, H, W, cfg, rt._stream())
            assert rc == 0, rt.lib.rvdd_last_error(rt.h)
        return fn

    lines = ["match_bench: %d frames of %d x %d, scale %.6g (s = %.4f), %d launches after %d" % (N, W, H, cfg.scale, s, LAUNCHES, WARMUP)]
    # the in-place runs last: they rewrite their operand, which the timing does not mind (the map has no data-dependent path)
    for name, fn, cell_bytes, kernel in (("rvdd_ingest_raw (u16 mosaic -> packed + gray)", ingest, 8 + 20, "ingest_raw_kernel<unsigned short, 0, true>"),
                                         ("rvdd_match_raw (packed -> packed)", match(mapped), 16 + 16, "match_kernel<false, 4>"),
                                         ("rvdd_unmatch_rgb (rgb -> rgb)", unmatch(back), 48 + 48, "match_kernel<true, 4>"),
                                         ("rvdd_match_raw (in place)", match(packed), 16 + 16, "match_kernel<false, 4>"),
                                         ("rvdd_unmatch_rgb (in place)", unmatch(rgb), 48 + 48, "match_kernel<true, 4>")):
        us = timed(fn)
        lines.append("%-48s %8.2f us/frame  %8.1f us/launch of %d frames  %7.1f GB/s of %d B/cell  %s vgpr"
                     % (name, us / N, us, N, N * hh * ww * cell_bytes / us / 1e3, cell_bytes, vgpr.get(kernel)))
    torch.cuda.synchronize()
    path = os.environ.get("MATCH_BENCH_OUT", os.path.join(REPO, "profiles", "match_kernel.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


if __name__ == "__main__":
    main()
