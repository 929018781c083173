#!/usr/bin/env python3
"""Time of rvdd_noise_hist alone on 1280x720 frames (640 x 360 cells, the wide form), n = 8, beside rvdd_dpc and rvdd_ingest_raw (a
u16 mosaic in, both outputs) in the same process.  rvdd_timer_start / rvdd_timer_stop_ms over LAUNCHES launches after a warm-up.
Two contents: "scene" -- a 12-bit ramp over 10 .. 85 % of the range with the noise of the ISO 3200 curve, whose blocks spread over
some forty mean bins -- and "flat" -- one level with that noise, whose 14400 blocks per frame all share one mean bin and a few dozen
variance sub-bins: the contention case of the histogram's atomics.  Prints one line per kernel and content and appends them to
profiles/noise_kernel.txt (or the file named by NOISE_BENCH_OUT).

Per line: microseconds per frame, and the bytes per raw cell over that time: the histogram reads 16 and writes next to nothing,
the correction reads 16 and writes 16, the ingest reads 8 and writes 20."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_resources  # noqa: E402
from rvdd_release_amd import _lib  # noqa: E402
from rvdd_release_amd.runtime import NOISE_ACC_BYTES, dpc_cfg, dpc_iso_curve, noise_acc_arrays, noise_fit  # noqa: E402
from rvdd_release_amd.util._ops import ops_runtime  # noqa: E402

N, H, W = int(os.environ.get("BATCH", "8")), 720, 1280
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20


def main():
    assert torch.cuda.is_available(), "noise_bench needs a GPU"
    rt = ops_runtime(0)
    hh, ww = H // 2, W // 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    a, b = dpc_iso_curve(3200, 12)
    cfg = dpc_cfg(4, 4, a, b)
    vgpr = {r["name"]: r.get("vgpr_count", 0) for r in kernel_resources.kernel_table(_lib.LIB_PATH)}
    ramp = (0.10 + 0.75 * torch.linspace(0, 1, H, device="cuda"))[None, :, None].expand(N, H, W)
    lines = []
    for content, level in (("scene", ramp), ("flat", torch.full((N, H, W), 0.4453125, device="cuda"))):
        m = level * 4095
        dn = (m + (a * m - b).clamp(min=0).sqrt() * torch.randn(N, H, W, device="cuda", generator=gen)).round().clamp(0, 4095)
        mosaic = dn.to(torch.int16)
        packed, gray = rt.ingest_raw(mosaic, 12, "mosaic")
        out = torch.empty_like(packed)
        counts = torch.zeros(N, 2, dtype=torch.int32, device="cuda")
        acc = torch.zeros(NOISE_ACC_BYTES // 4, dtype=torch.int32, device="cuda")

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

        def dpc():
            rc = rt.lib.rvdd_dpc(rt.h, packed.data_ptr(), out.data_ptr(), gray.data_ptr(), N, hh, ww, 12, cfg, counts.data_ptr(), rt._stream())
            assert rc == 0, rt.lib.rvdd_last_error(rt.h)

        def noise():
            rc = rt.lib.rvdd_noise_hist(rt.h, packed.data_ptr(), N, hh, ww, 12, acc.data_ptr(), rt._stream())
            assert rc == 0, rt.lib.rvdd_last_error(rt.h)

        for name, fn, cell_bytes, kernel in (("rvdd_ingest_raw (u16 mosaic -> packed + gray)", ingest, 8 + 20, "ingest_raw_kernel<unsigned short, 0, true>"),
                                             ("rvdd_dpc (packed -> packed, gray patched, counts)", dpc, 16 + 16, "dpc_kernel<4>"),
                                             ("rvdd_noise_hist (packed -> accumulator)", noise, 16, "noise_hist_kernel<true>")):
            us = timed(fn)
            lines.append("%-6s %-52s %8.2f us/frame  %8.1f us/launch of %d frames  %7.1f GB/s of %d B/cell  %s vgpr"
                         % (content, name, us / N, us, N, N * hh * ww * cell_bytes / us / 1e3, cell_bytes, vgpr.get(kernel)))
        torch.cuda.synchronize()
        arrays = noise_acc_arrays(acc)
        keys, bins = int((arrays["hist"] > 0).sum()), int((arrays["hist"].sum(axis=1) > 0).sum())
        try:
            fit = noise_fit(acc, 12)
            told = "fit a = %.4f b = %.2f (the curve drawn: %.4f, %.2f)" % (fit["a"], fit["b"], a, b)
        except RuntimeError as err:
            told = "fit refused: %s" % str(err).split(": ", 2)[-1][:60]
        lines.append("%-6s %d blocks per launch in %d distinct keys of %d mean bins; %s" % (content, int(arrays["counters"][0]) // (LAUNCHES + WARMUP), keys, bins, told))
    path = os.environ.get("NOISE_BENCH_OUT", os.path.join(REPO, "profiles", "noise_kernel.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


if __name__ == "__main__":
    main()
