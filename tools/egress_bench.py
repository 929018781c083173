#!/usr/bin/env python3
"""Throughput of rvdd_egress on 1280x720 frames, n = 8, for the six (layout, sample type) pairs, and of rvdd_ingest_raw (a u16
mosaic in, both outputs) in the same process as the yardstick: the project's existing streaming kernel of the same kind.  HIP
events over LAUNCHES launches after a warm-up.  Seven JSON lines, appended to profiles/egress_bench.jsonl.

Per line: microseconds per frame and two byte rates over that time.
  algorithmic_GBps  the bytes the result needs: RGB_HWC reads 12 B/px and writes 6 (u16) or 12 (f32); a mosaic layout uses 4 B/px
                    of its input and writes 2 or 4; ingest reads 2 B/px and writes 4 + 1.
  fetched_GBps      the bytes the loads ask for: the same, except that a mosaic layout fetches 8 B/px -- each site's colour comes
                    from a 16-byte vector whose other half is another colour's site (the cache line is fetched either way).
Each egress line carries its algorithmic rate as a fraction of the yardstick's."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rvdd_release_amd import _lib  # noqa: E402
from rvdd_release_amd.util._ops import ops_runtime  # noqa: E402

N, H, W = int(os.environ.get("BATCH", "8")), 720, 1280
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20
BIT_DEPTH = 12


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
    assert torch.cuda.is_available(), "egress_bench needs a GPU"
    rt = ops_runtime(0)
    lib, h, stream = rt.lib, rt.h, rt._stream()
    px = N * H * W
    rng = np.random.default_rng(1)
    rgb = torch.from_numpy(rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)).cuda()
    mosaic = torch.from_numpy(rng.integers(0, 4096, (N, H, W), dtype=np.uint16).view(np.int16)).cuda()
    packed = torch.empty(N, 4, H // 2, W // 2, device="cuda")
    gray = torch.empty(N, H // 2, W // 2, device="cuda")

    def ingest():
        rc = lib.rvdd_ingest_raw(h, mosaic.data_ptr(), _lib.RAW_U16, _lib.RAW_MOSAIC, N, H // 2, W // 2, BIT_DEPTH, packed.data_ptr(),
                                 gray.data_ptr(), stream)
        assert rc == 0, lib.rvdd_last_error(h)

    def line(name, us, algo_bpp, fetch_bpp, **more):
        return {"metric": f"{name} us/frame, 1280x720", "batch": N, "launches": LAUNCHES, "us_per_frame": round(us / N, 3),
                "us_per_launch": round(us, 2), "bytes_per_pixel": {"algorithmic": algo_bpp, "fetched_and_written": fetch_bpp},
                "algorithmic_GBps": round(px * algo_bpp / us / 1e3, 1), "fetched_GBps": round(px * fetch_bpp / us / 1e3, 1), **more}

    us = timed(ingest)
    yard = line("rvdd_ingest_raw (u16 mosaic -> packed + gray)", us, 2 + 4 + 1, 2 + 4 + 1)
    lines = [yard]
    for lname, layout, shape in (("rgb_hwc", _lib.OUT_RGB_HWC, (N, H, W, 3)), ("mosaic", _lib.OUT_MOSAIC, (N, H, W)),
                                 ("packed_hwc", _lib.OUT_PACKED_HWC, (N, H // 2, W // 2, 4))):
        for dname, dtype, tdt, esz in (("u16", _lib.RAW_U16, torch.int16, 2), ("f32", _lib.RAW_F32, torch.float32, 4)):
            out = torch.empty(shape, dtype=tdt, device="cuda")

            def egress():
                rc = lib.rvdd_egress(h, rgb.data_ptr(), N, H, W, layout, dtype, BIT_DEPTH, 0, out.data_ptr(), stream)
                assert rc == 0, lib.rvdd_last_error(h)

            us = timed(egress)
            read, fetched, written = (12, 12, 3 * esz) if layout == _lib.OUT_RGB_HWC else (4, 8, esz)
            ln = line(f"rvdd_egress {lname} {dname}", us, read + written, fetched + written, layout=lname, dtype=dname, bit_depth=BIT_DEPTH)
            ln["algorithmic_rate_over_ingest_raw"] = round(ln["algorithmic_GBps"] / yard["algorithmic_GBps"], 3)
            ln["fetched_rate_over_ingest_raw"] = round(ln["fetched_GBps"] / yard["fetched_GBps"], 3)
            lines.append(ln)
    os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "egress_bench.jsonl"), "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
