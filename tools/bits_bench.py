#!/usr/bin/env python3
"""Throughput of rvdd_ingest_bits and rvdd_egress_bits on 1280x720 frames, n = 8, for the six (order, bit depth) pairs of each,
and of rvdd_ingest_raw (a u16 mosaic in, both outputs) in the same process as the yardstick -- the form of tools/egress_bench.py.
HIP events over LAUNCHES launches after a warm-up.  Thirteen JSON lines, appended to profiles/bits_bench.jsonl (or the file
named by BITS_BENCH_OUT).

Per line: microseconds per frame, the algorithmic bytes per pixel -- ingest reads b / 8 and writes 4 + 1; egress uses 4 of its
input (and fetches 8: the other half of every 16-byte vector is another colour's site) and writes b / 8 -- the byte rate over
that time as a fraction of the yardstick's, and the kernel's vector registers.  The project's criterion: at least
half the yardstick's algorithmic rate."""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_resources  # noqa: E402
from rvdd_release_amd import _lib  # noqa: E402
from rvdd_release_amd.runtime import bits_row_bytes  # noqa: E402
from rvdd_release_amd.util._ops import ops_runtime  # noqa: E402

N, H, W = int(os.environ.get("BATCH", "8")), 720, 1280
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20
ORDERS = (("mipi", _lib.BITS_MIPI), ("msb", _lib.BITS_MSB))


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
    assert torch.cuda.is_available(), "bits_bench needs a GPU"
    rt = ops_runtime(0)
    lib, h, stream = rt.lib, rt.h, rt._stream()
    px = N * H * W
    rng = np.random.default_rng(1)
    rgb = torch.from_numpy(rng.uniform(-1, 1, (N, 3, H, W)).astype(np.float32)).cuda()
    mosaic = torch.from_numpy(rng.integers(0, 4096, (N, H, W), dtype=np.uint16).view(np.int16)).cuda()
    packed = torch.empty(N, 4, H // 2, W // 2, device="cuda")
    gray = torch.empty(N, H // 2, W // 2, device="cuda")
    vgpr = {r["name"]: r.get("vgpr_count", 0) for r in kernel_resources.kernel_table(_lib.LIB_PATH)}

    def ingest_raw():
        rc = lib.rvdd_ingest_raw(h, mosaic.data_ptr(), _lib.RAW_U16, _lib.RAW_MOSAIC, N, H // 2, W // 2, 12, packed.data_ptr(), gray.data_ptr(), stream)
        assert rc == 0, lib.rvdd_last_error(h)

    def line(name, us, algo_bpp, fetch_bpp, **more):
        return {"metric": f"{name} us/frame, 1280x720", "batch": N, "launches": LAUNCHES, "us_per_frame": round(us / N, 3),
                "us_per_launch": round(us, 2), "bytes_per_pixel": {"algorithmic": algo_bpp, "fetched_and_written": fetch_bpp},
                "algorithmic_GBps": round(px * algo_bpp / us / 1e3, 1), "fetched_GBps": round(px * fetch_bpp / us / 1e3, 1), **more}

    yard = line("rvdd_ingest_raw (u16 mosaic -> packed + gray)", timed(ingest_raw), 2 + 4 + 1, 2 + 4 + 1,
                vgpr=vgpr.get("ingest_raw_kernel<unsigned short, 0, true>"))
    lines = [yard]
    for direction in ("ingest", "egress"):
        for oname, order in ORDERS:
            for bits in (10, 12, 14):
                data = torch.randint(0, 256, (N, H, bits_row_bytes(W, bits, oname)), dtype=torch.uint8, device="cuda")

                def ingest():
                    rc = lib.rvdd_ingest_bits(h, data.data_ptr(), order, N, H // 2, W // 2, bits, packed.data_ptr(), gray.data_ptr(), stream)
                    assert rc == 0, lib.rvdd_last_error(h)

                def egress():
                    rc = lib.rvdd_egress_bits(h, rgb.data_ptr(), N, H, W, order, bits, 0, data.data_ptr(), stream)
                    assert rc == 0, lib.rvdd_last_error(h)

                us = timed(ingest if direction == "ingest" else egress)
                algo, fetched = (bits / 8 + 5, bits / 8 + 5) if direction == "ingest" else (4 + bits / 8, 8 + bits / 8)
                ln = line(f"rvdd_{direction}_bits {oname} {bits}", us, algo, fetched, order=oname, bit_depth=bits,
                          vgpr=vgpr.get(f"{direction}_bits_kernel<{bits}, {order}, true>"))
                ln["algorithmic_rate_over_ingest_raw"] = round(ln["algorithmic_GBps"] / yard["algorithmic_GBps"], 3)
                ln["fetched_rate_over_ingest_raw"] = round(ln["fetched_GBps"] / yard["fetched_GBps"], 3)
                lines.append(ln)
    path = os.environ.get("BITS_BENCH_OUT", os.path.join(REPO, "profiles", "bits_bench.jsonl"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
