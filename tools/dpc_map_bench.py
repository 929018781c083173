#!/usr/bin/env python3
"""Time of the static defect map's two kernels on 1280x720 frames (640 x 360 cells), n = 8, beside rvdd_dpc and rvdd_ingest_raw in the
same process: rvdd_dpc_detect (the wide form), and rvdd_dpc_map_apply with one defective sample in 10^4 and one in 10^3 (uniformly
scattered; the map's cells follow).  rvdd_timer_start / rvdd_timer_stop_ms over LAUNCHES launches after a warm-up.  The frames: a flat
12-bit scene with the noise of the ISO 3200 curve and the map's sites hot in every frame.
Prints one line per kernel and appends them to profiles/dpc_map_kernel.txt (or the file named by DPC_MAP_BENCH_OUT).
    python tools/dpc_map_bench.py --denoise     `denoise` end to end instead (see `denoise` below)"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import kernel_resources  # noqa: E402
from rvdd_release_amd import _lib  # noqa: E402
from rvdd_release_amd.runtime import dpc_cfg, dpc_detect_cfg, dpc_iso_curve, dpc_map_from_mosaic, dpc_map_stats  # noqa: E402
from rvdd_release_amd.util._ops import ops_runtime  # noqa: E402

N, H, W = int(os.environ.get("BATCH", "8")), 720, 1280
LAUNCHES, WARMUP = int(os.environ.get("LAUNCHES", "200")), 20


def main():
    assert torch.cuda.is_available(), "dpc_map_bench needs a GPU"
    rt = ops_runtime(0)
    hh, ww = H // 2, W // 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    a, b = dpc_iso_curve(3200, 12)
    m = 0.45 * 4095
    dn = (m + (a * m - b) ** 0.5 * torch.randn(N, H, W, device="cuda", generator=gen)).round().clamp(0, 4095)
    rng = np.random.default_rng(2)
    maps = {}
    for name, share in (("1 in 10^4", 1e-4), ("1 in 10^3", 1e-3)):
        maps[name] = rng.random((H, W)) < share
    dn[:, torch.from_numpy(maps["1 in 10^4"]).cuda()] = 4095
    mosaic = dn.to(torch.int16)
    packed, gray = rt.ingest_raw(mosaic, 12, "mosaic")
    out = torch.empty_like(packed)
    counts = torch.zeros(N, 2, dtype=torch.int32, device="cuda")
    hits = torch.zeros(4, hh, ww, dtype=torch.int32, device="cuda")
    cfg = dpc_cfg(4, 4, a, b)
    dcfg = dpc_detect_cfg(cfg, 0)
    vgpr = {r["name"]: r.get("vgpr_count", 0) for r in kernel_resources.kernel_table(_lib.LIB_PATH)}

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

    def detect():
        rc = rt.lib.rvdd_dpc_detect(rt.h, packed.data_ptr(), N, hh, ww, 12, dcfg, hits.data_ptr(), rt._stream())
        assert rc == 0, rt.lib.rvdd_last_error(rt.h)

    def apply():
        rc = rt.lib.rvdd_dpc_map_apply(rt.h, out.data_ptr(), gray.data_ptr(), N, hh, ww, 12, rt._stream())
        assert rc == 0, rt.lib.rvdd_last_error(rt.h)

    lines = []
    fmt = "%-58s %8.2f us/frame  %8.1f us/launch of %d frames  %s vgpr"
    for name, fn, kernel in (("rvdd_ingest_raw (u16 mosaic -> packed + gray)", ingest, "ingest_raw_kernel<unsigned short, 0, true>"),
                             ("rvdd_dpc (packed -> packed, gray patched, counts)", dpc, "dpc_kernel<4>"),
                             ("rvdd_dpc_detect (packed -> hits, tolerate 0)", detect, "dpc_detect_kernel<4>")):
        us = timed(fn)
        lines.append(fmt % (name, us / N, us, N, vgpr.get(kernel)))
    torch.cuda.synchronize()
    found = hits.cpu().numpy().view(np.uint32)
    lines.append("detect: %d sites hot in all %d frames of the last calls' total, %d injected"
                 % (int(((found & 0xffff) >= min(65535, N * (LAUNCHES + WARMUP))).sum()), N * (LAUNCHES + WARMUP), int(maps["1 in 10^4"].sum())))
    out.copy_(packed)
    for name, bad in maps.items():
        mask = dpc_map_from_mosaic(bad)
        st = dpc_map_stats(mask)
        rt.set_dpc_map(mask)
        us = timed(apply)
        lines.append(fmt % ("rvdd_dpc_map_apply (%s: %d samples, %d cells)" % (name, st["samples"], st["cells"]), us / N, us, N,
                            vgpr.get("dpc_map_apply_kernel")))
    rt.set_dpc_map(None)
    torch.cuda.synchronize()
    path = os.environ.get("DPC_MAP_BENCH_OUT", os.path.join(REPO, "profiles", "dpc_map_kernel.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


FLAGS = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(REPO, "weights", "recurrent-convunet+feat-iso3200"),
         "--feature_rec", "--bit_depth", "12", "--nFolder", "noisy"]


def _run(module, args, cwd=REPO):
    import subprocess
    p = subprocess.run([sys.executable, "-m", "rvdd_release_amd." + module] + args, cwd=cwd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    print("ran %s %s" % (module, " ".join(a for a in args if a.startswith("--dpc"))), flush=True)
    return p.stdout


def _write_tree(root, videos, bad):
    """<root>/noisy/<video>/<frame>.tif: uint16 mosaics [T,H,W] with the sites of `bad` (bool [H,W]) at 4095 in every frame"""
    from rvdd_release_amd import tiffio
    for v, frames in enumerate(videos):
        os.makedirs(os.path.join(root, "noisy", "%03d" % v))
        for t, m in enumerate(frames):
            m = m.copy()
            m[bad] = 4095
            tiffio.write(os.path.join(root, "noisy", "%03d" % v, "%08d.tif" % t), m.astype(np.uint16))


def denoise():
    """`denoise` end to end: (1) a small tree of synth's moving texture with injected static hot samples -- the samples --dpc 4 replaces
    per frame, the samples --dpc_map auto --dpc_static_only replaces, and whether every injected site is among the latter; (2) 720p,
    --dpc_map FILE off and on, alternating, three rounds.  Appends to profiles/dpc_map_denoise.txt (or the file named by
    DPC_MAP_BENCH_OUT)."""
    import re
    import tempfile
    from rvdd_release_amd import synth
    from rvdd_release_amd.dpc_map import read_map, write_map
    from rvdd_release_amd.runtime import dpc_iso_curve, dpc_map_to_mosaic
    lines = []
    rng = np.random.default_rng(5)
    # (1) the small tree
    T, H, W = 16, 128, 192
    with tempfile.TemporaryDirectory() as tmp:
        vids = []
        for v in range(2):
            raw = synth.make_sequence(T, H, W, iso=3200, seed=40 + v).raw.numpy()            # [T,4,h,w] in [-1,1]
            dn = np.clip(np.rint((raw + 1) * 0.5 * 4095), 0, 4095)
            m = np.zeros((T, H, W), np.float32)
            for k in range(4):
                m[:, k >> 1::2, k & 1::2] = dn[:, k]
            vids.append(m)
        bad = rng.random((H, W)) < 1e-3
        bad[10, 10] = bad[10, 12] = True                      # an equal pair of one colour: out of the dynamic rule's reach, and of tolerate 0
        _write_tree(tmp, vids, bad)
        rule = ["--dpc", "4", "--dpc_iso", "3200"]
        dyn = _run("denoise", ["--dataroot", tmp, "--results_dir", os.path.join(tmp, "r0")] + FLAGS + rule)
        per = [(int(h) + int(d)) / int(f) for h, d, f in re.findall(r"dpc: (\d+) hot, (\d+) dead samples corrected in (\d+) frames", dyn)]
        stat = _run("denoise", ["--dataroot", tmp, "--results_dir", os.path.join(tmp, "r1")] + FLAGS + rule + ["--dpc_map", "auto", "--dpc_static_only"])
        told = re.search(r"dpc_map: (\d+) samples in (\d+) cells, (\d+) unfixable, from (\d+) frames", stat)
        _run("dpc_map", ["--dataroot", tmp, "--nFolder", "noisy", "--bit_depth", "12", "--out", os.path.join(tmp, "map.tif")] + rule)
        found = dpc_map_to_mosaic(read_map(os.path.join(tmp, "map.tif"))) != 0
        lines += ["small tree: 2 videos of %d frames of %dx%d, synth's moving texture, noise of ISO 3200, %d static hot samples injected (one equal pair of one colour among them)"
                  % (T, W, H, int(bad.sum())),
                  "  --dpc 4 --dpc_iso 3200 replaces %s samples per frame (per video)" % ", ".join("%.1f" % p for p in per),
                  "  --dpc_map auto --dpc_static_only replaces %s samples per frame (%s cells, %s unfixable, found in %s frames)" % told.groups(),
                  "  injected sites in the map: %d of %d; map entries that were not injected: %d"
                  % (int((found & bad).sum()), int(bad.sum()), int((found & ~bad).sum()))]
    # (2) 720p, the map from a file
    T, H, W = 12, 720, 1280
    a, b = dpc_iso_curve(3200, 12)
    with tempfile.TemporaryDirectory() as tmp:
        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
        vids = []
        for v in range(2):
            fr = []
            for t in range(T):
                m = (0.3 + 0.1 * v + 0.05 * x / W + 0.04 * np.sin((x + 3 * t) * (2 * np.pi / 400))) * 4095
                fr.append(np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0)) * rng.standard_normal(m.shape, dtype=np.float32)), 0, 4095))
            vids.append(np.stack(fr))
        bad = rng.random((H, W)) < 1e-4
        _write_tree(tmp, vids, bad)
        from rvdd_release_amd.runtime import dpc_map_from_mosaic
        write_map(os.path.join(tmp, "map.tif"), dpc_map_from_mosaic(bad))
        lines.append("denoise 1280x720, 2 videos of %d frames, batch 2, recurrent-convunet+feat-iso3200, f32 files, one hot sample in 10^4 (%d); a fresh "
                     "process per run; --dpc_map FILE off and on alternating" % (T, int(bad.sum())))
        for r in range(3):
            for name, more in (("off", []), ("on ", ["--dpc_map", os.path.join(tmp, "map.tif")])):
                out = _run("denoise", ["--dataroot", tmp, "--results_dir", os.path.join(tmp, "res_%d_%s" % (r, name.strip())), "--batch_size", "2"] + FLAGS + more)
                told = re.search(r"\(denoise, (\d+) frames, ([0-9.]+) s, ([0-9.]+) frames/s\)", out)
                extra = "  ".join(ln for ln in out.splitlines() if ln.startswith("dpc_map:"))
                lines.append("  --dpc_map %s: %s frames, %s s, %s frames/s  %s" % (name, told.group(1), told.group(2), told.group(3), extra.replace(tmp, "<tmp>")))
    path = os.environ.get("DPC_MAP_BENCH_OUT", os.path.join(REPO, "profiles", "dpc_map_denoise.txt"))
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


if __name__ == "__main__":
    denoise() if "--denoise" in sys.argv else main()
