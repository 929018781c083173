#!/usr/bin/env python3
"""Golden vectors for the raw-dataset synthesis from the REFERENCE's own program (dataset/generate_raw_from_RGB.py), build
container only:

    python3 tools/make_golden_unprocess.py [--out DIR]

The reference is a script, not a module: it is run by path with runpy, as __main__, once per ISO and frame size, with
stand-ins for iio and skimage that hand it the input frames and capture every array it writes, and with `torch.Tensor.cuda`
patched to the identity (there is no GPU here) -- the treatment tools/make_golden_ppipe.py gives fwd_ppipe.py.  The linear
image it hands fwd_ppipe.ppipe is captured at that call (the script writes it only rounded to uint16).

The script draws its dither and its noise from numpy's global generator: `np.random.seed(k)` before the run, then replaying
`np.random.rand(H, W, 3) - 0.5` (cast to float32) and `np.random.randn(h, w, 4)` in loop order after the same seed, recovers
both planes of every frame.

Writes tests/golden/unprocess_iso3200.npz and unprocess_iso12800.npz: per size tag ("odd": 35 x 47 frames, cropped by the
script to 34 x 46 = 17 x 23 cells; "wide": 32 x 64), two sequences x two frames of input uint8, dither, normal, the gains of
each sequence, and the reference's lin_f32, lin_u16, gt_raw, noisy and gt_rgb."""
import argparse
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
SCRIPT = os.path.join(REF, "dataset", "generate_raw_from_RGB.py")
SIZES = {"odd": (35, 47), "wide": (32, 64)}
NSEQ, NFRAMES = 2, 2


def _standins(inputs, store):
    iio = types.ModuleType("iio")
    iio.read = lambda p: inputs[p].copy()
    iio.write = lambda p, a: store.__setitem__(p, np.array(a))
    sk = types.ModuleType("skimage")
    skio = types.ModuleType("skimage.io")
    skm = types.ModuleType("skimage.metrics")
    skio.imsave = lambda p, a, **k: store.__setitem__(p, np.array(a))
    skio.imread = None
    skm.structural_similarity = None
    sk.io, sk.metrics = skio, skm
    sys.modules.update({"iio": iio, "skimage": sk, "skimage.io": skio, "skimage.metrics": skm})


def frames_of(tag, iso):
    """Input frames: uniform noise over the 8-bit range, rows of 0 and of 255 (both clamps), a dark and a bright band."""
    H, W = SIZES[tag]
    rng = np.random.default_rng([iso, H, W])
    x = rng.integers(0, 256, (NSEQ, NFRAMES, H, W, 3)).astype(np.uint8)
    x[:, :, :3] = 0
    x[:, :, 3:6] = 255
    x[:, :, 6:9] = rng.integers(0, 6, (NSEQ, NFRAMES, 3, W, 3))
    x[:, :, 9:12] = rng.integers(250, 256, (NSEQ, NFRAMES, 3, W, 3))
    return x


def run_reference(tag, iso, seed):
    x = frames_of(tag, iso)
    inputs = {"/in/%03d/%08d.png" % (s, i): x[s, i].astype(np.float32) for s in range(NSEQ) for i in range(NFRAMES)}
    store, lin = {}, []
    _standins(inputs, store)
    import fwd_ppipe
    if not os.path.realpath(fwd_ppipe.__file__).startswith(os.path.realpath(REF) + os.sep):
        raise RuntimeError(f"fwd_ppipe was imported from {fwd_ppipe.__file__!r}, not from {REF}: refusing to write fixtures")
    real = fwd_ppipe.ppipe

    def capture(im, *a, **k):
        lin.append(np.array(im))
        return real(im, *a, **k)

    fwd_ppipe.ppipe = capture
    argv = sys.argv
    try:
        with tempfile.TemporaryDirectory() as tmp:             # the script creates its (empty) output folders
            sys.argv = ["generate_raw_from_RGB.py", "--input_val_dataset", "/in/%03d/%08d.png", "--output_val_dataset", tmp + "/val/",
                        "--output_train_dataset", tmp + "/train/", "--nb_seq_val", str(NSEQ), "--nb_seq_train", "0", "--ISO", str(iso),
                        "--first", "0", "--last", str(NFRAMES - 1)]
            np.random.seed(seed)
            g = runpy.run_path(SCRIPT, run_name="__main__")
            store = {os.path.relpath(k, tmp): v for k, v in store.items()}
    finally:
        sys.argv = argv
        fwd_ppipe.ppipe = real
    H, W = 2 * (SIZES[tag][0] // 2), 2 * (SIZES[tag][1] // 2)
    np.random.seed(seed)
    dither, normal = [], []
    for _ in range(NSEQ * NFRAMES):
        dither.append((np.random.rand(H, W, 3) - 0.5).astype(np.float32))
        normal.append(np.random.randn(H // 2, W // 2, 4).astype(np.float32))

    def tree(folder, ext):
        return np.stack([np.stack([store["val/%s_iso%4d/%03d/%08d.%s" % (folder, iso, s, i, ext)] for i in range(NFRAMES)])
                         for s in range(NSEQ)])

    out = {"in": x, "dither": np.stack(dither).reshape(NSEQ, NFRAMES, H, W, 3),
           "normal": np.stack(normal).reshape(NSEQ, NFRAMES, H // 2, W // 2, 4),
           "gains": np.array([g["find_gains"](s, iso) for s in range(NSEQ)], np.float64),
           "lin_f32": np.stack(lin).reshape(NSEQ, NFRAMES, H, W, 3), "lin_u16": tree("gt_raw_linear_RGB", "tiff"),
           "gt_raw": tree("gt", "tiff"), "noisy": tree("noisy", "tiff"), "gt_rgb": tree("gt_RGB", "png")}
    assert out["lin_f32"].dtype == np.float32 and out["gt_raw"].dtype == np.float32 and out["noisy"].dtype == np.float32
    assert out["lin_u16"].dtype == np.uint16 and out["gt_rgb"].dtype == np.uint8
    return {f"{k}_{tag}": v for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"), help="write the fixtures here instead of tests/golden")
    args = ap.parse_args(argv)
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    if not os.path.isfile(SCRIPT):
        raise SystemExit(f"{SCRIPT} is missing: the fixtures are made from the reference itself")
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, os.path.join(REF, "dataset"))
    os.makedirs(args.out, exist_ok=True)
    for iso in (3200, 12800):
        data = {}
        for k, tag in enumerate(SIZES):
            data.update(run_reference(tag, iso, seed=11 + k))
        np.savez_compressed(os.path.join(args.out, f"unprocess_iso{iso}.npz"), **data)
        print(f"unprocess_iso{iso}.npz:", ", ".join(f"{k}{tuple(v.shape)}" for k, v in sorted(data.items())))


if __name__ == "__main__":
    main()
