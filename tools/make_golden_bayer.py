#!/usr/bin/env python3
"""Golden Hamilton-Adams demosaics in all four Bayer patterns, captured from the reference's HamiltonAdam(pattern)
(util/Hamilton_Adam_demo.py:175-289) like tools/make_golden.py does for GBRG (build container only):

    PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_bayer.py

Writes tests/golden/op_hamilton_adams_bayer.npz: `raw` [2,8,18,26] (two packed frames per item, with plateaus so that
the sign() selections also see exact ties) and `rgb_<pattern>` = HamiltonAdam(pattern)(raw) for gbrg, grbg, rggb, bggr."""
import os
import sys
import tempfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import make_golden as MG  # noqa: E402

PATTERNS = ("gbrg", "grbg", "rggb", "bggr")
NAME = "op_hamilton_adams_bayer.npz"


def main(argv=None):
    args = MG.parse_args(argv)
    gold = os.path.abspath(args.out) if args.out else MG.GOLD
    os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
    sys.dont_write_bytecode = True
    MG._install_standins()
    sys.path.insert(0, MG.REF)
    os.makedirs(gold, exist_ok=True)
    os.chdir(tempfile.mkdtemp(prefix="rvdd_golden_"))
    gen = torch.Generator().manual_seed(2718)
    torch.set_num_threads(8)
    import util.Hamilton_Adam_demo
    MG.assert_reference_modules(util.Hamilton_Adam_demo)
    from util.Hamilton_Adam_demo import HamiltonAdam

    raw = torch.rand(2, 8, 18, 26, generator=gen) * 2 - 1
    # plateaus: the sign() selections of algo1 / algo2 tie exactly there, in every plane
    raw[0, :4, 4:9, 5:12] = 0.25
    raw[1, 4:, :, :6] = -0.5
    raw[0, 4:, 10:, 14:] = 0.125
    raw[1, :2, 3:7, 9:20] = -0.75          # two of the four planes only: ties in one colour, not in the other
    out = {"raw": raw.numpy()}
    for p in PATTERNS:
        out[f"rgb_{p}"] = HamiltonAdam(p)(raw).numpy()
    np.savez(os.path.join(gold, NAME), **out)
    print(f"wrote {os.path.join(gold, NAME)}")


if __name__ == "__main__":
    main()
