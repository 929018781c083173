#!/usr/bin/env python3
"""The constants of rvdd_noise_fit: the lower quartile C_Q (and, for the tests' comparison, the median) of the block variance
estimate v of rvdd_noise_hist's rule on unit white Gaussian samples.  v = (1/72) * the sum over 8 rows of 6 squared second
differences d = x[c] - (x[c-1] + x[c+1]) / 2 has mean 1 for unit variance but is skewed, so its quantiles lie below 1.

Seeded: BLOCKS (default 4194304) blocks from numpy's default_rng(SEED), in chunks, through tests/noise_ref.block_stats -- the f32
arithmetic of the rule itself.  Prints the two constants to six places; the literals in csrc/ops.hip and tests/noise_ref.py are
this output rounded to four."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import noise_ref  # noqa: E402

SEED = 20261019
BLOCKS = int(os.environ.get("BLOCKS", str(1 << 22)))
CHUNK = 1 << 16


def main():
    rng = np.random.default_rng(SEED)
    v = np.empty(BLOCKS, np.float32)
    for at in range(0, BLOCKS, CHUNK):
        k = min(CHUNK, BLOCKS - at)
        v[at:at + k] = noise_ref.block_stats(rng.standard_normal((k, 8, 8)).astype(np.float32))[1]
    q25, q50 = np.quantile(v.astype(np.float64), [0.25, 0.5])
    # the standard error of a quantile: sqrt(p (1 - p) / n) / density; the density of v near both is about 1.7
    print("seed %d, %d blocks: mean %.6f  C_Q (lower quartile) %.6f  C_MED (median) %.6f  (standard error about %.1e)"
          % (SEED, BLOCKS, v.mean(dtype=np.float64), q25, q50, 0.5 / BLOCKS ** 0.5 / 1.7))


if __name__ == "__main__":
    main()
