"""The validation dataset on disk, for the tests that run validate.py or the dataset classes on a tree of their own."""
import os

import numpy as np


def write_dataset(root, seqs, iso=3200, with_flows=True, future=0):
    """The reference's validation layout (scripts/test-recurrent-feat-convunet.sh, data/infer4rec_dataset.py:64-80)."""
    from rvdd_release_amd import tiffio
    for v, s in enumerate(seqs):
        nd = os.path.join(root, f"noisy_iso{iso}", "%03d" % v)
        gd = os.path.join(root, f"gt_raw_linear_RGB_iso{iso}", "%03d" % v)
        fd = os.path.join(root, "flow", f"noisy_iso{iso}", "tvl1", "noisyinputs", "%03d" % v)
        for d in (nd, gd, fd):
            os.makedirs(d, exist_ok=True)
        Tn = s.raw.shape[0]
        for t in range(Tn):
            code = "%08d" % (3 * t)
            tiffio.write(os.path.join(nd, code + ".tiff"), ((s.raw[t].permute(1, 2, 0).numpy() + 1) / 2 * 4095).astype(np.float32))
            tiffio.write(os.path.join(gd, code + ".tiff"),
                         np.round((s.gt[t].permute(1, 2, 0).numpy() + 1) / 2 * 4095).clip(0, 4095).astype(np.uint16))
            if with_flows and t > 0:
                tiffio.write(os.path.join(fd, "%08d_%s.tif" % (3 * (t - 1), code)), s.flow_prev[t].permute(1, 2, 0).numpy())
            if with_flows and future and t < Tn - 1:
                tiffio.write(os.path.join(fd, "%08d_%s.tif" % (3 * (t + 1), code)), s.flow_next[t].permute(1, 2, 0).numpy())
