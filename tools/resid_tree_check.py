#!/usr/bin/env python3
"""Is a wild residual report the network's doing, or the measurement's?

    python tools/resid_tree_check.py      six frames of 384 x 256 of `synth` and of each of the two shots of `cuts_bench.py`'s throughput
                                          tree (a gray scene at 13 .. 32 % and at 45 .. 77 % of the range, the noise of the ISO 3200 curve)
                                          through `video_push` with the stage on (recurrent-convunet+feat-iso3200, --all_frames): per frame
                                          the mean of the noisy frame and of the re-mosaicked output taken with torch, and the report of
                                          the shot beside them -- the stage's bias is the mean of the per-frame differences.

Prints its lines and appends them to profiles/resid_tree_check.txt (or the file named by RESID_TREE_OUT)."""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from safetensors.torch import load_file
from rvdd_release_amd.runtime import RvddRuntime, dpc_iso_curve, resid_fit
from rvdd_release_amd import synth, _lib


def emit(line):
    path = os.environ.get("RESID_TREE_OUT", os.path.join(REPO, "profiles", "resid_tree_check.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    print(line)
    with open(path, "a") as f:
        f.write(line + "\n")


H, W, T = 256, 384, 6
a, b = dpc_iso_curve(3200, 12)
rng = np.random.default_rng(7)
y, x = np.mgrid[0:H, 0:W].astype(np.float32)
def tree(level, tilt):
    out = []
    for t in range(T):
        m = (level + tilt * (y / H - 0.5) * 0.4 + 0.05 * x / W + 0.04 * np.sin((x + 3 * t) * (2 * np.pi / 400))) * 4095
        out.append(np.clip(np.rint(m + np.sqrt(np.maximum(a * m - b, 0)) * rng.standard_normal(m.shape, dtype=np.float32)), 0, 4095).astype(np.uint16))
    return np.stack(out)
s = synth.make_sequence(T, H, W, iso=3200, seed=1)
dn = np.clip(np.rint((s.raw.numpy() + 1) * 0.5 * 4095), 0, 4095)
mos = np.zeros((T, H, W), np.uint16)
for k in range(4):
    mos[:, k >> 1::2, k & 1::2] = dn[:, k]
rt = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
rt.load_state_dict(load_file(os.path.join(REPO, "weights", "recurrent-convunet+feat-iso3200.safetensors")))
rt.set_option("stream_all_frames", 1)
rt.set_resid(True)
for name, video in (("synth", mos), ("tree dark", tree(0.18, 0.25)), ("tree bright", tree(0.55, -0.2))):
    for t in range(T):
        fr = torch.from_numpy(video[t:t + 1].view(np.int16)).cuda()
        out, valid = rt.video_push(fr, [_lib.PUSH_FIRST if t == 0 else _lib.PUSH_NEXT], 12, "mosaic")
        o = (out[0] + 1) * 0.5 * 4095
        re = torch.stack([o[(1, 2, 0, 1)[k], k >> 1::2, k & 1::2] for k in range(4)])
        pk = torch.stack([fr[0].view(torch.int16).to(torch.int32).bitwise_and(0xffff).float()[k >> 1::2, k & 1::2] for k in range(4)])
        emit("%-11s t=%d valid=%s noisy mean %.1f  remosaic(out) mean %.1f  min %.1f max %.1f  diff mean %+.2f std %.1f" % (
            name, t, valid[0], float(pk.mean()), float(re.mean()), float(re.min()), float(re.max()), float((pk - re).mean()), float((pk - re).std())))
    acc = rt.resid_read(0)
    try:
        emit("%-11s %s" % (name, resid_fit(acc, 12, a, b)))
    except RuntimeError as e:
        emit("%-11s fit: %s" % (name, e))
