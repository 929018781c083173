#!/usr/bin/env python3
"""Fixtures of tests/test_gpu_prologue.py: what the library of ONE commit computes for small convunet+feat frame-steps whose
border ring is not a whole number of 16-pixel runs.  Run it on the GPU box with the library of the commit the later ones are
to be held to (the fixtures in the tree: the parent of the commit that rewrote pre_border_fix_kernel by runs):

    python3 tools/make_golden_prologue.py [--out DIR]

Writes tests/golden/prologue_parent_<H>x<W>.npz (or DIR/...): the inputs (synth.make_sequence, fixed seeds, made on the CPU
and stored, so that the test feeds the very same bits whatever libm regenerates them), the output frames of the first two steps of a
video and the recurrent state after them.  The features are stored as their four byte planes (`feat_planes` [4][n] uint8, little endian:
plane k = byte k of every float), which deflate far better than the floats; the test puts the floats together again."""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ARCH, STEM = "convunet+feat", "recurrent-convunet+feat-iso3200"
CASES = [(34, 50, 3, 3), (18, 16, 1, 3), (48, 64, 2, 5)]      # H, W, B, input frames stored (the first STEPS + 1 are stepped)
STEPS = 2
SEED0 = 4100


def inputs(H, W, B, T):
    from rvdd_release_amd import synth
    seqs = [synth.make_sequence(T, H, W, iso=3200, seed=SEED0 + 10 * H + b) for b in range(B)]
    raw = torch.stack([s.raw for s in seqs], 1).contiguous()              # [T,B,4,h,w]
    flow = torch.stack([s.flow_prev for s in seqs], 1).contiguous()       # [T,B,2,h,w]
    return raw, flow


def run(raw, flow, H, W, B, options=()):
    """-> (frames [STEPS,B,3,H,W], den [B,3,H,W], feat [B,48,H,W]) on the CPU"""
    from safetensors.torch import load_file
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime(ARCH, 0, B, H, W, 0)
    for k, v in options:
        rt.set_option(k, v)
    rt.load_state_dict(load_file(os.path.join(REPO, "weights", STEM + ".safetensors")))
    raw, flow = raw.cuda(), flow.cuda()
    frames = [rt.step(raw[t - 1] if t == 1 else None, raw[t], None, flow[t], None).clone() for t in range(1, STEPS + 1)]
    den, feat = rt.get_state()
    torch.cuda.synchronize()
    rt.close()
    return torch.stack(frames, 0).cpu(), den.cpu(), feat.cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    for H, W, B, T in CASES:
        raw, flow = inputs(H, W, B, T)
        frames, den, feat = run(raw, flow, H, W, B)
        planes = np.ascontiguousarray(feat.numpy().reshape(-1).view(np.uint8).reshape(-1, 4).T)
        dst = os.path.join(args.out, f"prologue_parent_{H}x{W}.npz")
        np.savez_compressed(dst, raw=raw.numpy(), flow_prev=flow.numpy(), frames=frames.numpy(), den=den.numpy(), feat_planes=planes)
        print(f"[golden] {dst}: {os.path.getsize(dst)} bytes, frames {tuple(frames.shape)}, |frames| max {float(frames.abs().max()):.4f}, "
              f"features non-zero {float((feat != 0).float().mean()):.3f}")


if __name__ == "__main__":
    main()
