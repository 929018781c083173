#!/usr/bin/env python3
"""The quality table of DESIGN.md 4.16: what mapping footage onto the checkpoint's noise curve (rvdd_match_raw -> step ->
rvdd_unmatch_rgb) buys or costs, from weights/ and rvdd_release_amd.synth alone.

Per camera (bit depth, a, black level; var(m) = a (m - black) + 100 in DN of that depth) and checkpoint family (ISO 3200, ISO 12800):
the scene is synth.make_sequence(6, 96, 128, iso=3200, seed)'s `gt`, taken as the scene in the camera's own range; its GBRG mosaic
gets the camera's noise sqrt(max(a dn - b, 0)) z, z from torch.Generator().manual_seed(5).randn, is rounded and clipped; the frames
go through rt.step with the sequence's analytic flows and weights/recurrent-convunet+feat-iso<ISO>, once as they are and once
mapped (the output mapped back).  Mean PSNR, 10 log10(4 / mse), of outputs 2..5 against the scene, both in the camera's domain.

    python tools/match_study.py [--seeds 0,1,2,3,4] [--backend hip|oracle] [--out FILE]

--backend oracle runs the f32 CPU oracle (oracle/rvdd_oracle.py) with the NumPy restatement of the two maps instead of the device.
One line per row; the a = 60 camera is run for every seed, the others for the first."""
import argparse
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rvdd_release_amd import synth  # noqa: E402
from rvdd_release_amd.runtime import match_coeffs  # noqa: E402

CAMERAS = [(12, 3.0, 256), (12, 15.0, 256), (12, 60.0, 256), (12, 120.0, 256), (10, 4.0, 64), (14, 60.0, 1024)]
H, W, T = 96, 128, 6


def camera_frames(gt, bits, a, b):
    top = float(2 ** bits - 1)
    dn = (gt.double() + 1.0) * 0.5 * top
    u = torch.stack([dn[:, (1, 2, 0, 1)[k], (k >> 1)::2, (k & 1)::2] for k in range(4)], 1)      # G B / R G
    z = torch.randn(u.shape, generator=torch.Generator().manual_seed(5)).double()
    noisy = torch.round(u + torch.sqrt(torch.clamp(a * u - b, min=0.0)) * z).clamp(0, top)
    return (2.0 * (noisy / top) - 1.0).float().contiguous()


def psnr(x, y):
    return 10.0 * math.log10(4.0 / float(((x.double() - y.double()) ** 2).mean()))


class Hip:
    def __init__(self, iso):
        from safetensors.torch import load_file
        from rvdd_release_amd.runtime import RvddRuntime
        self.rt = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
        self.rt.load_state_dict(load_file(os.path.join(REPO, "weights", "recurrent-convunet+feat-iso%d.safetensors" % iso)))

    def run(self, seq, frames, cfg):
        rt = self.rt
        frames, fl, gt = frames.cuda(), seq.flow_prev.cuda(), seq.gt.cuda()
        if cfg is not None:
            frames = rt.match_raw(frames, cfg)
        rt.reset()
        ps = []
        for t in range(1, T):
            out = rt.step(frames[t - 1][None], frames[t][None], None, fl[t][None], None)
            if cfg is not None:
                out = rt.unmatch_rgb(out, cfg)
            if t >= 2:
                ps.append(psnr(out, gt[t][None]))
        return sum(ps) / len(ps)


class Oracle:
    def __init__(self, iso):
        from safetensors.torch import load_file
        sys.path.insert(0, os.path.join(REPO, "oracle"))
        import rvdd_oracle
        self.make = lambda: rvdd_oracle.RecurrentOracle(
            load_file(os.path.join(REPO, "weights", "recurrent-convunet+feat-iso%d.safetensors" % iso)), future=0)

    def run(self, seq, frames, cfg):
        F = np.float32
        if cfg is not None:
            frames = torch.from_numpy((F(cfg.scale) * frames.numpy()) + F(cfg.offset))
        orc, ps = self.make(), []
        with torch.no_grad():
            for t in range(1, T):
                out = orc.step(frames[t - 1][None], frames[t][None], None, seq.flow_prev[t][None], None, first=(t == 1))[0].float()
                if cfg is not None:
                    out = torch.from_numpy((out.numpy() - F(cfg.offset)) * F(1.0 / float(F(cfg.scale))))
                if t >= 2:
                    ps.append(psnr(out, seq.gt[t][None]))
        return sum(ps) / len(ps)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", default="0,1,2,3,4")
    p.add_argument("--backend", default="hip", choices=("hip", "oracle"))
    p.add_argument("--out", default=None, help="also append the lines to this file")
    args = p.parse_args()
    seeds = [int(v) for v in args.seeds.split(",")]
    lines = ["match_study: backend %s, %d frames of %d x %d, outputs 2..%d" % (args.backend, T, W, H, T - 1)]
    print(lines[0], flush=True)
    nets = {iso: (Hip if args.backend == "hip" else Oracle)(iso) for iso in (3200, 12800)}
    for bits, a, black in CAMERAS:
        b = a * black - 100.0
        for seed in (seeds if (bits, a) == (12, 60.0) else seeds[:1]):
            seq = synth.make_sequence(T, H, W, iso=3200, seed=seed)
            frames = camera_frames(seq.gt, bits, a, b)
            row = "%2d-bit a = %-5g black %-4d seed %d" % (bits, a, black, seed)
            for iso, net in nets.items():
                cfg, s, _ = match_coeffs(a, b, bits, iso)
                un, ma = net.run(seq, frames, None), net.run(seq, frames, cfg)
                row += " | ISO %-5d s = %-6.3g unmatched %6.2f matched %6.2f gain %+5.2f dB" % (iso, s, un, ma, ma - un)
            lines.append(row)
            print(row, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
