#!/usr/bin/env python3
"""What the green equilibration gains and costs on footage whose truth is known.

    python tools/green_study.py [SEEDS]      synth sequences of 13 frames of 384 x 256 (12 outputs each), SEEDS (default 3) seeds, both
                                             checkpoint families (recurrent-convunet+feat-iso3200 / -iso12800 on footage of their own
                                             curve, analytic flows).  The clean GBRG mosaic is taken from the sequence's ground truth; an
                                             imbalance of 0, 1, 3 and 5 % -- flat, and ramped from half to one and a half of it from
                                             the left to the right edge -- is put on the CLEAN signal above black (plane 0 up, plane 3
                                             down by half of it each), then the family's noise, then the rounding to uint16, and the
                                             frames come back through rvdd_ingest_raw.  Per case, without the stage, with the map
                                             (rvdd_green_estimate on the sequence's 13 frames, rvdd_green_fit with min_frames 7, k_sig 3,
                                             max_gain 0.10 and min_signal top / 64, the family's curve and a gate of 3, then
                                             rvdd_green_apply on every frame) and with the flat estimate: the PSNR of outputs 2..12
                                             against the scene, and the map's counts, rms gain, floor and flat estimate.
    There is no bar on the gain: whether an imbalance below the noise hurts this network at all is what the table shows.  The one
    hard condition is checked: where the map is zero the outputs are bit for bit those without the stage.

Prints its lines and appends them to profiles/green_study.txt (or the file named by GREEN_STUDY_OUT)."""
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T, H, W = 13, 256, 384


def emit(lines):
    path = os.environ.get("GREEN_STUDY_OUT", os.path.join(REPO, "profiles", "green_study.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


def main(seeds):
    import numpy as np
    import torch
    from safetensors.torch import load_file
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import DPC_ISO_CURVES, RvddRuntime, green_cfg, green_fit
    assert torch.cuda.is_available(), "green_study needs a GPU"
    lines = ["green_study: %d seeds, %d frames of %d x %d, recurrent-convunet+feat, 12 outputs per case, PSNR of outputs 2..12; the map from the "
             "sequence's own %d frames: gate 3, min_frames %d, k_sig 3, max_gain 0.10, min_signal %.1f DN" % (seeds, T, W, H, T, (T + 1) // 2, 4095.0 / 64.0)]
    colour = (1, 2, 0, 1)                                       # GBRG: the RGB plane of CFA position k
    ramp = np.linspace(0.5, 1.5, W // 2)[None, None, :]
    for iso in DPC_ISO_CURVES:
        a, b = DPC_ISO_CURVES[iso]
        black = b / a
        rule = green_cfg(3.0, a, b, 1.0)
        rt = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
        rt.load_state_dict(load_file(os.path.join(REPO, "weights", "recurrent-convunet+feat-iso%d.safetensors" % iso)))
        lines.append("ISO %d: black %.1f DN, pixel sigma at the mid level %.1f DN" % (iso, black, math.sqrt(a * 2047.5 - b)))
        for gain, ramped in ((0.0, False), (0.01, False), (0.01, True), (0.03, False), (0.03, True), (0.05, False), (0.05, True)):
            plain_out = None
            for mode in ("off", "map", "flat"):
                ps, tot, outs, zero = [], None, [], True
                for seed in range(seeds):
                    seq = synth.make_sequence(T, H, W, iso=iso, seed=seed, device="cuda")
                    gt, fl = seq.gt.cuda(), seq.flow_prev.cuda()
                    dn = ((gt.double() + 1.0) / 2.0 * 4095.0).cpu().numpy()                                        # [T,3,H,W], clean
                    u = np.stack([dn[:, colour[k], (k >> 1)::2, (k & 1)::2] for k in range(4)], 1)                  # [T,4,hh,ww]
                    g = gain * (ramp if ramped else 1.0)
                    u[:, 0], u[:, 3] = u[:, 0] + 0.5 * g * (u[:, 0] - black), u[:, 3] - 0.5 * g * (u[:, 3] - black)
                    rng = np.random.default_rng(1000 * iso + seed)
                    noisy = u + np.sqrt(np.maximum(a * u - b, 0.0)) * rng.standard_normal(u.shape)
                    mosaic = np.zeros((T, H, W), np.uint16)
                    for k in range(4):
                        mosaic[:, (k >> 1)::2, (k & 1)::2] = np.clip(np.rint(noisy[:, k]), 0, 4095)
                    frames, grays = [], []
                    for t in range(T):
                        p, gr = rt.ingest_raw(torch.from_numpy(mosaic[t:t + 1].view(np.int16)).cuda(), 12, "mosaic")
                        frames.append(p)
                        grays.append(gr)
                    if mode != "off":
                        e, level, state = rt.green_estimate(torch.cat(frames), rule, 12, "gbrg")
                        gmap, _, st = green_fit(e, level, state, black, (T + 1) // 2, 3.0, 0.10, 4095.0 / 64.0)
                        if mode == "flat":
                            gmap = np.full((1, 1), st["flat_gain"], np.float32)
                        zero = zero and not gmap.any()
                        dev = torch.from_numpy(gmap).cuda()
                        for p, gr in zip(frames, grays):
                            rt.green_apply(p, dev, black, 12, gray=gr, pattern="gbrg")
                        tot = {k: [v] if tot is None else tot[k] + [v] for k, v in st.items()}
                    rt.reset()
                    for t in range(1, T):
                        out = rt.step(frames[t - 1], frames[t], None, fl[t][None], None)
                        outs.append(out.clone())
                        if t >= 2:
                            ps.append(10.0 * math.log10(4.0 / float(((out.double() - gt[t][None].double()) ** 2).mean())))
                if mode == "off":
                    plain_out = outs
                note = ""
                if tot is not None:
                    blocks = seeds * (H // 64) * (W // 64)
                    note = "  green: %d applied, %d insignificant, %d unsupported, %d clamped of %d blocks, map rms gain %.5f, floor %.5f, flat %s" % (
                        sum(tot["applied"]) + sum(tot["clamped"]), sum(tot["insignificant"]), sum(tot["unsupported"]), sum(tot["clamped"]), blocks,
                        (sum(tot["sum_q2"]) / blocks) ** 0.5 / 16384.0, sum(tot["floor"]) / seeds, " / ".join("%.5f" % v for v in tot["flat_gain"]))
                    if zero:
                        same = all(torch.equal(x, y) for x, y in zip(outs, plain_out))
                        assert same, "a map of zeros changed the outputs"
                        note += "  (the map is zero: the outputs are bit for bit those without the stage)"
                lines.append("ISO %-5d imbalance %4.1f %% %-6s stage %-4s | PSNR %6.2f dB%s"
                             % (iso, 100.0 * gain, "ramped" if ramped else "flat", mode, sum(ps) / len(ps), note))
        rt.close()
    emit(lines)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
