#!/usr/bin/env python3
"""What the column-noise correction gains and costs on footage whose truth is known.

    python tools/cols_study.py [SEEDS]       synth sequences of 13 frames of 384 x 256 (12 outputs each), SEEDS (default 2) seeds, both
                                             checkpoint families (recurrent-convunet+feat-iso3200 / -iso12800 on footage of their own
                                             curve, analytic flows).  The frames are quantised to uint16 mosaics on the host, one STATIC
                                             Gaussian offset per mosaic column of sigma_col = 0, 1/8, 1/4 and 1/2 of the pixel noise at the
                                             mid level is added there -- the same in every frame of a sequence --, and they come back
                                             through rvdd_ingest_raw.  Per case, with the stage off and on (rvdd_cols_estimate on the
                                             sequence's 13 frames, rvdd_cols_fit with min_frames 7, k_sig 3 and clamp top / 64, the
                                             family's curve and a gate of 3, then rvdd_cols_apply on every frame): the PSNR of outputs
                                             2..12 against the scene, the residual report's ratio and rho (rvdd_resid_stats /
                                             rvdd_resid_fit against the family's curve: what a user without ground truth sees), and the
                                             map's counts, rms and floor.
    The line at sigma_col = 0 is the price of switching the stage on blindly.

Prints its lines and appends them to profiles/cols_study.txt (or the file named by COLS_STUDY_OUT)."""
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T, H, W = 13, 256, 384


def emit(lines):
    path = os.environ.get("COLS_STUDY_OUT", os.path.join(REPO, "profiles", "cols_study.txt"))
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
    from rvdd_release_amd.runtime import DPC_ISO_CURVES, RvddRuntime, cols_cfg, cols_fit, resid_fit
    assert torch.cuda.is_available(), "cols_study needs a GPU"
    lines = ["cols_study: %d seeds, %d frames of %d x %d, recurrent-convunet+feat, 12 outputs per case, PSNR of outputs 2..12; the map from the "
             "sequence's own %d frames: gate 3, min_frames %d, k_sig 3, clamp %.1f DN" % (seeds, T, W, H, T, (T + 1) // 2, 4095.0 / 64.0)]
    for iso in DPC_ISO_CURVES:
        a, b = DPC_ISO_CURVES[iso]
        sigma = math.sqrt(a * 2047.5 - b)
        rule = cols_cfg(3.0, a, b, 1.0)
        rt = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
        rt.load_state_dict(load_file(os.path.join(REPO, "weights", "recurrent-convunet+feat-iso%d.safetensors" % iso)))
        lines.append("ISO %d: pixel sigma at the mid level %.1f DN" % (iso, sigma))
        for share in (0.0, 0.125, 0.25, 0.5):
            for on in (False, True):
                ps, reps, tot = [], [], None
                for seed in range(seeds):
                    seq = synth.make_sequence(T, H, W, iso=iso, seed=seed, device="cuda")
                    gt, fl = seq.gt.cuda(), seq.flow_prev.cuda()
                    dn = torch.round((seq.raw.double() + 1.0) / 2.0 * 4095.0).clamp(0, 4095).cpu().numpy()          # [T,4,hh,ww]
                    mosaic = np.zeros((T, H, W), np.float64)
                    for k in range(4):
                        mosaic[:, (k >> 1)::2, (k & 1)::2] = dn[:, k]
                    rng = np.random.default_rng(1000 * iso + seed)
                    mosaic = np.clip(np.rint(mosaic + share * sigma * rng.standard_normal((1, 1, W))), 0, 4095).astype(np.uint16)
                    frames, grays = [], []
                    for t in range(T):
                        p, g = rt.ingest_raw(torch.from_numpy(mosaic[t:t + 1].view(np.int16)).cuda(), 12, "mosaic")
                        frames.append(p)
                        grays.append(g)
                    if on:
                        offsets, state = rt.cols_estimate(torch.cat(frames), rule, 12)
                        cmap, _, st = cols_fit(offsets, state, (T + 1) // 2, 3.0, 4095.0 / 64.0)
                        dev = torch.from_numpy(cmap).cuda()
                        for p, g in zip(frames, grays):
                            rt.cols_apply(p, dev, 12, gray=g)
                        st["floor_sum"] = st.pop("floor_dn")
                        tot = st if tot is None else {k: tot[k] + v for k, v in st.items()}
                    rt.reset()
                    resid = None
                    for t in range(1, T):
                        out = rt.step(frames[t - 1], frames[t], None, fl[t][None], None)
                        resid = rt.resid_stats(frames[t], out, 12, "gbrg", acc=resid)
                        if t >= 2:
                            ps.append(10.0 * math.log10(4.0 / float(((out.double() - gt[t][None].double()) ** 2).mean())))
                    reps.append(resid_fit(resid, 12, a, b))
                cols = "" if tot is None else "  cols: %d applied, %d insignificant, %d unsupported, %d clamped, map rms %.2f DN, floor %.2f DN" % (
                    tot["applied"] + tot["clamped"], tot["insignificant"], tot["unsupported"], tot["clamped"],
                    (tot["sum_q2"] / (seeds * W)) ** 0.5 / 16.0, tot["floor_sum"] / seeds)
                lines.append("ISO %-5d sigma_col %5.1f DN (%5.3f sigma) stage %-3s | PSNR %6.2f dB  ratio %s  rho %s%s"
                             % (iso, share * sigma, share, "on" if on else "off", sum(ps) / len(ps), " / ".join("%.3f" % r["ratio"] for r in reps),
                                " / ".join("%+.4f" % r["rho"] for r in reps), cols))
        rt.close()
    emit(lines)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 2)
