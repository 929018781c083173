#!/usr/bin/env python3
"""What the residual report reads on footage whose truth is known.

    python tools/resid_study.py [SEEDS]      synth sequences of 13 frames of 384 x 256 (12 outputs each), SEEDS (default 3) seeds, both
                                             checkpoint families (recurrent-convunet+feat-iso3200 / -iso12800 on footage of their own
                                             curve, analytic flows).  Per case the report of rvdd_resid_stats / rvdd_resid_fit over the
                                             12 outputs, and the true PSNR of outputs 2..12 against the scene:
      matched        the family's own footage, judged against its curve: the BASELINE (the ratio is not 1: the output keeps some noise)
      scale 0.5 / 2  the footage's DN scaled by s (a camera with another gain: curve s a, s^2 b), unmatched, judged against that curve
      wrong family   the other family's network on the footage, judged against the footage's curve
      match x0.5/x2  --match_noise with a curve that is off by that factor (a and b alike), judged as `denoise` judges matched footage:
                     in the network's domain against the family's curve
      black +16      the footage's DN shifted by 16, unmatched, judged against the unshifted curve
    A case counts as SEPARATED in a figure when its range over the seeds lies outside the baseline's range over the seeds.

Prints its lines and appends them to profiles/resid_study.txt (or the file named by RESID_STUDY_OUT)."""
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

T, H, W = 13, 256, 384
FIGURES = ("ratio", "ratio_lo", "ratio_hi", "rho", "bias")


def emit(lines):
    path = os.environ.get("RESID_STUDY_OUT", os.path.join(REPO, "profiles", "resid_study.txt"))
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        for ln in lines:
            print(ln)
            f.write(ln + "\n")


def main(seeds):
    import torch
    from safetensors.torch import load_file
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import DPC_ISO_CURVES, RvddRuntime, match_coeffs, resid_fit
    assert torch.cuda.is_available(), "resid_study needs a GPU"
    nets = {}
    for iso in DPC_ISO_CURVES:
        nets[iso] = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
        nets[iso].load_state_dict(load_file(os.path.join(REPO, "weights", "recurrent-convunet+feat-iso%d.safetensors" % iso)))

    def affine(x, s, t_dn):                    # DN x' = s x + t on samples in [-1,1]
        return (s * x + ((s - 1.0) + 2.0 * t_dn / 4095.0)).contiguous()

    def run(rt, frames, gt, flows, curve, pre=None):
        """frames: the footage as the camera gave it; pre: the map of --match_noise (the stage's domain is then the mapped one)"""
        inp = frames if pre is None else rt.match_raw(frames, pre)
        rt.reset()
        acc, ps = None, []
        for t in range(1, T):
            out = rt.step(inp[t - 1][None], inp[t][None], None, flows[t][None], None)
            acc = rt.resid_stats(inp[t][None], out, 12, "gbrg", acc=acc)
            if t >= 2:
                user = out if pre is None else rt.unmatch_rgb(out, pre)
                ps.append(10.0 * math.log10(4.0 / float(((user.double() - gt[t][None].double()) ** 2).mean())))
        rep = resid_fit(acc, 12, *curve)
        rep["psnr"] = sum(ps) / len(ps)
        return rep

    lines = ["resid_study: %d seeds, %d frames of %d x %d, recurrent-convunet+feat, 12 outputs per report, PSNR of outputs 2..12" % (seeds, T, W, H)]
    for iso, other in ((3200, 12800), (12800, 3200)):
        a, b = DPC_ISO_CURVES[iso]
        table = {}
        for seed in range(seeds):
            seq = synth.make_sequence(T, H, W, iso=iso, seed=seed, device="cuda")
            raw, gt, fl = seq.raw.cuda(), seq.gt.cuda(), seq.flow_prev.cuda()
            rt = nets[iso]
            cases = [("matched", rt, raw, gt, (a, b), None)]
            for s in (0.5, 2.0):
                cases.append(("scale %.1f" % s, rt, affine(raw, s, 0.0), affine(gt, s, 0.0), (s * a, s * s * b), None))
            cases.append(("wrong family", nets[other], raw, gt, (a, b), None))
            for k in (0.5, 2.0):
                cases.append(("match x%.1f" % k, rt, raw, gt, (a, b), match_coeffs(k * a, k * b, 12, iso)[0]))
            cases.append(("black +16", rt, affine(raw, 1.0, 16.0), affine(gt, 1.0, 16.0), (a, b), None))
            for name, net, frames, truth, curve, pre in cases:
                rep = run(net, frames, truth, fl, curve, pre)
                table.setdefault(name, []).append(rep)
                lines.append("ISO %-5d %-12s seed %d | ratio %6.3f  lo %6.3f  hi %6.3f  rho %+7.4f  bias %+7.2f DN  a_fit %7.3f  b_fit %9.1f  bins %2d | PSNR %6.2f dB"
                             % (iso, name, seed, rep["ratio"], rep["ratio_lo"], rep["ratio_hi"], rep["rho"], rep["bias"], rep["a_fit"], rep["b_fit"],
                                rep["bins"], rep["psnr"]))
        base = table["matched"]
        span = lambda reps, k: (min(r[k] for r in reps), max(r[k] for r in reps))
        for name, reps in table.items():
            cells = []
            for k in FIGURES + ("psnr",):
                lo, hi = span(reps, k)
                blo, bhi = span(base, k)
                mark = "" if name == "matched" or k == "psnr" else (" SEP" if lo > bhi or hi < blo else " -  ")
                cells.append("%s %.3f..%.3f%s" % (k, lo, hi, mark))
            lines.append("ISO %-5d %-12s over %d seeds | %s" % (iso, name, seeds, "  ".join(cells)))
    emit(lines)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 3)
