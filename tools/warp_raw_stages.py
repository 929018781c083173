#!/usr/bin/env python3
"""--warp_raw stage by stage against the oracle, per Bayer pattern (GPU box): a 10-frame sequence at 74x106 whose oracle is
restarted from the runtime's state each step; at every step the re-demosaic of the previous output is compared stage by
stage -- the warp of its re-mosaicked planes (rvdd_warp_bicubic, the step's kernel, against the oracle's grid_sample) and
Hamilton-Adams of the warped planes (the device's HamiltonAdam(P) against tests/bayer_ref.py on the SAME input, and on each
side's own warp).  usage: python tools/warp_raw_stages.py   (one line per pattern / seed)"""
import sys, os, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import rvdd_oracle as O, bayer_ref as R
from rvdd_release_amd import synth
from rvdd_release_amd.runtime import RvddRuntime
from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
from safetensors.torch import load_file
torch.set_num_threads(16)
for pattern, seed, fut in [("rggb", 335, 1), ("rggb", 328, 0), ("bggr", 338, 0), ("gbrg", 328, 0)]:
    T, H, W = 10, 74, 106
    stem = "recurrent-convunet-future-iso3200" if fut else "recurrent-convunet-iso3200"
    sd = load_file(os.path.join(ROOT, "weights", stem + ".safetensors"))
    seq = synth.make_sequence(T, H, W, seed=seed, pattern=pattern)
    rt = RvddRuntime("convunet", fut, 1, H, W, 0); rt.load_state_dict(sd)
    rt.set_option("warp_raw", 1); rt.set_option("bayer_pattern", R.PATTERNS.index(pattern))
    ops = RvddRuntime("convunet", 0, 1, 16, 16, 0)
    raw, fp, fn = seq.raw.cuda(), seq.flow_prev.cuda(), seq.flow_next.cuda()
    line = []
    for t in range(1, T - fut):
        if t > 1:
            lastden = rt.get_state(want_feat=False)[0].cpu()
            packed = R.remosaick(lastden, pattern)
            w_dev = ops.warp(packed.cuda(), fp[t][None]).cpu()
            w_cpu = O.warp(packed, seq.flow_prev[t][None])
            ha_dev = HamiltonAdam(pattern)(w_cpu.cuda()).cpu()
            ha_cpu = R.hamilton_adams(w_cpu, pattern)
            ha_dev_w = HamiltonAdam(pattern)(w_dev.cuda()).cpu()
            line.append(f"t{t}: warp {float((w_dev - w_cpu).abs().max()):.1e} (n{int((w_dev != w_cpu).sum())}) "
                        f"HA-same-input {float((ha_dev - ha_cpu).abs().max()):.1e} HA(dev warp)-HA(cpu warp) {float((ha_dev_w - ha_cpu).abs().max()):.1e}")
        rt.step(raw[t - 1][None] if t == 1 else None, raw[t][None], raw[t + 1][None] if fut else None, fp[t][None],
                fn[t][None] if fut else None)
    rt.close(); ops.close()
    print(pattern, seed, fut, " | ".join(line), flush=True)
