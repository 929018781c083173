#!/usr/bin/env python3
"""BASELINE's C2 workload (convunet+feat ISO3200, B = 8 sequences of 1280x720) with the handle's Bayer pattern set, for a
kernel-trace comparison of the pre-stage across patterns (bench.py has no pattern switch and stays as it is):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/bayer_c2.py rggb [STEPS]

Prints one JSON line: pattern, steps, frames/s (wall clock over the timed steps, after one untimed step)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import torch  # noqa: E402
from safetensors.torch import load_file  # noqa: E402
from rvdd_release_amd import synth  # noqa: E402
from rvdd_release_amd.runtime import BAYER_PATTERNS, RvddRuntime  # noqa: E402

pattern = sys.argv[1] if len(sys.argv) > 1 else "gbrg"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
arch, stem, fut, iso, H, W, _, B, _ = bench.CONFIGS["C2"]
seqs = [synth.make_sequence(steps + 2, H, W, iso=iso, seed=4000 + b, device="cuda", pattern=pattern) for b in range(B)]
raw = torch.stack([s.raw for s in seqs], 1).contiguous()
fp = torch.stack([s.flow_prev for s in seqs], 1).contiguous()
del seqs
rt = RvddRuntime(arch, fut, B, H, W, 0)
rt.load_state_dict(load_file(os.path.join(bench.REPO, "weights", stem + ".safetensors")))
rt.set_option("bayer_pattern", BAYER_PATTERNS.index(pattern))
out = torch.empty(B, 3, H, W, device="cuda")
rt.step(raw[0], raw[1], None, fp[1], None, out=out)
torch.cuda.synchronize()
t0 = time.perf_counter()
for t in range(2, steps + 2):
    rt.step(None, raw[t], None, fp[t], None, out=out)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(json.dumps({"pattern": pattern, "config": "C2", "steps": steps, "frames_per_s": round(B * steps / dt, 2),
                  "out_checksum": float(out.double().abs().sum())}))
rt.close()
