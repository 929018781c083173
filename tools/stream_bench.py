#!/usr/bin/env python3
"""Frames/s of the raw-footage stream (`RvddRuntime.video_push`: ingest + TV-L1 flows + frame-step per push, everything on
the device) beside the same handle stepping with the flows computed beforehand (the form of bench.py's headline), on
synthetic uint16 mosaics.  Two JSON lines: {"mode": "stream"} and {"mode": "step_flows_at_hand"}.

usage (GPU box, repo root):  timeout -k 10 600 python tools/stream_bench.py --config C2 [--batch 8] [--frames 12] [--warmup 3]
                             [--flow-from-denoised] [--all-frames] [--video-len N]
One process, no retries: a failure is the exit status."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from rvdd_release_amd import _lib, synth  # noqa: E402
from rvdd_release_amd.runtime import RvddRuntime  # noqa: E402
from safetensors.torch import load_file  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="C2", choices=sorted(bench.CONFIGS))
ap.add_argument("--batch", type=int, default=None)
ap.add_argument("--frames", type=int, default=12, help="pushes timed per slot")
ap.add_argument("--warmup", type=int, default=3, help="pushes before the clock starts (they fill the rings)")
ap.add_argument("--no-sampler", action="store_true", help="do not sample the shader clock (rocm-smi) beside the loops")
ap.add_argument("--flow-from-denoised", action="store_true",
                help="option stream_flow_from_denoised: flows towards the previous frame against the previous output (stream mode only)")
ap.add_argument("--all-frames", action="store_true",
                help="option stream_all_frames: every frame of a video is output; with a future frame each video ends with one IDLE push "
                     "(stream mode only)")
ap.add_argument("--video-len", type=int, default=None,
                help="frames per video: every slot streams its warmup + frames frames as videos of this length, one after the other "
                     "(default: one video)")
args = ap.parse_args()
arch, stem, fut, iso, H, W, _, B0, _ = bench.CONFIGS[args.config]
B = args.batch or B0
T = args.warmup + args.frames
assert args.warmup >= 2 + fut, "the warm-up must fill the rings (2 + future pushes)"
dev = torch.device("cuda", 0)

# whole 12-bit DN, one sequence per slot: [T,B,H,W] uint16 mosaics, uploaded before the clock starts (as int16: same bits)
frames = torch.empty(T, B, H, W, dtype=torch.int16, device=dev)
for b in range(B):
    raw = synth.make_sequence(T, H, W, iso=iso, seed=500 + b, device="cuda").raw
    dn = torch.round((raw + 1.0) / 2.0 * 4095.0).clamp(0, 4095).to(torch.int16)          # [T,4,h,w]
    for k in range(4):
        frames[:, b, (k >> 1)::2, (k & 1)::2] = dn[:, k]
del raw, dn

rt = RvddRuntime(arch, fut, B, H, W, 0)
rt.load_state_dict(load_file(os.path.join(REPO, "weights", stem + ".safetensors")))
rt.set_option("stream_flow_from_denoised", int(args.flow_from_denoised))
rt.set_option("stream_all_frames", int(args.all_frames))
sampler = None if args.no_sampler else bench.GpuSampler(0, 0.05)


def clock(t0, t1):
    if sampler is None:
        return {}
    w = sampler.window(t0, t1)
    return {k: w[k] for k in ("sclk_mhz_mean", "sclk_mhz_min", "samples") if k in w}


common = {"config": args.config, "arch": arch, "future": fut, "batch": B, "height": H, "width": W, "frames_per_slot": args.frames,
          "flow_from_denoised": bool(args.flow_from_denoised)}
V = args.video_len or T
assert V >= 1
# the pushes of a slot: (ctl, frame); with --all-frames and a future frame every video is followed by the IDLE that outputs its last frame
pushes = []
for t in range(T):
    pushes.append((_lib.PUSH_FIRST if t % V == 0 else _lib.PUSH_NEXT, t))
    if args.all_frames and fut and (t % V == V - 1 or t == T - 1):
        pushes.append((_lib.PUSH_IDLE, t))

# ---- the stream --------------------------------------------------------------------------------------------------------
out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
outputs = timed = 0
for i, (c, t) in enumerate(pushes):
    if i == args.warmup:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.timer_start()
    _, valid = rt.video_push(frames[t], [c] * B, 12, "mosaic", out)
    if i >= args.warmup:
        outputs += sum(valid)
        timed += 1
ms = rt.timer_stop_ms()
t1 = time.perf_counter()
rt.set_option("tvl1_async", 0)              # the deferred check of every flow batch above
if V == T and not args.all_frames:
    assert outputs == B * args.frames
print(json.dumps(dict(common, mode="stream", all_frames=bool(args.all_frames), video_len=V, pushes=timed, outputs=outputs,
                      fps=round(outputs / (ms * 1e-3), 2), ms_per_push=round(ms / timed, 3), **clock(t0, t1))))
sys.stdout.flush()
rt.set_option("stream_all_frames", 0)

# ---- the same handle, flows at hand ----------------------------------------------------------------------------------------
packed = torch.empty(T, B, 4, H // 2, W // 2, dtype=torch.float32, device=dev)
gray = torch.empty(T, B, H // 2, W // 2, dtype=torch.float32, device=dev)
for t in range(T):
    packed[t], gray[t] = rt.ingest_raw(frames[t], 12, "mosaic")
fp = [None] + [rt.tvl1flow_batch(gray[t], gray[t - 1]) for t in range(1, T)]
fn = [rt.tvl1flow_batch(gray[t], gray[t + 1]) for t in range(T - 1)] + [None] if fut else [None] * T
rt.reset()
first, steps = 1, 0
for c in range(1, T - fut):
    if c == args.warmup - fut:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rt.timer_start()
        first = c
    rt.step(packed[c - 1], packed[c], packed[c + 1] if fut else None, fp[c], fn[c], out)
steps = T - fut - first
ms = rt.timer_stop_ms()
t1 = time.perf_counter()
print(json.dumps(dict(common, mode="step_flows_at_hand", fps=round(B * steps / (ms * 1e-3), 2), ms_per_step=round(ms / steps, 3), **clock(t0, t1))))
sys.stdout.flush()
if sampler is not None:
    sampler.close()
rt.close()        # before the interpreter tears the HIP runtime down (a profiler's exit handlers run after that)
