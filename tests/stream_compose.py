"""What rvdd_video_push must equal, once: compose() makes the outputs of a video from the stand-alone entry points of a batch-1
handle, and push_schedule() walks a schedule of pushes.  With them the ctl words, the two fixed schedules and the small videos the
stream tests share.  tests/test_stream_compose_host.py pins compose()'s sequence of runtime calls and the schedules on the CPU.
A plain module: pytest does not rewrite its asserts, so each one carries its message."""
from collections import namedtuple

import numpy as np
import torch

import bits_ref
import stream_ref
from gpu_support import make_runtime
from stream_ref import mosaic_of, quantised_dn

NEXT, FIRST, IDLE = 0, 1, 2
OFF = (IDLE, -1, -1)                                          # a slot that sits a push out

# (arch, weights stem, future, options): the handles test_gpu_stream.py and test_gpu_stream_all.py compose
CASES = [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {}),
    ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, {}),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, {}),
    ("convunet", "recurrent-convunet-iso3200", 0, {"no_warp": 1}),
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, {"bayer_pattern": 2}),
    ("convunet", "non_recurrent-convunet-iso3200", 0, {"stream_reset_each": 1}),
]


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def compose(rt, video, future, *, all_frames=False, no_warp=False, reset_each=False, from_denoised=False, bit_depth=12, dmap=False,
            dpc=None, match=None, to_gpu=None):
    """The outputs of a video (uint16 mosaics [N,H,W]) through the EXISTING entry points of a batch-1 handle that has none of the
    stream's stages and options set (`dmap`: it carries the map):
      per frame    ingest_raw -> (dmap: dpc_map_apply, packed and gray in place) -> (dpc: packed corrected out of place, gray patched)
                   -> (match: match_raw on the packed frame).  The gray planes stay the sensor's.
      centres      1 .. N-1-future; all_frames ("stream_all_frames"): every frame, with the head c = 0 and, with a future frame, the
                   tail c = N-1 (N = 1: both in one step).  A head has itself as its previous frame, a tail itself as its next.
      flows        tvl1flow_batch(gray_c, gray of the neighbour); zero towards a head's previous and a tail's next frame; none at all
                   with no_warp.  from_denoised ("stream_flow_from_denoised"): from c = 2 on the previous frame's gray plane is
                   gray_of_rgb(previous output) -- the un-mapped output, and never a head's.
      step         reset() where c <= 1 (reset_each: on every step), step(), and with `match` unmatch_rgb on the output.
    -> [one output per centre]"""
    to_gpu = to_gpu or stream_ref.to_gpu
    N = video.shape[0]
    pg = []
    for t in range(N):
        p, g = rt.ingest_raw(to_gpu(video[t:t + 1]), bit_depth, "mosaic")
        if dmap:
            rt.dpc_map_apply(p, bit_depth, gray=g)
        if dpc is not None:
            p = rt.dpc(p, dpc, bit_depth, gray=g)
        if match is not None:
            p = rt.match_raw(p, match)
        pg.append((p, g))
    outs = []
    for c in (range(N) if all_frames else range(1, N - future)):
        head, tail = c == 0, bool(future) and c == N - 1
        prev = pg[c] if head else pg[c - 1]
        nxt = (pg[c] if tail else pg[c + 1]) if future else None
        fp = fn = None
        if not no_warp:
            g = pg[c][1]
            zeros = torch.zeros(g.shape[0], 2, g.shape[1], g.shape[2], device=g.device)
            if head:
                fp = zeros
            else:
                fp = rt.tvl1flow_batch(g, rt.gray_of_rgb(outs[-1], bit_depth) if from_denoised and c >= 2 else pg[c - 1][1])
            if future:
                fn = zeros if tail else rt.tvl1flow_batch(g, pg[c + 1][1])
        if c <= 1 or reset_each:
            rt.reset()
        out = rt.step(prev[0], pg[c][0], nxt[0] if future else None, fp, fn)
        outs.append(out.clone() if match is None else rt.unmatch_rgb(out, match))
    return outs


# ---- the pushes ---------------------------------------------------------------------------------------------------------------------
Pushed = namedtuple("Pushed", "by_slot by_video flags")       # {slot: [outputs]}, {video: [outputs]}, [the valid flags of every push]


def push_schedule(rt, videos, steps, bit_depth=12, container=None, between=None, after=None):
    """Push `steps` -- per push one (ctl, video, frame) per slot, as denoise.deal_slots deals them -- of uint16 mosaics `videos`
    (NumPy, [N,H,W] each; `container`: bit-packed into it on the way, bits_ref.pack).  A slot on IDLE gets a frame that is not read.
    between(i, frames) runs before push i, after(i, out) behind it.  -> Pushed; every output is a [1,3,H,W] clone."""
    B = len(steps[0])
    H, W = videos[0].shape[1:]
    got = Pushed({s: [] for s in range(B)}, {v: [] for v in range(len(videos))}, [])
    for i, step in enumerate(steps):
        if container is None:
            batch = np.zeros((B, H, W), np.uint16)
        else:
            batch = np.full((B, H, bits_ref.row_bytes(W, bit_depth, container)), 0xFF, np.uint8)
        for s, (c, v, k) in enumerate(step):
            if c != IDLE:
                batch[s] = videos[v][k] if container is None else bits_ref.pack(videos[v][k], bit_depth, container)
        frames = stream_ref.to_gpu(batch) if container is None else torch.from_numpy(batch).cuda()
        if between is not None:
            between(i, frames)
        out, valid = rt.video_push(frames, [c for c, _, _ in step], bit_depth, "mosaic", container=container)
        got.flags.append(list(valid))
        for s, (c, v, k) in enumerate(step):
            if valid[s]:
                got.by_slot[s].append(out[s:s + 1].clone())
                if v >= 0:
                    got.by_video[v].append(got.by_slot[s][-1])
        if after is not None:
            after(i, out)
    return got


def push_alone(rt, video, future, bit_depth=12, idle=False):
    """One video through a batch-1 handle: FIRST, NEXT ..., and with a future frame and `idle` one IDLE, the push that gives the tail
    of "stream_all_frames".  -> (outputs, the valid flag of every push)"""
    N = video.shape[0]
    steps = [[(FIRST if t == 0 else NEXT, 0, t)] for t in range(N)] + ([[(IDLE, 0, N)]] if future and idle else [])
    got = push_schedule(rt, [video], steps, bit_depth)
    return got.by_slot[0], [f[0] for f in got.flags]


def two_slot_schedule(videos):
    """Slot 0: video 0, one IDLE, video 2, one IDLE; slot 1: video 1, then IDLE."""
    a, b, c = (len(v) for v in videos)
    assert a == b, ("two_slot_schedule: videos 0 and 1 are as long as each other", a, b)
    s = [[(FIRST if t == 0 else NEXT, 0, t), (FIRST if t == 0 else NEXT, 1, t)] for t in range(a)]
    s.append([OFF, OFF])
    s += [[(FIRST if t == 0 else NEXT, 2, t), OFF] for t in range(c)]
    s.append([OFF, OFF])
    return s


def mid_stream_schedule(B, T, slot=5, short=3):
    """B slots, video b of T frames in slot b; `slot` holds video B, of `short` frames, first and starts its own video mid-stream; the
    others idle at the end."""
    steps = []
    for t in range(T + short):
        at = lambda b: t - short if b == slot else t
        steps.append([(FIRST if t == 0 else NEXT, B, t) if b == slot and t < short else
                      (FIRST if at(b) == 0 else NEXT, b, at(b)) if at(b) < T else OFF for b in range(B)])
    return steps


def push_two_slots(rt, videos, bits=12, container=None):
    """two_slot_schedule(videos) pushed, then the deferred check of the pushes' flow batches.  -> {slot: [outputs in order]}"""
    got = push_schedule(rt, videos, two_slot_schedule(videos), bits, container).by_slot
    rt.set_option("tvl1_async", 0)                            # nothing gave up
    return got


# ---- videos -------------------------------------------------------------------------------------------------------------------------
def synth_video(T, H, W, seed, iso=3200, device="cpu"):
    """T whole-DN 12-bit frames as uint16 mosaics [T,H,W] (numpy)."""
    from rvdd_release_amd import synth
    s = synth.make_sequence(T, H, W, iso=iso, seed=seed, device=device)
    return mosaic_of(quantised_dn(s.raw.cpu())).astype(np.uint16)


SMALL = 32                                                    # 16 x 16 cells: the least rvdd_video_push takes
SMALL_STEM = {0: "recurrent-convunet-iso3200", 1: "recurrent-convunet-future-iso3200"}
STATIC = [(0, 0, 0, "hot"), (1, 3, 4, "hot"), (2, 10, 2, "dead"), (0, 6, 6, "hot"), (0, 6, 7, "hot"), (3, 15, 15, "dead"), (3, 0, 9, "hot")]


def small_runtime(future, B, **options):
    return make_runtime("convunet", SMALL_STEM[future], future, B, SMALL, SMALL, **options)


def small_videos(bits=12, defects=True):
    """three videos of 5, 5 and 3 frames of 32 x 32 sites, uint16 mosaics of `bits` bits, with a hot and a dead sample per frame that
    move from frame to frame (and stay clear of each other)"""
    out = []
    for v, T in enumerate((5, 5, 3)):
        m = synth_video(T, SMALL, SMALL, seed=300 + v) >> (12 - bits)
        if defects:
            for t in range(T):
                m[t, 2 * (3 + v) + (t & 1), 2 * (4 + t) + 1] = 2 ** bits - 1      # hot: plane 1 or 3, cell (3 + v, 4 + t)
                m[t, 2 * 10 + 1, 2 * (2 + 2 * t)] = 0                               # dead: plane 2, cell (10, 2 + 2 t)
                m[t, 0, 0] = 2 ** bits - 1                                          # hot in the frame's corner, plane 0
        out.append(m)
    return out


def static_videos(bits=12):
    """small_videos without the moving defects, with the same static defects in every frame of every video: singles in every plane,
    at a corner and on an edge, and an equal hot pair.  -> (videos, cellmask [16,16])"""
    videos = small_videos(bits=bits, defects=False)
    mask = np.zeros((SMALL // 2, SMALL // 2), np.uint8)
    for k, y, x, kind in STATIC:
        mask[y, x] |= 1 << k
        for m in videos:
            m[:, 2 * y + (k >> 1), 2 * x + (k & 1)] = 2 ** bits - 1 if kind == "hot" else 0
    return videos, mask
