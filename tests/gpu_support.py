"""What the GPU tests share, once: the batch-0 ops handle, uploads on and off a 16-byte boundary, the exact comparison of two lists
of frames, handles with their weights and options, the synthetic sequences stepped by (video, frame), and the bytes of a results
tree.  A plain module: pytest does not rewrite its asserts, so each one carries its message."""
import math
import os

import numpy as np
import torch

from conftest import load_weights


def ops_rt():
    from rvdd_release_amd.util._ops import ops_runtime
    return ops_runtime(0)


def bits_of(t):
    """the 32-bit words of a device tensor, on the host"""
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def upload(a, offset=False, fill=None):
    """A NumPy array or a tensor on the device, in an allocation of its own.  offset False: on a 16-byte boundary.  offset True:
    four bytes behind one, so that the one-sample kernel forms run; an int: that many bytes behind one.  With `fill` the rest of
    the allocation (the bytes in front, seven elements behind) holds that value and (view, whole allocation) comes back, for the
    checks that nothing outside the view is written."""
    t = a
    if not torch.is_tensor(a):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a)      # torch has no uint32 everywhere: the same words
    at = 4 if offset is True else int(offset)
    k, rest = divmod(at, t.element_size())
    assert rest == 0, ("upload: an offset of whole elements", at, t.dtype)
    whole = torch.empty(k + t.numel() + 7, dtype=t.dtype, device="cuda") if fill is None else \
        torch.full((k + t.numel() + 7,), fill, dtype=t.dtype, device="cuda")
    v = whole[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert whole.data_ptr() % 16 == 0 and v.data_ptr() % 16 == at % 16, ("upload", whole.data_ptr() % 16, v.data_ptr() % 16, at)
    return v if fill is None else (v, whole)


def same(got, want, what="", allow_empty=False):
    """two lists of tensors: as long as each other, every tensor finite and equal bit for bit.  An empty `want` proves nothing and
    is refused, unless the caller says that it compares two empty lists on purpose."""
    assert len(got) == len(want) and (allow_empty or len(want) > 0), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(g).all() and torch.equal(g, w), (what, k, float((g - w).abs().max()))


def parity_psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 200.0 if mse == 0 else 10 * math.log10(4.0 / mse)


def make_runtime(arch, weights, future, B, H, W, **options):
    """a handle with `weights` (a stem under weights/, or a state dict) loaded and the options set"""
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime(arch, future, B, H, W, 0)
    rt.load_state_dict(load_weights(weights) if isinstance(weights, str) else weights)
    for k, v in options.items():
        rt.set_option(k, v)
    return rt


def dpc_rule(k_hot, k_dead, a, b, floor=1.0):
    from rvdd_release_amd.runtime import dpc_cfg
    return dpc_cfg(k_hot, k_dead, a, b, floor)


def launches(rt):
    return {p["name"]: (p["launches"], p["bytes"]) for p in rt.profile_read() if p["launches"]}


def files_of(res):
    """{path below `res`: the file's bytes}"""
    out = {}
    for d, _, names in os.walk(res):
        for name in names:
            with open(os.path.join(d, name), "rb") as f:
                out[os.path.relpath(os.path.join(d, name), res)] = f.read()
    return out


# ---- synthetic sequences with their analytic flows, stepped by (video, frame) ------------------------------------------------------
def synth_videos(lengths, H, W, future, seed0=500):
    from rvdd_release_amd import synth
    return [synth.make_sequence(T + future, H, W, iso=3200, seed=seed0 + v, device="cuda") for v, T in enumerate(lengths)]


def frames_of(seq, future):
    return seq.raw.shape[0] - future


def step_frames(rt, seqs, frame, future, live=None):
    """One step over frame = [(video, t)] * n."""
    st = lambda f: torch.stack([f(seqs[v], t) for v, t in frame])
    return rt.step(st(lambda s, t: s.raw[t - 1]), st(lambda s, t: s.raw[t]), st(lambda s, t: s.raw[t + 1]) if future else None,
                   st(lambda s, t: s.flow_prev[t]), st(lambda s, t: s.flow_next[t]) if future else None, live=live)


def run_alone(arch, sd, future, seqs, H, W, opts):
    """Each video on a batch-1 handle from rvdd_reset: -> per video, its output frames [T-1-f, 3, H, W]."""
    rt = make_runtime(arch, sd, future, 1, H, W, **opts)
    outs = []
    for v, s in enumerate(seqs):
        rt.reset()
        outs.append(torch.cat([step_frames(rt, seqs, [(v, t)], future).clone() for t in range(1, frames_of(s, future))]))
    rt.close()
    return outs
