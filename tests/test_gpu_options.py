"""rvdd_set_option: every option is a field of the handle it is set on (one table in handle.hip), the measurement hook
leaves the handle's conv selection as it found it, and every documented name is known with its range."""
import os
import re

import pytest
import torch

from conftest import REPO, load_weights
from gpu_support import launches as _launches, make_runtime, step_frames as _step, synth_videos as _videos

pytestmark = pytest.mark.gpu


def test_debug_bench_leaves_the_selection():
    """conv_kernel 2 (Winograd at every size) survives rvdd_debug_conv_bench.  96 x 128 is 48 units of 32 x 8 pixels, below
    the 200 at which selection by size takes Winograd: a handle that came back as conv_kernel 4 would launch the direct kernel."""
    H, W = 96, 128
    assert ((W + 31) // 32) * ((H + 7) // 8) < 200
    sd = load_weights("recurrent-convunet-iso3200")
    seqs = _videos([3], H, W, 0, seed0=1500)
    frames = []
    for hook in (False, True):
        rt = make_runtime("convunet", sd, 0, 1, H, W, conv_kernel=2)
        if hook:
            rt.debug_conv_bench(0, 1, 1)
        rt.reset()
        rt.profile_enable(True)
        frames.append(_step(rt, seqs, [(0, 1)], 0).clone())
        seen = _launches(rt)
        rt.profile_enable(False)
        rt.close()
        assert any(k.startswith("wino3x3") for k in seen), (hook, sorted(seen))
        assert not any(k.startswith("conv3x3_kernel<") for k in seen), (hook, sorted(seen))
    assert torch.equal(frames[0], frames[1]), float((frames[0] - frames[1]).abs().max())


def test_switches_are_per_handle():
    """A handle with cout_split 0 and small_prestage 0 beside one with the defaults, stepped alternately, in both orders of
    creation: both give the frames and features of a default handle run alone (the two forms of either switch give the same
    bits, so this guards against a crash or mixed-up state; which kernels ran is shown by profiles/opt_*_kernel_stats.csv).
    64 x 96 is 24 tiles of 16 x 16: the output-channel split and the one-kernel pre-stage apply at every level."""
    H, W, T = 64, 96, 3
    arch, off = "convunet+feat", {"cout_split": 0, "small_prestage": 0}
    sd = load_weights("recurrent-convunet+feat-iso3200")
    seqs = _videos([T + 1], H, W, 0, seed0=1600)

    alone = make_runtime(arch, sd, 0, 1, H, W)
    alone.reset()
    want = [_step(alone, seqs, [(0, t)], 0).clone() for t in range(1, T + 1)]
    want_feat = alone.get_state()[1].clone()
    alone.close()

    for b_first in (False, True):
        if b_first:
            b = make_runtime(arch, sd, 0, 1, H, W)
            a = make_runtime(arch, sd, 0, 1, H, W, **off)
        else:
            a = make_runtime(arch, sd, 0, 1, H, W, **off)
            b = make_runtime(arch, sd, 0, 1, H, W)
        a.reset()
        b.reset()
        for t in range(1, T + 1):
            for tag, rt in (("A", a), ("B", b)):
                got = _step(rt, seqs, [(0, t)], 0)
                assert torch.equal(got, want[t - 1]), (b_first, tag, t, float((got - want[t - 1]).abs().max()))
        for tag, rt in (("A", a), ("B", b)):
            assert torch.equal(rt.get_state()[1], want_feat), (b_first, tag)
        a.close()
        b.close()


def test_every_option_round_trips():
    """Every name include/rvdd.h documents takes its default value; the three ranged options refuse a value outside their
    range; an unknown name is refused with the full list of known ones."""
    txt = open(os.path.join(REPO, "include", "rvdd.h")).read()
    doc = txt[txt.index("Known names:"):txt.index("int rvdd_set_option(")]
    documented = re.findall(r'^ \*   "([a-z0-9_]+)"', doc, flags=re.M)
    assert len(documented) == len(set(documented)) >= 20
    on = {"fuse_upsample", "next_split", "next_pipe", "next_pool", "next_projfuse", "block_fp", "fuse_pre", "pre5_cin8", "cout_split",
          "small_prestage"}                                   # default 1; every other option defaults to 0
    assert on <= set(documented)
    rt = make_runtime("convunet", load_weights("recurrent-convunet-iso3200"), 0, 1, 32, 48)
    lib, h = rt.lib, rt.h
    for name in documented:
        assert lib.rvdd_set_option(h, name.encode(), 1 if name in on else 0) == 0, (name, lib.rvdd_last_error(h).decode())
    for name, bad in (("conv_kernel", 3), ("seq_major", 2), ("bayer_pattern", 4)):
        assert lib.rvdd_set_option(h, name.encode(), bad) == -1, (name, bad)          # RVDD_ERR_ARG
        assert name in lib.rvdd_last_error(h).decode()
    assert lib.rvdd_set_option(h, b"bogus", 0) == -1
    msg = lib.rvdd_last_error(h).decode()
    m = re.search(r"unknown option 'bogus' \(known: ([a-z0-9_, ]+)\)", msg)
    assert m, msg
    assert sorted(m.group(1).split(", ")) == sorted(documented)
    # the handle still steps with every default in place
    seqs = _videos([2], 32, 48, 0, seed0=1700)
    rt.reset()
    assert torch.isfinite(_step(rt, seqs, [(0, 1)], 0)).all()
    rt.close()
