"""Defective-pixel correction on the device: rvdd_dpc against its NumPy restatement (tests/dpc_ref.py) bit for bit, the frame in
which nothing is flagged, one side off, the argument errors, and the stage inside rvdd_video_push (rvdd_set_dpc) against the same
schedule made by hand from the existing entry points, with rvdd_dpc_counts.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import dpc_ref as R
from gpu_support import bits_of as _bits, dpc_rule as _cfg, ops_rt as _rt, same as _same, upload
from stream_compose import compose, push_two_slots as _push_all, small_runtime as _runtime, small_videos as _videos
from stream_ref import cells_of

pytestmark = pytest.mark.gpu

SHAPES = [(1, 2, 2), (1, 3, 5), (3, 16, 20), (2, 18, 17), (1, 16, 24)]
CLASSES = {"corner", "edge", "pair", "marginal", "batch", "plane0", "plane1", "plane2", "plane3"}


def _run(rt, packed, gray, counts0, bits, cfg, offset=False):
    up = lambda a: upload(a, offset=offset)
    p, g, c = up(packed), up(gray), up(np.asarray(counts0, np.int32))
    out = up(np.zeros_like(packed))
    rt.dpc(p, cfg, bits, gray=g, counts=c, out=out)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(p), np.ascontiguousarray(packed).view(np.uint32))      # the input is not touched
    return out, g, c


# ---- 1. parity with the restatement ----------------------------------------------------------------------------------------
def test_reference_fires_on_every_class():
    """On the reference alone: over the shapes below every class of injected defect is flagged, and the marginal one refused."""
    seen = set()
    for n, hh, ww in SHAPES:
        packed, gray, sites = R.make_case(n, hh, ww, 12, 3200, seed=11)
        a, b = R.iso_curve(3200, 12)
        _, _, _, hot, dead = R.dpc_ref(packed, gray, 12, 4, 4, a, b)
        seen |= R.check_sites(sites, hot, dead)
    assert seen == CLASSES


@pytest.mark.parametrize("n,hh,ww", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_dpc_is_the_restatement(n, hh, ww):
    rt = _rt()
    for bits in (10, 12, 14, 16):
        for iso in (3200, 12800):
            packed, gray, sites = R.make_case(n, hh, ww, bits, iso, seed=100 * bits + iso % 7)
            a, b = R.iso_curve(iso, bits)
            counts0 = np.arange(7, 7 + 2 * n).reshape(n, 2)            # accumulation: the counters do not start at zero
            want_p, want_g, want_c, hot, dead = R.dpc_ref(packed, gray, bits, 4, 4, a, b, 1.0, counts=counts0)
            # a parity test on frames where nothing fires proves nothing: every class injected into this shape fired
            seen = R.check_sites(sites, hot, dead)
            assert {s[0] for s in sites} <= seen and {"corner", "plane0", "plane1", "plane2", "plane3"} <= seen
            for cls, i, k, y, x, kind in sites:
                if kind == "marginal":                                  # above its largest neighbour, and refused
                    dn = ((packed[i, k] + np.float32(1)) * np.float32(0.5)) * np.float32(2 ** bits - 1)
                    assert dn[y, x] > max(dn[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)
            assert (want_c > counts0).any() and not np.array_equal(want_g, gray)
            cfg = _cfg(4, 4, a, b)
            out, g, c = _run(rt, packed, gray, counts0, bits, cfg)
            what = (n, hh, ww, bits, iso)
            assert np.array_equal(_bits(out), want_p.view(np.uint32)), what
            assert np.array_equal(_bits(g), want_g.view(np.uint32)), what
            assert np.array_equal(c.cpu().numpy(), want_c), (what, c.cpu().numpy(), want_c)
            if (hh, ww) == (16, 24):
                # every pointer 4 bytes off a 16-byte boundary: the one-cell form on a shape the wide form takes -- the same bits
                out1, g1, c1 = _run(rt, packed, gray, counts0, bits, cfg, offset=True)
                assert np.array_equal(_bits(out1), _bits(out)) and np.array_equal(_bits(g1), _bits(g)) and torch.equal(c1, c), what


# ---- 2. nothing flagged -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hh,ww", [(1, 2, 2), (2, 18, 17), (3, 16, 20)])
def test_nothing_flagged_is_a_bit_copy(n, hh, ww):
    rt = _rt()
    packed, _, _ = R.make_case(n, hh, ww, 12, 12800, seed=5)
    a, b = R.iso_curve(12800, 12)
    sentinel = np.frombuffer(bytes([0xA5]) * (4 * n * hh * ww), dtype=np.float32).reshape(n, hh, ww).copy()
    out, g, c = _run(rt, packed, sentinel, np.full((n, 2), 3), 12, _cfg(1e18, 1e18, a, b))      # 1e18 squared is +inf in f32
    assert np.array_equal(_bits(out), packed.view(np.uint32))
    assert g.cpu().numpy().tobytes() == sentinel.tobytes() and (c == 3).all()
    # gray and counts are optional
    out2 = rt.dpc(torch.from_numpy(packed).cuda(), _cfg(1e18, 1e18, a, b), 12)
    assert np.array_equal(_bits(out2), packed.view(np.uint32))


# ---- 3. one side off --------------------------------------------------------------------------------------------------------
def test_one_side_off():
    rt = _rt()
    n, hh, ww = 2, 18, 17
    packed, gray, sites = R.make_case(n, hh, ww, 12, 3200, seed=9)
    a, b = R.iso_curve(3200, 12)
    zero = np.zeros((n, 2), np.int64)
    for k_hot, k_dead in ((0, 4), (4, 0)):
        want_p, want_g, want_c, hot, dead = R.dpc_ref(packed, gray, 12, k_hot, k_dead, a, b, counts=zero)
        out, g, c = _run(rt, packed, gray, zero, 12, _cfg(k_hot, k_dead, a, b))
        assert np.array_equal(_bits(out), want_p.view(np.uint32)) and np.array_equal(_bits(g), want_g.view(np.uint32))
        c = c.cpu().numpy()
        assert np.array_equal(c, want_c) and c[:, 0 if k_hot == 0 else 1].sum() == 0 and c[:, 1 if k_hot == 0 else 0].sum() > 0
        off, on = ("hot", "dead") if k_hot == 0 else ("dead", "hot")
        for cls, i, k, y, x, kind in sites:
            same = _bits(out)[i, k, y, x] == packed.view(np.uint32)[i, k, y, x]
            assert same if kind in (off, "marginal") else not same, (cls, kind, k_hot, k_dead)


# ---- 4. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from rvdd_release_amd import _lib
    rt = _rt()
    n, hh, ww = 1, 16, 20
    p = torch.zeros(n, 4, hh, ww, device="cuda")
    out = torch.full((n, 4, hh, ww), 7.0, device="cuda")
    gray = torch.full((n, hh, ww), 7.0, device="cuda")
    counts = torch.full((n, 2), 7, dtype=torch.int32, device="cuda")
    a, b = R.iso_curve(3200, 12)
    good = dict(k_hot=4.0, k_dead=4.0, noise_a=a, noise_b=b, var_floor=1.0)
    nan, inf = float("nan"), float("inf")

    def call(pin=None, pout=None, n_=n, hh_=hh, ww_=ww, bits=12, cfg=good):
        c = None if cfg is None else C.byref(_lib.RvddDpcCfg(*(float(cfg[f]) for f, _ in _lib.RvddDpcCfg._fields_)))
        rc = rt.lib.rvdd_dpc(rt.h, (p if pin is None else pin).data_ptr(), out.data_ptr() if pout is None else pout, gray.data_ptr(), n_, hh_, ww_,
                             bits, c, counts.data_ptr(), None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    bad = [(dict(pout=p.data_ptr()), "packed_out"), (dict(pout=p.data_ptr() + 16), "packed_out"),
           (dict(pin=out), "packed_out"),
           (dict(hh_=1), "hh"), (dict(ww_=1), "ww"), (dict(hh_=0), "hh"), (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"),
           (dict(cfg=None), "cfg"), (dict(n_=-1), r"\bn\b"),
           (dict(n_=2 ** 31 - 1), "blocks")]                 # 16 x 5 threads of the wide form are two blocks per frame
    for field, values in (("k_hot", (-1.0, nan, inf)), ("k_dead", (-0.5, nan, inf)), ("noise_a", (nan, inf, -inf)), ("noise_b", (nan, inf)),
                          ("var_floor", (0.0, -1.0, nan))):
        bad += [(dict(cfg=dict(good, **{field: v})), field) for v in values]
    import re
    for kwargs, names in bad:
        rc, msg = call(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_dpc:") and re.search(names, msg), (kwargs, rc, msg)
    assert call(n_=0)[0] == 0                                 # an empty batch is fine and does nothing
    torch.cuda.synchronize()
    assert (out == 7).all() and (gray == 7).all() and (counts == 7).all() and (p == 0).all()
    # rvdd_set_dpc validates the same way, and a refused call leaves the stage as it was
    for field, v in (("k_hot", nan), ("k_dead", -1.0), ("noise_a", inf), ("noise_b", nan), ("var_floor", 0.0)):
        cfg = _lib.RvddDpcCfg(*(float(dict(good, **{field: v})[f]) for f, _ in _lib.RvddDpcCfg._fields_))
        assert rt.lib.rvdd_set_dpc(rt.h, C.byref(cfg)) == -1
        msg = rt.lib.rvdd_last_error(rt.h).decode()
        assert msg.startswith("rvdd_set_dpc:") and field in msg
    assert rt.dpc_counts() == [(0, 0)] * rt.B


# ---- 5 - 7. the stage inside the stream -------------------------------------------------------------------------------------
@pytest.mark.parametrize("all_frames", [0, 1])
@pytest.mark.parametrize("future", [0, 1])
def test_stream_with_the_stage_is_the_composition(future, all_frames):
    videos = _videos()
    a, b = R.iso_curve(3200, 12)
    cfg = _cfg(4, 4, a, b)
    # the reference's flags per video: every frame has its hot and its dead sample
    totals = []
    for v in videos:
        p, g = R.ingest(cells_of(v, "mosaic"), 12)
        c = R.dpc_ref(p, g, 12, 4, 4, a, b)[2]
        assert (c[:, 0] >= 2).all() and (c[:, 1] >= 1).all(), c
        totals.append(c.sum(axis=0))
    rt = _runtime(future, 2, stream_all_frames=all_frames)
    rt.set_dpc(cfg)
    got = _push_all(rt, videos)
    assert rt.dpc_counts() == [tuple(int(x) for x in totals[0] + totals[2]), tuple(int(x) for x in totals[1])]
    alone = _runtime(future, 1)
    want = [compose(alone, v, future, all_frames=all_frames, dpc=cfg) for v in videos]
    _same(got[0], want[0] + want[2], "slot 0")
    _same(got[1], want[1], "slot 1")
    # the stage matters on these frames: the same pushes without it give other outputs
    rt.set_dpc(None)
    plain = _push_all(rt, videos)
    assert not torch.equal(plain[0][0], got[0][0])
    assert rt.dpc_counts() == [tuple(int(x) for x in totals[0] + totals[2]), tuple(int(x) for x in totals[1])]      # off: nothing more is counted
    rt.set_dpc(cfg)                                           # switched on again: the totals start again
    assert rt.dpc_counts() == [(0, 0), (0, 0)]


@pytest.mark.parametrize("future", [0, 1])
def test_stage_that_finds_nothing_is_the_plain_stream(future):
    videos = _videos(defects=False)
    a, b = R.iso_curve(3200, 12)
    on = _runtime(future, 2, stream_all_frames=1)
    on.set_dpc(_cfg(1e18, 1e18, a, b))
    never = _runtime(future, 2, stream_all_frames=1)
    got, want = _push_all(on, videos), _push_all(never, videos)
    for s in range(2):
        _same(got[s], want[s], s)
    assert on.dpc_counts() == [(0, 0), (0, 0)] and never.dpc_counts() == [(0, 0), (0, 0)]


def test_stage_on_mipi_raw10_is_the_stage_on_the_unpacked_frames():
    videos = _videos(bits=10)
    a, b = R.iso_curve(3200, 10)
    cfg = _cfg(4, 4, a, b)
    future = 1
    plain = _runtime(future, 2, stream_all_frames=1)
    plain.set_dpc(cfg)
    want = _push_all(plain, videos, bits=10)
    mipi = _runtime(future, 2, stream_all_frames=1)
    mipi.set_dpc(cfg)
    got = _push_all(mipi, videos, bits=10, container="mipi")
    for s in range(2):
        _same(got[s], want[s], s)
    counts = mipi.dpc_counts()
    assert counts == plain.dpc_counts() and all(h >= 10 and d >= 5 for h, d in counts[:1])
