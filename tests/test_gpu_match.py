"""Footage matched to the checkpoint's noise curve on the device: rvdd_match_raw / rvdd_unmatch_rgb against their NumPy restatement
(tests/match_ref.py) bit for bit, the argument errors, the round trip of every DN through ingest, map, demosaic, way back and egress,
the stage inside rvdd_video_push (rvdd_set_match) against the same schedule made by hand on a batch-1 handle, `denoise --match_noise`
end to end, and the quality the map buys on noisy footage."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import dpc_ref
import match_ref as R
import noise_ref
from conftest import WEIGHTS, load_weights
from gpu_support import bits_of as _bits, files_of as _files, ops_rt as _rt, same as _same, upload as _up
from stream_compose import compose, push_two_slots as _push_all, small_runtime as _runtime, small_videos as _videos
from stream_ref import mosaic_of, to_gpu

pytestmark = pytest.mark.gpu

CAM60 = R.camera_curve(60.0, 256)                         # noisier than both checkpoint curves against ISO 3200: s = 0.133
CAM3 = R.camera_curve(3.0, 256)                           # cleaner: s = 2.67


def _coeffs(curve, iso=3200, bits=12):
    from rvdd_release_amd.runtime import match_coeffs
    return match_coeffs(curve[0], curve[1], bits, iso)[0]


def _samples(shape, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.25, 1.25, size=shape).astype(np.float32)
    flat = v.reshape(-1)
    special = np.array([0.0, -0.0, 1.0, -1.0, 3e38, 0.33333334], np.float32)
    flat[:min(flat.size, special.size)] = special[:flat.size]
    return v


# ---- 1. the kernels are the restatement ---------------------------------------------------------------------------------------
RAW_SHAPES = [(3, 5, 7), (1, 1, 1), (2, 8, 16)]
RGB_SHAPES = [(2, 6, 10), (1, 16, 32), (1, 3, 3)]         # the last: 27 samples, no multiple of 4 -- the one-sample form on aligned pointers


@pytest.mark.parametrize("which,shape", [("raw", s) for s in RAW_SHAPES] + [("rgb", s) for s in RGB_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else "%dx%dx%d" % v)
def test_kernels_are_the_restatement(which, shape):
    rt = _rt()
    n, d0, d1 = shape
    c = 4 if which == "raw" else 3
    call, ref = (rt.match_raw, R.match_raw_ref) if which == "raw" else (rt.unmatch_rgb, R.unmatch_rgb_ref)
    v = _samples((n, c, d0, d1), seed=n * 1000 + d0 * 10 + d1)
    for curve, iso in ((CAM60, 3200), (CAM3, 3200), (CAM60, 12800), (R.ISO_CURVES[3200], 3200)):
        cfg = _coeffs(curve, iso)
        with np.errstate(over="ignore"):
            want = ref(v, cfg.scale, cfg.offset).view(np.uint32)
        if curve == R.ISO_CURVES[3200]:
            assert (cfg.scale, cfg.offset) == (1.0, 0.0)
        else:
            assert not np.array_equal(want, v.view(np.uint32))
        got = []
        for offset in (False, True):                      # aligned: the wide form where the count allows; offset: the one-sample form
            src = _up(v, offset)
            out = _up(np.full(v.shape, 7.0, np.float32), offset)
            assert call(src, cfg, out=out) is out
            torch.cuda.synchronize()
            assert np.array_equal(_bits(src), v.view(np.uint32))      # out of place: the input is not touched
            got.append(_bits(out))
            assert call(src, cfg, out=src) is src          # in place
            got.append(_bits(src))
            # one aligned, one not: the one-sample form again
            got.append(_bits(call(_up(v, offset), cfg, out=_up(np.zeros_like(v), not offset))))
        got.append(_bits(call(torch.from_numpy(v).cuda(), cfg)))      # a new tensor
        for k, g in enumerate(got):
            assert np.array_equal(g, want), (which, shape, curve, iso, k, np.argwhere(g != want)[:4].tolist())


def test_empty_batch_and_argument_errors_launch_nothing():
    from rvdd_release_amd import _lib
    rt = _rt()
    n, hh, ww = 2, 8, 16
    nan, inf = float("nan"), float("inf")
    for fn, name, c, in_name, out_name, d0, d1 in ((rt.lib.rvdd_match_raw, "rvdd_match_raw", 4, "packed_in", "packed_out", "hh", "ww"),
                                                    (rt.lib.rvdd_unmatch_rgb, "rvdd_unmatch_rgb", 3, "rgb_in", "rgb_out", "H", "W")):
        src = torch.full((n, c, hh, ww), 0.5, device="cuda")
        out = torch.full((n, c, hh, ww), 7.0, device="cuda")

        def call(pin=0, pout=0, n_=n, d0_=hh, d1_=ww, cfg=(0.5, 0.25)):
            s = None if cfg is None else C.byref(_lib.RvddMatchCfg(*cfg))
            rc = fn(rt.h, src.data_ptr() if pin == 0 else pin, out.data_ptr() if pout == 0 else pout, n_, d0_, d1_, s, None)
            return rc, rt.lib.rvdd_last_error(rt.h).decode()

        bad = [(dict(cfg=None), "cfg"), (dict(n_=-1), r"\bn\b"), (dict(d0_=0), r"\b%s\b" % d0), (dict(d1_=0), r"\b%s\b" % d1),
               (dict(d0_=-3), r"\b%s\b" % d0), (dict(pin=None), in_name), (dict(pout=None), out_name),
               (dict(pout=src.data_ptr() + 16), out_name), (dict(pin=out.data_ptr() + 4 * (n * c * hh * ww - 1)), out_name),
               (dict(n_=2 ** 31 - 1, d0_=2 ** 10, d1_=2 ** 10), "blocks")]
        bad += [(dict(cfg=(v, 0.0)), "scale") for v in (0.0, -1.0, nan, inf, -inf)]
        bad += [(dict(cfg=(1.0, v)), "offset") for v in (nan, inf, -inf)]
        for kwargs, names in bad:
            rc, msg = call(**kwargs)
            assert rc == -1 and msg.startswith(name + ":") and re.search(names, msg), (name, kwargs, rc, msg)
        assert call(n_=0)[0] == 0                             # an empty batch is fine and does nothing ...
        assert call(n_=0, pin=None, pout=None)[0] == 0        # ... and needs no tensors
        torch.cuda.synchronize()
        assert (out == 7).all() and (src == 0.5).all()
    # rvdd_set_match validates the same way, and a refused call leaves the stage as it was (off: identity checked further down)
    for cfg, field in (((nan, 0.0), "scale"), ((0.0, 0.0), "scale"), ((-2.0, 0.0), "scale"), ((inf, 0.0), "scale"), ((1.0, nan), "offset"),
                       ((1.0, inf), "offset")):
        assert rt.lib.rvdd_set_match(rt.h, C.byref(_lib.RvddMatchCfg(*cfg))) == -1
        msg = rt.lib.rvdd_last_error(rt.h).decode()
        assert msg.startswith("rvdd_set_match:") and field in msg
    with pytest.raises(RuntimeError, match="match_raw: the frames are"):
        rt.match_raw(torch.zeros(1, 3, 4, 4, device="cuda"), _coeffs(CAM60))
    with pytest.raises(RuntimeError, match=r"rvdd_unmatch_rgb failed \(-1\).*cfg"):
        rt.unmatch_rgb(torch.zeros(1, 3, 4, 4, device="cuda"), None)


# ---- 2. every DN comes back ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,side", [(12, 64), (10, 32)])
def test_device_round_trip_returns_every_dn(bits, side):
    """ingest_raw -> match_raw -> demosaic -> unmatch_rgb -> egress(u16, mosaic): the frames come back exactly.  Two frames hold every
    DN of the bit depth, in two different orders."""
    rt = _rt()
    rng = np.random.default_rng(bits)
    assert side * side == 2 ** bits
    frames = np.stack([rng.permutation(2 ** bits), np.arange(2 ** bits)]).reshape(2, side, side).astype(np.uint16)
    dev = to_gpu(frames)
    packed, _ = rt.ingest_raw(dev, bits, "mosaic")
    plain = rt.egress(rt.demosaic(packed, "gbrg"), "mosaic", torch.int16, bits, "gbrg")
    assert torch.equal(plain, dev)                            # the path itself returns the frames: the maps are what is tested
    # the camera's curve in DN of the frames' bit depth: the same camera, its DN scaled
    k = (2 ** bits - 1) / 4095.0
    for a, b in (CAM60, CAM3):
        for iso in (3200, 12800):
            cfg = _coeffs((k * a, k * k * b), iso, bits)
            mapped = rt.match_raw(packed, cfg)
            assert not torch.equal(mapped, packed)
            rgb = rt.demosaic(mapped, "gbrg")
            back = rt.egress(rt.unmatch_rgb(rgb, cfg, out=rgb), "mosaic", torch.int16, bits, "gbrg")
            assert torch.equal(back, dev), (bits, a, iso, int((back != dev).sum()))


# ---- 3. the stage inside the stream ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("all_frames", [0, 1])
@pytest.mark.parametrize("future", [0, 1])
def test_stream_with_the_stage_is_the_composition(future, all_frames):
    videos = _videos(defects=False)
    cfg = _coeffs(CAM60)
    rt = _runtime(future, 2, stream_all_frames=all_frames)
    rt.set_match(cfg)
    got = _push_all(rt, videos)
    alone = _runtime(future, 1)
    want = [compose(alone, v, future, all_frames=all_frames, match=cfg) for v in videos]
    _same(got[0], want[0] + want[2], "slot 0")
    _same(got[1], want[1], "slot 1")
    # the stage matters: the same pushes with it off give other outputs, those of a handle that never had it
    rt.set_match(None)
    plain = _push_all(rt, videos)
    assert not torch.equal(plain[0][0], got[0][0])
    never = _push_all(_runtime(future, 2, stream_all_frames=all_frames), videos)
    for s in range(2):
        _same(plain[s], never[s], "off, slot %d" % s)


def test_stage_with_flows_from_denoised():
    videos = _videos(defects=False)
    cfg = _coeffs(CAM60)
    rt = _runtime(1, 2, stream_flow_from_denoised=1)
    rt.set_match(cfg)
    got = _push_all(rt, videos)
    alone = _runtime(1, 1)
    want = [compose(alone, v, 1, match=cfg, from_denoised=True) for v in videos]
    _same(got[0], want[0] + want[2], "slot 0")
    _same(got[1], want[1], "slot 1")
    # the plane matters here: the composition on the noisy pairs gives other outputs from the second one on
    noisy = compose(alone, videos[0], 1, match=cfg)
    assert torch.equal(noisy[0], want[0][0]) and not torch.equal(noisy[1], want[0][1])


def test_stage_behind_the_correction():
    """DPC first, in the sensor's domain with the sensor's curve, then the map"""
    from rvdd_release_amd.runtime import dpc_cfg
    videos = _videos()
    a, b = dpc_ref.iso_curve(3200, 12)
    dpc = dpc_cfg(4, 4, a, b)
    cfg = _coeffs(CAM60)
    rt = _runtime(1, 2, stream_all_frames=1)
    rt.set_dpc(dpc)
    rt.set_match(cfg)
    got = _push_all(rt, videos)
    alone = _runtime(1, 1)
    want = [compose(alone, v, 1, all_frames=True, match=cfg, dpc=dpc) for v in videos]
    _same(got[0], want[0] + want[2], "slot 0")
    _same(got[1], want[1], "slot 1")
    assert all(h >= 10 and d >= 5 for h, d in rt.dpc_counts())
    uncorrected = compose(alone, videos[0], 1, all_frames=True, match=cfg)
    assert not torch.equal(uncorrected[0], want[0][0])


def test_stage_on_mipi_raw10_is_the_stage_on_the_unpacked_frames():
    videos = _videos(bits=10, defects=False)
    k = 1023.0 / 4095.0
    cfg = _coeffs((k * CAM60[0], k * k * CAM60[1]), 3200, 10)
    assert abs(cfg.scale - _coeffs(CAM60).scale) < 1e-6
    mipi = _runtime(1, 2, stream_all_frames=1)
    mipi.set_match(cfg)
    got = _push_all(mipi, videos, bits=10, container="mipi")
    alone = _runtime(1, 1)
    want = [compose(alone, v, 1, all_frames=True, match=cfg, bit_depth=10) for v in videos]
    _same(got[0], want[0] + want[2], "slot 0")
    _same(got[1], want[1], "slot 1")


@pytest.mark.parametrize("future", [0, 1])
def test_identity_coefficients_are_the_plain_stream(future):
    from rvdd_release_amd.runtime import match_cfg
    videos = _videos(defects=False)
    on = _runtime(future, 2, stream_all_frames=1)
    on.set_match(match_cfg(1.0, 0.0))
    never = _runtime(future, 2, stream_all_frames=1)
    got, want = _push_all(on, videos), _push_all(never, videos)
    for s in range(2):
        _same(got[s], want[s], s)


# ---- 4. denoise end to end ------------------------------------------------------------------------------------------------------
Hc, Wc, T = 64, 96, 4                                       # cells: the size at which tests/test_noise_host.py fits four frames


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """2 videos of 4 frames of noise_ref's smooth scene with the ISO 12800 curve, 12 bits, as uint16 TIFFs"""
    from rvdd_release_amd import tiffio
    root = tmp_path_factory.mktemp("match_tree")
    for v in range(2):
        m = mosaic_of(noise_ref.scene_cells(T, Hc, Wc, 12, 12800, seed=40 + v)).astype(np.uint16)
        os.makedirs(root / "u16" / ("%03d" % v))
        for t in range(T):
            tiffio.write(str(root / "u16" / ("%03d/%08d.tif" % (v, t))), m[t])
    return root


def test_denoise_auto_is_denoise_with_the_printed_numbers(tree, tmp_path, capsys, monkeypatch):
    from rvdd_release_amd import denoise, noise
    from rvdd_release_amd.runtime import match_coeffs
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--dataroot", str(tree), "--nFolder", "u16"]

    def run(name, *more):
        capsys.readouterr()
        res = str(tmp_path / name)
        stats = denoise.main(flags + ["--results_dir", res] + list(more))
        out = capsys.readouterr().out.splitlines()
        assert stats["frames"] == 2 * (T - 1)
        return (_files(res), [ln[len("noise: "):] for ln in out if ln.startswith("noise: ")],
                [ln[len("match: "):] for ln in out if ln.startswith("match: ")])

    typed = match_line = None
    for B in (1, 2):
        auto, line, match = run("auto%d" % B, "--match_noise", "auto", "--match_iso", "3200", "--batch_size", str(B))
        assert len(line) == 1 and len(match) == 1 and len(auto) == 2 * (T - 1)
        ab = re.search(r'"a": (\S+), "b": (\S+),', line[0])
        typed = "%s,%s" % (ab.group(1), ab.group(2))
        cfg, s, t = match_coeffs(float(ab.group(1)), float(ab.group(2)), 12, 3200)
        assert json.loads(match[0]) == {"scale": cfg.scale, "offset": cfg.offset, "s": s, "t_dn12": t, "iso": 3200}
        assert 0.2 < s < 0.4                                  # 8.0034 / 28.3015 = 0.283, and the estimate is within a few per cent
        same, none, match_ab = run("ab%d" % B, "--match_noise", typed, "--match_iso", "3200", "--batch_size", str(B))
        assert none == [] and match_ab == match and same == auto
        assert match_line in (None, match[0])
        match_line = match[0]
    # both on auto: one estimate, one `noise:` line, and the same map
    calls = []
    estimate = noise.estimate
    monkeypatch.setattr(noise, "estimate", lambda *a, **k: calls.append(1) or estimate(*a, **k))
    both, line, match = run("both", "--dpc", "1e18", "--dpc_noise", "auto", "--match_noise", "auto", "--match_iso", "3200", "--batch_size", "2")
    assert calls == [1] and len(line) == 1 and match == [match_line] and both == auto      # a correction that flags nothing
    # without the flags no estimate, no line, the plain stream's files: those of the identity map, and not those of the map
    monkeypatch.setattr(noise, "estimate", lambda *a, **k: pytest.fail("an estimate without auto"))
    plain, line, match = run("plain", "--batch_size", "2")
    assert line == [] and match == [] and sorted(plain) == sorted(auto) and plain != auto
    ident, line, match = run("ident", "--match_noise", "8.0034,2043.51144", "--match_iso", "3200", "--batch_size", "2")
    assert ident == plain and len(match) == 1 and json.loads(match[0])["scale"] == 1.0 and json.loads(match[0])["offset"] == 0.0
    # footage cleaner than the curve is mapped all the same, with the warning
    capsys.readouterr()
    denoise.main(flags + ["--results_dir", str(tmp_path / "warn"), "--match_noise", "3,668", "--match_iso", "12800", "--batch_size", "2"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("match: ")]
    assert len(out) == 2 and "WARNING" in out[1] and "9.43" in out[1]


def test_noise_command_prints_the_match_line(tree, capsys):
    from rvdd_release_amd import noise
    from rvdd_release_amd.runtime import match_coeffs
    args = ["--dataroot", str(tree), "--nFolder", "u16", "--bit_depth", "12"]
    capsys.readouterr()
    noise.main(args)
    first = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("{", "match: "))]
    r = noise.main(args + ["--match_iso", "12800"])
    out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(("{", "match: "))]
    assert len(first) == 1 and len(out) == 2 and out[0] == first[0] and out[1].startswith("match: {")
    cfg, s, t = match_coeffs(r["a"], r["b"], 12, 12800)
    assert json.loads(out[1][len("match: "):]) == {"scale": cfg.scale, "offset": cfg.offset, "s": s, "t_dn12": t, "iso": 12800}
    with pytest.raises(SystemExit, match="--match_iso must be one of"):
        noise.main(args + ["--match_iso", "6400"])


# ---- 5. it helps where it should --------------------------------------------------------------------------------------------------
def test_matching_gains_3_db_on_footage_noisier_than_the_curve():
    """The recipe of DESIGN.md 4.16: make_sequence(6, 96, 128, iso=3200, seed=0), camera a = 60, b = 60 * 256 - 100 at 12 bits, noise
    seed 5, analytic flows, recurrent-convunet+feat-iso3200; mean PSNR of outputs 2..5 against the scene.  The f32 oracle measured
    33.47 dB unmatched and 36.98 dB matched, +3.51 dB; the bound of 3.0 dB leaves half a dB for the split-f16 path.
    Measured on the device: unmatched 33.475 dB, matched 36.981 dB, +3.506 dB."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    seq = synth.make_sequence(6, 96, 128, iso=3200, seed=0)
    cam = R.camera_frames(seq.gt, *CAM60).cuda()
    cfg = _coeffs(CAM60)
    rt = RvddRuntime("convunet+feat", 0, 1, 96, 128, 0)
    rt.load_state_dict(load_weights("recurrent-convunet+feat-iso3200"))
    fl, gt = seq.flow_prev.cuda(), seq.gt.cuda()

    def run(frames, back):
        rt.reset()
        ps = []
        for t in range(1, 6):
            out = back(rt.step(frames[t - 1][None], frames[t][None], None, fl[t][None], None))
            if t >= 2:
                ps.append(R.psnr(out, gt[t][None]))
        return sum(ps) / len(ps)

    unmatched = run(cam, lambda o: o)
    matched = run(rt.match_raw(cam, cfg), lambda o: rt.unmatch_rgb(o, cfg))
    print("unmatched %.3f dB, matched %.3f dB, gain %.3f dB" % (unmatched, matched, matched - unmatched))
    assert matched - unmatched >= 3.0, (unmatched, matched)
