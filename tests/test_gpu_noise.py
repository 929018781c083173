"""The noise-curve estimate on the device: every integer of rvdd_noise_hist's accumulator against the NumPy restatement
(tests/noise_ref.py), the argument errors, the fit of a device accumulator, and `denoise --dpc_noise auto` against the same run with
the printed numbers typed in.  Every comparison is exact."""
import json
import os
import re

import numpy as np
import pytest
import torch

import bits_ref
import dpc_ref
import noise_ref as R
from conftest import WEIGHTS
from gpu_support import files_of as _files, ops_rt as _rt, upload

pytestmark = pytest.mark.gpu

F = np.float32


def _arrays(acc):
    from rvdd_release_amd.runtime import noise_acc_arrays
    return noise_acc_arrays(acc)


def _same(got, want, what=""):
    """every integer of a device accumulator (or its arrays) against the reference's"""
    got = got if isinstance(got, dict) else _arrays(got)
    for k in ("hist", "msum", "counters"):
        assert torch.equal(torch.from_numpy(got[k]), torch.from_numpy(want[k])), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


def _hist(packed, bits, acc=None, offset=False):
    p = upload(packed, offset=offset)
    if not offset:
        assert p.data_ptr() % 16 == 0
    acc = _rt().noise_hist(p, bits, acc)
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy().view(np.uint32), np.ascontiguousarray(packed).view(np.uint32))      # the input is not touched
    return acc


def _packed(n, hh, ww, bits=12, iso=3200, seed=0, **more):
    return dpc_ref.ingest(R.scene_cells(n, hh, ww, bits, iso, seed, **more), bits)[0]


# ---- 1. the accumulators ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hh,ww", [(1, 8, 8), (1, 13, 21), (3, 24, 40), (2, 17, 30), (1, 64, 264)])
def test_accumulator_is_the_restatement(n, hh, ww):
    """one block per plane; remainders dropped (one-sample form: 21 and 30 are no multiples of 4); several frames, both forms; and
    (1, 64, 264): 8 x 33 blocks per plane, 1056 in all -- more than four workgroups, the last one partly filled"""
    p = _packed(n, hh, ww, seed=n + hh)
    want = R.noise_hist_ref(p, 12)
    assert want["counters"][0] == n * 4 * (hh // 8) * (ww // 8) and want["hist"].sum() > 0
    _same(_hist(p, 12), want, "aligned")
    _same(_hist(p, 12, offset=True), want, "offset by 4 bytes")


def test_zero_blocks_leave_the_buffer_alone():
    rt = _rt()
    acc = torch.full((32904,), 7, dtype=torch.int32, device="cuda")
    for shape in ((1, 4, 7, 40), (2, 4, 40, 7), (0, 4, 16, 16), (1, 4, 0, 16)):
        rt.noise_hist(torch.zeros(shape, device="cuda"), 12, acc)
    # NULL packed is fine where there is no block
    assert rt.lib.rvdd_noise_hist(rt.h, None, 1, 7, 40, 12, acc.data_ptr(), None) == 0
    assert rt.lib.rvdd_noise_hist(rt.h, None, 0, 16, 16, 12, acc.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (acc == 7).all()


def test_one_sample_form_is_the_wide_form():
    p = _packed(2, 24, 40, seed=9)
    wide, narrow = _arrays(_hist(p, 12)), _arrays(_hist(p, 12, offset=True))
    _same(narrow, wide)
    # ww % 4 != 0 on the same data: the frames cropped to 39 columns hold the whole blocks of the first 32
    q = np.ascontiguousarray(p[:, :, :, :39])
    _same(_hist(q, 12), R.noise_hist_ref(np.ascontiguousarray(p[:, :, :, :32]), 12))


def test_flat_frame_equal_keys_inside_a_wave():
    p, _ = dpc_ref.ingest(R.flat_cells(1, 64, 64, 12, 3200, seed=4), 12)
    want = R.noise_hist_ref(p, 12)
    rows = np.nonzero(want["hist"].sum(axis=1))[0]
    assert want["hist"].sum() == 256 and want["hist"][28].sum() >= 240 and len(rows) <= 3 and (want["hist"] > 1).sum() >= 20
    _same(_hist(p, 12), want)
    # a noise-free flat frame but for one sample per block: every block has the very same key
    cells = np.full((1, 64, 64, 4), 1000.0, F)
    cells[:, 3::8, 3::8] = 1016.0
    p, _ = dpc_ref.ingest(cells, 12)
    want = R.noise_hist_ref(p, 12)
    assert (want["hist"] == 256).sum() == 1 and want["hist"].sum() == 256
    _same(_hist(p, 12), want)


def test_counters_clipped_corner_and_constant_patch():
    p = _packed(2, 32, 48, seed=6, clip=True, patch=True)
    want = R.noise_hist_ref(p, 12)
    seen, clipped, degenerate, _ = want["counters"].tolist()
    assert seen == 2 * 4 * 24 and clipped >= 2 * 4 * 4 and degenerate == 2 * 4 * 4
    _same(_hist(p, 12), want)
    # samples at 0 clip too, and a block with one sample at top
    cells = R.scene_cells(1, 16, 16, 12, 3200, seed=2)
    cells[0, 0, 0, 0] = 0
    cells[0, 15, 15, 3] = 4095
    p, _ = dpc_ref.ingest(cells, 12)
    want = R.noise_hist_ref(p, 12)
    assert want["counters"].tolist()[:3] == [16, 2, 0]
    _same(_hist(p, 12), want)


def test_non_integer_dn_and_a_mean_on_a_bin_edge():
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.9, 0.9, (2, 4, 16, 24)).astype(F)           # packed values of no whole DN at all
    want = R.noise_hist_ref(p, 12)
    assert want["hist"].sum() == 2 * 4 * 6
    _same(_hist(p, 12), want)
    # a block whose mean is exactly 2048 DN, the lower edge of bin 32 at 12 bits: columns alternately 2053 and 2043, whole DN that
    # survive the packed round trip exactly near the middle of the range (asserted, not assumed)
    x = np.full((1, 4, 8, 8), F(2048.0), F)
    x[..., 0::2] += F(5)
    x[..., 1::2] -= F(5)
    p = F(2.0) * (x / F(4095.0)) - F(1.0)
    blocks = R.blocks_of(p, 12)
    m, v = R.block_stats(blocks)
    assert np.array_equal(blocks.reshape(x.shape), x) and (m == F(2048.0)).all() and (v > 0).all()
    want = R.noise_hist_ref(p, 12)
    assert want["hist"][32].sum() == 4 and want["msum"][32] == 4 * 2048 * 16
    _same(_hist(p, 12), want)


@pytest.mark.parametrize("bits", [8, 10, 12, 14, 16])
def test_bit_depths(bits):
    p = _packed(1, 24, 32, bits=bits, iso=12800, seed=bits)
    want = R.noise_hist_ref(p, bits)
    assert want["hist"].sum() >= 40 and len(np.nonzero(want["hist"].sum(axis=1))[0]) >= 8
    _same(_hist(p, bits), want)


def test_two_halves_are_the_whole_and_two_runs_agree():
    p = _packed(4, 24, 40, seed=8, texture=0.3)
    want = R.noise_hist_ref(p, 12)
    whole = _hist(p, 12)
    _same(whole, want)
    halves = _hist(p[2:], 12, _hist(p[:2], 12))
    again = _hist(p, 12)
    assert torch.equal(halves, whole) and torch.equal(again, whole)
    # the reference accumulates the same way
    _same(halves, R.noise_hist_ref(p[2:], 12, R.noise_hist_ref(p[:2], 12)))


# ---- 2. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    rt = _rt()
    p = torch.zeros(1, 4, 16, 16, device="cuda")
    acc = torch.full((32904 + 2,), 7, dtype=torch.int32, device="cuda")
    assert acc.data_ptr() % 8 == 0

    def call(packed=p.data_ptr(), n=1, hh=16, ww=16, bits=12, a=acc.data_ptr()):
        rc = rt.lib.rvdd_noise_hist(rt.h, packed, n, hh, ww, bits, a, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    for kwargs, name in ((dict(a=None), r"\bacc\b"), (dict(a=acc.data_ptr() + 4), "8-byte"), (dict(packed=None), "packed"),
                         (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"), (dict(n=-1), r"\bn\b"), (dict(hh=-8), r"\bhh\b"),
                         (dict(ww=-8), r"\bww\b"), (dict(n=2 ** 31 - 1, hh=2 ** 20, ww=2 ** 20), "workgroups")):
        rc, msg = call(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_noise_hist:") and re.search(name, msg), (kwargs, rc, msg)
    torch.cuda.synchronize()
    assert (acc == 7).all() and (p == 0).all()
    with pytest.raises(RuntimeError, match="131616 bytes"):
        rt.noise_hist(p, 12, acc)
    with pytest.raises(RuntimeError, match=r"\[n,4,hh,ww\]"):
        rt.noise_hist(p[0], 12)


# ---- 3. end to end ----------------------------------------------------------------------------------------------------------
def test_fit_of_a_device_accumulator_is_the_fit_of_the_reference():
    from rvdd_release_amd.runtime import nearest_iso, noise_fit
    p = _packed(4, 64, 96, iso=12800, seed=1)
    want = R.noise_hist_ref(p, 12)
    got = noise_fit(_hist(p, 12), 12)
    assert got == noise_fit(R.acc_bytes(want), 12)
    ref = R.noise_fit_ref(want, 12)
    assert abs(got["a"] - ref["a"]) <= 1e-12 * abs(ref["a"]) and abs(got["b"] - ref["b"]) <= 1e-12 * abs(ref["b"])
    assert nearest_iso(got["a"], got["b"], 12)[0] == 12800
    with pytest.raises(RuntimeError, match=r"\(-2\).*usable mean bins"):
        noise_fit(_hist(_packed(1, 16, 16), 12), 12)


Hc, Wc, T, SEEDS = 96, 128, 5, (0, 32, 20)           # 48 x 64 cells; seeds whose scenes together span 7 mean bins (the synthetic scenes are dark)


def _mosaic(packed_dn):
    """[T,4,h,w] -> [T,2h,2w]: channel k at CFA position (k >> 1, k & 1)"""
    t, _, h, w = packed_dn.shape
    m = np.empty((t, 2 * h, 2 * w), packed_dn.dtype)
    for k in range(4):
        m[:, (k >> 1)::2, (k & 1)::2] = packed_dn[:, k]
    return m


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """<root>/u16 and <root>/mipi: 3 synthetic videos of 5 frames, ISO 12800, 12 bits, as uint16 TIFFs and as MIPI RAW12
    -> (root, the reference's accumulator of the first 4 frames of each)"""
    from rvdd_release_amd import synth, tiffio
    root = tmp_path_factory.mktemp("noise_tree")
    acc = R.new_acc()
    for v, seed in enumerate(SEEDS):
        raw = synth.make_sequence(T, Hc, Wc, iso=12800, seed=seed).raw.numpy()
        dn = np.clip(np.rint((raw.astype(np.float64) + 1.0) * 0.5 * 4095.0), 0, 4095).astype(np.uint16)
        R.noise_hist_ref(dpc_ref.ingest(dn[:4].transpose(0, 2, 3, 1), 12)[0], 12, acc)
        m = _mosaic(dn)
        for folder in ("u16", "mipi"):
            os.makedirs(root / folder / ("%03d" % v))
        for t in range(T):
            tiffio.write(str(root / "u16" / ("%03d/%08d.tif" % (v, t))), m[t])
            bits_ref.pack(m[t], 12, "mipi").tofile(str(root / "mipi" / ("%03d/%08d.raw" % (v, t))))
    return root, acc


def test_noise_command_reads_every_container_the_same(tree, capsys):
    from rvdd_release_amd import noise
    from rvdd_release_amd.runtime import noise_fit
    root, acc = tree
    want = noise_fit(R.acc_bytes(acc), 12)
    lines = []
    for folder, more in (("u16", []), ("mipi", ["--raw_container", "mipi", "--raw_size", "%dx%d" % (Wc, Hc)])):
        capsys.readouterr()
        r = noise.main(["--dataroot", str(root), "--nFolder", folder, "--bit_depth", "12"] + more)
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(line) == 1
        back = json.loads(line[0])
        assert (back["a"], back["b"]) == (want["a"], want["b"]) == (r["a"], r["b"])
        assert (back["bins"], back["blocks"], back["frames"], back["clipped"]) == (want["bins"], want["blocks"], 12, 0)
        assert back["nearest_iso"] in (3200, 12800) and len(back["ratio_20_45_80"]) == 3
        lines.append(line[0])
    assert lines[0] == lines[1]
    r5 = noise.main(["--dataroot", str(root), "--nFolder", "u16", "--bit_depth", "12", "--frames", "5"])
    assert r5["frames"] == 15 and r5["blocks"] > want["blocks"]


def test_denoise_auto_is_denoise_with_the_printed_numbers(tree, tmp_path, capsys, monkeypatch):
    from rvdd_release_amd import denoise, noise
    from rvdd_release_amd.runtime import noise_fit
    root, acc = tree
    want = noise_fit(R.acc_bytes(acc), 12)
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--dataroot", str(root), "--nFolder", "u16"]

    def run(name, *more):
        capsys.readouterr()
        res = str(tmp_path / name)
        stats = denoise.main(flags + ["--results_dir", res] + list(more))
        out = capsys.readouterr().out.splitlines()
        assert stats["frames"] == 3 * (T - 1)
        return _files(res), sorted(ln for ln in out if ln.startswith("dpc:")), [ln[len("noise: "):] for ln in out if ln.startswith("noise: ")]

    typed = None
    for B in (1, 3):
        auto, counts, line = run("auto%d" % B, "--dpc", "4", "--dpc_noise", "auto", "--batch_size", str(B))
        assert len(line) == 1 and len(counts) == 3 and len(auto) == 3 * (T - 1)
        back = json.loads(line[0])
        assert (back["a"], back["b"]) == (want["a"], want["b"])
        ab = re.search(r'"a": (\S+), "b": (\S+),', line[0])
        typed = "%s,%s" % (ab.group(1), ab.group(2))
        same, counts_ab, none = run("ab%d" % B, "--dpc", "4", "--dpc_noise", typed, "--batch_size", str(B))
        assert none == [] and same == auto and counts_ab == counts
    # without auto no estimate is made: none with the numbers typed in, none without --dpc; and a run without --dpc writes what a
    # stage that flags nothing leaves, bit for bit the plain stream (tests/test_gpu_dpc.py)
    monkeypatch.setattr(noise, "estimate", lambda *a, **k: pytest.fail("an estimate without --dpc_noise auto"))
    plain, counts, line = run("plain", "--batch_size", "3")
    assert counts == [] and line == []
    inert, counts, line = run("inert", "--dpc", "1e18", "--dpc_noise", typed, "--batch_size", "3")
    assert inert == plain and line == [] and all(ln.startswith("dpc: 0 hot, 0 dead") for ln in counts)
    assert sorted(plain) == sorted(auto)


def test_denoise_auto_refuses_with_the_fits_message(tmp_path):
    from rvdd_release_amd import denoise, tiffio
    os.makedirs(tmp_path / "flat" / "000")
    cells = R.flat_cells(3, 16, 16, 12, 3200, seed=1)
    m = _mosaic(cells.transpose(0, 3, 1, 2).astype(np.uint16))
    for t in range(3):
        tiffio.write(str(tmp_path / "flat" / "000" / ("%08d.tif" % t)), m[t])
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, "recurrent-convunet+feat-iso3200"),
             "--feature_rec", "--bit_depth", "12", "--dataroot", str(tmp_path), "--nFolder", "flat", "--results_dir", str(tmp_path / "res")]
    with pytest.raises(SystemExit, match=r"--dpc_noise auto: .*usable mean bins.*--dpc_noise a,b"):
        denoise.main(flags + ["--dpc", "4", "--dpc_noise", "auto"])
    assert not os.path.exists(tmp_path / "res")
