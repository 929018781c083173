"""Scene cuts on the device: every integer of rvdd_frame_sigs against the NumPy restatement (tests/cuts_ref.py), the argument errors,
and `denoise --cuts` against the same frames laid out as one folder per shot.  Every comparison is exact."""
import json
import os
import re

import numpy as np
import pytest
import torch

import bits_ref
import cuts_ref as R
import dpc_ref
from conftest import WEIGHTS
from gpu_support import ops_rt as _rt, upload

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = ("integer", "fractions", "outside", "flat")


def _frames(hh, ww, bits, seed):
    """[4,hh,ww] f32, one frame per kind: whole DN over the range; DN with quarter and eighth fractions (c * 4 lands on .0 and .5: the
    ties of rintf); values below 0 and above top mixed into whole DN; a perfectly flat frame"""
    rng = np.random.default_rng(seed)
    top = 2 ** bits - 1
    whole = rng.integers(0, top + 1, (hh, ww)).astype(F)
    frac = np.minimum(rng.integers(0, top, (hh, ww)).astype(F) + rng.integers(0, 8, (hh, ww)).astype(F) * F(0.125), F(top))
    out = whole.copy()
    where = rng.random((hh, ww))
    out[where < 0.2] = -rng.uniform(0.25, 3.0 * top, int((where < 0.2).sum())).astype(F)
    out[where > 0.8] = (top + rng.uniform(0.125, 3.0 * top, int((where > 0.8).sum()))).astype(F)
    flat = np.full((hh, ww), F(int(0.45 * top)), F)
    return np.stack([whole, frac, out, flat])


def _sigs(gray, bits, offset=False, out=None):
    g = upload(gray, offset=offset)
    assert g.data_ptr() % 16 == (4 if offset else 0)
    sig = _rt().frame_sigs(g, bits, out)
    torch.cuda.synchronize()
    assert np.array_equal(g.cpu().numpy().view(np.uint32), np.ascontiguousarray(gray).view(np.uint32))      # the input is not touched
    return sig


def _same(sig, gray, bits, what=""):
    """every byte of the device's signatures against the reference's"""
    from rvdd_release_amd.runtime import frame_sig_arrays
    want = R.frame_sig_ref(gray, bits)
    got = frame_sig_arrays(sig)
    for k in ("hist", "sum"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())
    assert sig.cpu().numpy().tobytes() == R.sig_bytes(want), what


# ---- 1. the signatures --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 12, 16])
@pytest.mark.parametrize("hh,ww", [(16, 16), (17, 19), (16, 20), (37, 52), (45, 80)])
def test_signature_is_the_restatement(hh, ww, bits):
    """16 x 16: one row per band, one cell per block; 17 x 19: uneven bands, odd ww, the single-float form; 16 x 20: the wide form with
    block columns that change inside a lane's four cells (ww / 16 = 1.25); 37 x 52: bands of two and three rows; 45 x 80: n = 3, the
    last frame checked like the first.  Every kind of input alone, and the wide shapes again from a pointer one float off (the
    single-float form: same integers)."""
    frames = _frames(hh, ww, bits, seed=hh * 100 + bits)
    for k, kind in enumerate(KINDS):
        _same(_sigs(frames[k:k + 1], bits), frames[k:k + 1], bits, kind)
    if ww % 4 == 0:
        _same(_sigs(frames, bits, offset=True), frames, bits, "offset by 4 bytes")
    if (hh, ww) == (45, 80):
        sig = _sigs(frames[:3], bits)
        _same(sig, frames[:3], bits, "n = 3")
        assert sig[2].cpu().numpy().tobytes() == R.sig_bytes(R.frame_sig_ref(frames[2:3], bits))


def test_a_band_of_more_than_one_chunk():
    """a band of 524 293 cells in the single-float form is 2049 iterations: two chunks, the LDS words folded and cleared in between;
    all but a hundredth of the cells are one value, so a lane counts every one of its 2049 cells into one 16-bit half"""
    rng = np.random.default_rng(5)
    g = np.full((1, 16, 524293), F(1000.0), F)
    spots = rng.random(g.shape) < 0.01
    g[spots] = rng.integers(0, 4096, int(spots.sum())).astype(F)
    _same(_sigs(g, 12), g, 12)


def test_batch_is_its_frames_and_two_runs_agree():
    for hh, ww in ((37, 52), (45, 80), (33, 47)):
        frames = _frames(hh, ww, 12, seed=hh)
        whole = _sigs(frames, 12)
        again = _sigs(frames, 12)
        assert torch.equal(whole, again)
        for k in range(4):
            assert torch.equal(_sigs(frames[k:k + 1], 12)[0], whole[k]), (hh, ww, k)
        _same(whole, frames, 12)


def test_buffer_is_overwritten_and_nothing_beyond_it():
    rt = _rt()
    frames = _frames(37, 52, 12, seed=3)[:3]
    g = torch.from_numpy(frames).cuda()
    buf = torch.full((4, 6144), 0xFF, dtype=torch.uint8, device="cuda")
    assert rt.lib.rvdd_frame_sigs(rt.h, g.data_ptr(), 3, 37, 52, 12, buf.data_ptr(), None) == 0
    torch.cuda.synchronize()
    _same(buf[:3], frames, 12, "pre-filled with 0xFF")
    assert (buf[3] == 0xFF).all()
    # out= of the Python call is that buffer's shape, checked
    assert rt.frame_sigs(g, 12, buf[:3]).data_ptr() == buf.data_ptr()
    with pytest.raises(RuntimeError, match=r"uint8 tensor \[3,6144\]"):
        rt.frame_sigs(g, 12, buf)
    with pytest.raises(RuntimeError, match=r"\[n,hh,ww\]"):
        rt.frame_sigs(g[0], 12)


def test_argument_errors_launch_nothing():
    rt = _rt()
    g = torch.zeros(1, 16, 16, device="cuda")
    buf = torch.full((6144 + 8,), 7, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 8 == 0

    def call(gray=g.data_ptr(), n=1, hh=16, ww=16, bits=12, sig=buf.data_ptr()):
        rc = rt.lib.rvdd_frame_sigs(rt.h, gray, n, hh, ww, bits, sig, None)
        return rc, rt.lib.rvdd_last_error(rt.h).decode()

    for kwargs, name in ((dict(gray=None), r"\bgray\b"), (dict(sig=None), r"\bsig\b"), (dict(sig=buf.data_ptr() + 4), "8-byte"),
                         (dict(hh=15), r"\bhh\b"), (dict(ww=15), r"\bww\b"), (dict(bits=0), "bit_depth"), (dict(bits=17), "bit_depth"),
                         (dict(n=-1), r"\bn\b"), (dict(n=2 ** 27), "blocks")):
        rc, msg = call(**kwargs)
        assert rc == -1 and msg.startswith("rvdd_frame_sigs:") and re.search(name, msg), (kwargs, rc, msg)
    # n = 0 does nothing, whatever the pointers
    assert call(n=0, gray=None, sig=None)[0] == 0
    torch.cuda.synchronize()
    assert (buf == 7).all() and (g == 0).all()


def test_score_of_device_signatures_is_the_reference_score():
    from rvdd_release_amd.runtime import cut_score
    gray = np.concatenate([R.scene_gray(1, 2, 48, 64, 12800, 8.0), R.scene_gray(2, 1, 48, 64, 12800, 8.0)])
    sig = _sigs(gray, 12)
    want = R.scores_ref(R.frame_sig_ref(gray, 12), 48, 64)
    assert [cut_score(sig[k - 1], sig[k], 48, 64) for k in (1, 2)] == want
    with pytest.raises(RuntimeError, match="another frame size"):
        cut_score(sig[0], sig[1], 48, 65)


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------
Hc, Wc, T = 96, 128, 5                     # pixels: 48 x 64 cells, the frame size of the other denoise tests
FEAT = {0: "recurrent-convunet+feat-iso3200", 1: "recurrent-convunet+feat-future-iso12800"}


def _mosaic(cells):
    """[T,h,w,4] -> [T,2h,2w] uint16: channel k at CFA position (k >> 1, k & 1)"""
    t, h, w, _ = cells.shape
    m = np.empty((t, 2 * h, 2 * w), np.uint16)
    for k in range(4):
        m[:, (k >> 1)::2, (k & 1)::2] = cells[..., k]
    return m


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """Two shots of 5 frames without motion, a dark flat-ish one and a bright one (a level, a gentle ramp, the ISO 3200 noise), as
      X/000/00000000 .. 00000009.tif    one folder          X_mipi: the same as MIPI RAW12
      Y/000/00000000 .. 4, Y/001/00000005 .. 9              one folder per shot
    The reference rule finds exactly frame 5 at the defaults: checked here, on the CPU.  -> (root, the line the cuts command prints)"""
    from rvdd_release_amd import cuts, tiffio
    root = tmp_path_factory.mktemp("cuts_tree")
    cells = np.concatenate([dpc_ref.noisy_cells(T, Hc // 2, Wc // 2, 12, 3200, seed=1, level=0.15),
                            dpc_ref.noisy_cells(T, Hc // 2, Wc // 2, 12, 3200, seed=2, level=0.60)])
    scores = R.scores_ref(R.frame_sig_ref(dpc_ref.ingest(cells, 12)[1], 12), Hc // 2, Wc // 2)
    assert R.find_cuts_ref(scores) == [5] and cuts.find_cuts(scores) == [5]
    assert max(max(s) for k, s in enumerate(scores) if k != 4) < 0.08 and scores[4][0] > 0.9
    m = _mosaic(cells)
    for d in ("X/000", "X_mipi/000", "Y/000", "Y/001"):
        os.makedirs(root / d)
    for t in range(2 * T):
        tiffio.write(str(root / "X" / "000" / ("%08d.tif" % t)), m[t])
        tiffio.write(str(root / "Y" / ("%03d" % (t // T)) / ("%08d.tif" % t)), m[t])
        bits_ref.pack(m[t], 12, "mipi").tofile(str(root / "X_mipi" / "000" / ("%08d.raw" % t)))
    return root, cuts.format_line("000", 2 * T, [5]), scores


def _by_name(res):
    """results tree -> {file name: bytes}; the frames' names are unique over the folders"""
    out = {}
    for d, _, names in os.walk(res):
        for name in names:
            assert name not in out
            with open(os.path.join(d, name), "rb") as f:
                out[name] = f.read()
    return out


def _run(capsys, tmp_path, root, name, folder, future, *more):
    from rvdd_release_amd import denoise
    flags = ["--netDenoiser", "convunet-mode=fixedfeatures+feat", "--path2epoch", os.path.join(WEIGHTS, FEAT[future]), "--feature_rec",
             "--future_patch_depth", str(future), "--bit_depth", "12", "--dataroot", str(root), "--nFolder", folder]
    capsys.readouterr()
    res = str(tmp_path / name)
    stats = denoise.main(flags + ["--results_dir", res] + list(more))
    log = capsys.readouterr().out.splitlines()
    files = _by_name(res)
    assert stats["frames"] == len(files)
    return files, [ln for ln in log if ln.startswith("cuts:") and "shots at" in ln], [ln for ln in log if ln.startswith("dpc:")]


@pytest.mark.parametrize("all_frames", [False, True])
@pytest.mark.parametrize("future", [0, 1])
def test_denoise_cuts_auto_is_one_folder_per_shot(trees, tmp_path, capsys, future, all_frames):
    root, _, _ = trees
    more = ["--all_frames"] if all_frames else []
    want, none, _ = _run(capsys, tmp_path, root, "y", "Y", future, "--batch_size", "2", *more)
    names = ["%08d_denoised.tif" % t for t in range(2 * T) if all_frames or 1 <= t % T < T - future]
    assert none == [] and sorted(want) == names                      # per SHOT: without --all_frames its first and last `future` frames are not written
    for B in (1, 2):
        got, lines, _ = _run(capsys, tmp_path, root, "x%d" % B, "X", future, "--cuts", "auto", "--batch_size", str(B), *more)
        assert lines == ["cuts: 000: 10 frames, shots at [0, 5]"]
        assert sorted(got) == names and all(got[k] == want[k] for k in names), (B, [k for k in names if got[k] != want[k]])


def test_denoise_cuts_file_no_cuts_and_the_dpc_lines(trees, tmp_path, capsys, monkeypatch):
    from rvdd_release_amd import cuts
    root, line, _ = trees
    auto, _, _ = _run(capsys, tmp_path, root, "auto", "X", 0, "--cuts", "auto", "--batch_size", "2", "--all_frames")
    # no pass from here on: --cuts FILE reads what the command printed, a run without the flag calls nothing new
    monkeypatch.setattr(cuts, "detect", lambda *a, **k: pytest.fail("a pass over the frames without --cuts auto"))
    listed = str(tmp_path / "cuts.txt")
    with open(listed, "w") as f:
        f.write("1 videos\n" + line + "\n")
    filed, lines, dpc = _run(capsys, tmp_path, root, "file", "X", 0, "--cuts", listed, "--batch_size", "2", "--all_frames", "--dpc", "4", "--dpc_iso", "3200")
    assert lines == ["cuts: 000: 10 frames, shots at [0, 5]"]
    # a correction that flags nothing on defect-free noise would be luck; the lines are per shot and name its first frame
    assert len(dpc) == 2 and sorted(re.search(r"in 5 frames \((.*)\)$", ln).group(1) for ln in dpc) == ["000 from 00000000.tif", "000 from 00000005.tif"]
    plain_file, _, _ = _run(capsys, tmp_path, root, "file_plain", "X", 0, "--cuts", listed, "--batch_size", "2", "--all_frames")
    assert plain_file == auto
    # without --cuts: the run of before, through the untouched path and through the path of a list without cuts -- the same bytes
    with open(listed, "w") as f:
        f.write(cuts.format_line("000", 2 * T, []) + "\n")
    plain, none, _ = _run(capsys, tmp_path, root, "plain", "X", 0, "--batch_size", "2", "--all_frames")
    uncut, lines, _ = _run(capsys, tmp_path, root, "uncut", "X", 0, "--cuts", listed, "--batch_size", "2", "--all_frames")
    assert none == [] and lines == ["cuts: 000: 10 frames, shots at [0]"] and uncut == plain and sorted(plain) == sorted(auto)
    # ... and the cut is not for nothing: up to it the two runs agree, from it on the uncut run carries the first shot along
    differ = sorted(k for k in plain if plain[k] != auto[k])
    assert "%08d_denoised.tif" % 5 in differ and all(int(k[:8]) >= 5 for k in differ), differ
    for bad, what in (('{"video": "007", "frames": 10, "cuts": [5]}', "video '007' is not in this run"),
                      ('{"video": "000", "frames": 10, "cuts": [10]}', r"cut 10 is outside 1 \.\. 9")):
        with open(listed, "w") as f:
            f.write(bad + "\n")
        with pytest.raises(SystemExit, match=what):
            _run(capsys, tmp_path, root, "bad", "X", 0, "--cuts", listed)
    assert not os.path.exists(tmp_path / "bad")


def test_cuts_command_reads_every_container_the_same(trees, capsys):
    from rvdd_release_amd import cuts
    root, line, scores = trees
    printed = []
    for folder, more in (("X", []), ("X_mipi", ["--raw_container", "mipi", "--raw_size", "%dx%d" % (Wc, Hc)])):
        capsys.readouterr()
        found = cuts.main(["--dataroot", str(root), "--nFolder", folder, "--bit_depth", "12", "--scores"] + more)
        out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        assert len(out) == 1 and found[0]["cuts"] == [5] and found[0]["scores"] == scores      # the device's integers: the reference's scores, to the bit
        back = json.loads(out[0])
        assert back["video"] == "000" and back["frames"] == 10 and back["cuts"] == [5] and [tuple(s) for s in back["scores"]] == scores
        printed.append(out[0])
    assert printed[0] == printed[1] and printed[0].startswith(line[:-1])
    # two folders, no cut in either; a longer least shot drops the cut
    capsys.readouterr()
    found = cuts.main(["--dataroot", str(root), "--nFolder", "Y", "--bit_depth", "12"])
    assert capsys.readouterr().out.splitlines()[-2:] == ['{"video": "000", "frames": 5, "cuts": []}', '{"video": "001", "frames": 5, "cuts": []}']
    assert cuts.main(["--dataroot", str(root), "--nFolder", "X", "--bit_depth", "12", "--cut_min_len", "6"])[0]["cuts"] == []
