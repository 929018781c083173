"""Scene cuts without a GPU: rvdd_cut_score through ctypes against the score on Python integers (tests/cuts_ref.py), its refusals,
`find_cuts`, the rule itself on synthetic shots of known cuts, the arguments of the denoise command line and the shots it hands to
`deal_slots`, and header, binding and struct."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import cuts_ref as R


def _random_sig(rng, hh, ww, scale=1.0):
    """one signature of consistent totals: hh * ww cells dealt to the bands as the rule deals rows, to level bins at random"""
    rows = np.bincount((16 * np.arange(hh)) // hh, minlength=16)
    hist = np.stack([rng.multinomial(int(r) * ww, rng.dirichlet(np.ones(64) * 0.3)) for r in rows])
    total = (rng.integers(0, 4 * 4095, (16, 16)) * scale * (hh * ww // 256)).astype(np.uint64)
    return {"hist": hist[None].astype(np.uint32), "sum": total[None]}


# ---- rvdd_cut_score ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hh,ww", [(16, 16), (37, 52), (360, 640), (1080, 1920)])
def test_c_score_is_the_integer_score(hh, ww):
    from rvdd_release_amd.runtime import cut_score, frame_sig_arrays
    rng = np.random.default_rng(hh)
    for trial in range(8):
        a, b = _random_sig(rng, hh, ww), _random_sig(rng, hh, ww, scale=rng.uniform(0.2, 1.5))
        want = R.cut_score_ref(a["hist"][0], a["sum"][0], b["hist"][0], b["sum"][0], hh, ww)
        got = cut_score(R.sig_bytes(a), R.sig_bytes(b), hh, ww)
        assert got == want and 0 < got[0] <= 1 and 0 < got[1] <= 1, (trial, got, want)      # equal, not close
        back = frame_sig_arrays(R.sig_bytes(a) + R.sig_bytes(b))
        assert np.array_equal(back["hist"][0], a["hist"][0]) and np.array_equal(back["sum"][1], b["sum"][0])
    assert cut_score(R.sig_bytes(a), R.sig_bytes(a), hh, ww) == (0.0, 0.0)
    # disjoint level bins, disjoint blocks: both distances are exactly 1
    x = {"hist": np.zeros((1, 16, 64), np.uint32), "sum": np.zeros((1, 16, 16), np.uint64)}
    y = {"hist": np.zeros((1, 16, 64), np.uint32), "sum": np.zeros((1, 16, 16), np.uint64)}
    x["hist"][0, 0, 3] = y["hist"][0, 5, 60] = hh * ww
    x["sum"][0, 2, 2] = 1000
    y["sum"][0, 9, 1] = 77
    assert cut_score(R.sig_bytes(x), R.sig_bytes(y), hh, ww) == (1.0, 1.0) == R.cut_score_ref(x["hist"][0], x["sum"][0], y["hist"][0], y["sum"][0], hh, ww)
    # all sums zero (a black frame): the denominator is 1, not 0
    x["sum"][:] = y["sum"][:] = 0
    assert cut_score(R.sig_bytes(x), R.sig_bytes(y), hh, ww) == (1.0, 0.0)


def test_score_refusals_name_the_argument():
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import cut_score
    lib = _lib.load()
    rng = np.random.default_rng(1)
    a, b = _random_sig(rng, 24, 40), _random_sig(rng, 24, 40)
    sa, sb = (_lib.RvddFrameSig.from_buffer_copy(R.sig_bytes(s)) for s in (a, b))
    out = (C.c_double * 2)(-7.0, -7.0)
    assert lib.rvdd_cut_score(C.byref(sa), C.byref(sb), 24, 40, out) == 0 and out[0] >= 0
    out[0] = out[1] = -7.0
    for args, word in (((None, C.byref(sb), 24, 40, out), rb"\ba is required"), ((C.byref(sa), None, 24, 40, out), rb"\bb is required"),
                       ((C.byref(sa), C.byref(sb), 24, 40, None), rb"out2"), ((C.byref(sa), C.byref(sb), 15, 64, out), rb"\bhh\b"),
                       ((C.byref(sa), C.byref(sb), 60, 15, out), rb"\bww\b"),
                       ((C.byref(sa), C.byref(sb), 24, 41, out), rb"a counts 960 cells.*another frame size")):
        assert lib.rvdd_cut_score(*args) == -1, word
        msg = lib.rvdd_last_error(None)
        assert msg.startswith(b"rvdd_cut_score:") and re.search(word, msg), (word, msg)
    # only b of another size
    big = _lib.RvddFrameSig.from_buffer_copy(R.sig_bytes(_random_sig(rng, 24, 44)))
    assert lib.rvdd_cut_score(C.byref(sa), C.byref(big), 24, 40, out) == -1 and re.search(rb"b counts 1056 cells", lib.rvdd_last_error(None))
    assert (out[0], out[1]) == (-7.0, -7.0)                      # refused: *out2 untouched
    with pytest.raises(RuntimeError, match=r"\(-1\).*another frame size"):
        cut_score(R.sig_bytes(a), R.sig_bytes(b), 25, 40)
    with pytest.raises(RuntimeError, match="6144 bytes"):
        cut_score(b"\0" * 100, R.sig_bytes(b), 24, 40)
    with pytest.raises(RuntimeError, match="ONE signature"):
        cut_score(R.sig_bytes(a) + R.sig_bytes(b), R.sig_bytes(b), 24, 40)
    with pytest.raises(ValueError, match="another frame size"):
        R.cut_score_ref(a["hist"][0], a["sum"][0], b["hist"][0], b["sum"][0], 25, 40)


# ---- the reference rule by hand ---------------------------------------------------------------------------------------------
def test_rule_by_hand():
    g = np.zeros((1, 16, 16), R.F)
    g[0, 0, 0], g[0, 0, 1], g[0, 1, 0], g[0, 15, 15], g[0, 2, 2], g[0, 3, 3], g[0, 4, 4] = 100.25, 100.125, 100.375, 5000.0, -3.0, 4095.0, 63.99
    s = R.frame_sig_ref(g, 12)
    # 100.25 * 4 = 401; 100.125 * 4 = 400.5 -> 400 and 100.375 * 4 = 401.5 -> 402 (ties to even); above top -> 4 * 4095; below 0 -> 0
    assert [int(s["sum"][0][b]) for b in ((0, 0), (0, 1), (1, 0), (15, 15), (2, 2), (3, 3), (4, 4))] == [401, 400, 402, 16380, 0, 16380, 256]
    assert s["hist"][0, 0, 1] == 2 and s["hist"][0, 0, 0] == 14 and s["hist"][0, 1, 1] == 1 and s["hist"][0, 15, 63] == 1 and s["hist"][0, 3, 63] == 1
    assert s["hist"][0, 4, 0] == 16 and s["hist"].sum() == 256                    # 63.99 DN lies in bin 0 at 12 bits, 64 would lie in bin 1
    # uneven bands and columns: 17 rows -> band 0 has two rows (16 y / 17 = 0 for y = 0, 1), 19 columns -> columns 0, 5 and 10 have two
    s = R.frame_sig_ref(np.full((1, 17, 19), 10.0, R.F), 8)
    assert s["hist"][0, :, 2].tolist() == [38] + [19] * 15 and s["sum"][0, 1].tolist() == [40 * (2 if b in (0, 5, 10) else 1) for b in range(16)]
    assert len(R.sig_bytes(s)) == R.SIG_BYTES == 6144


# ---- find_cuts --------------------------------------------------------------------------------------------------------------
def test_find_cuts_edge_cases():
    from rvdd_release_amd.cuts import find_cuts
    lo, hi_h, hi_g = (0.01, 0.01), (0.5, 0.0), (0.0, 0.5)
    assert find_cuts([]) == [] and find_cuts([hi_h]) == [] and find_cuts([lo] * 20) == []
    scores = [lo] * 19
    scores[7] = hi_h                                   # the pair (7, 8): frame 8 starts a shot
    assert find_cuts(scores) == [8]
    scores[8] = hi_g                                   # frame 9 too: adjacent, the second is dropped
    assert find_cuts(scores) == [8]
    scores[11] = hi_g                                  # frame 12: exactly min_len behind
    assert find_cuts(scores) == [8, 12] and find_cuts(scores, min_len=5) == [8]
    assert find_cuts(scores, min_len=1) == [8, 9, 12]
    scores[16] = hi_h                                  # frame 17 of 20: three frames before the end -> dropped; 16 would stay
    assert find_cuts(scores) == [8, 12]
    scores[15] = hi_h
    assert find_cuts(scores) == [8, 12, 16]
    scores[2] = hi_h                                   # frame 3: too close to frame 0
    assert find_cuts(scores) == [8, 12, 16] and find_cuts(scores, min_len=3)[:1] == [3]
    # strictly greater: a score on the threshold is no cut; either score alone suffices
    assert find_cuts([lo] * 5 + [(0.10, 0.12)] + [lo] * 5) == [] and find_cuts([lo] * 5 + [(0.1000001, 0.0)] + [lo] * 5) == [6]
    assert find_cuts([lo] * 5 + [(0.0, 0.2)] + [lo] * 5, t_grid=0.25) == []
    rng = np.random.default_rng(3)
    for _ in range(50):
        s = [tuple(v) for v in rng.uniform(0, 0.2, (int(rng.integers(0, 30)), 2))]
        m = int(rng.integers(1, 6))
        assert find_cuts(s, min_len=m) == R.find_cuts_ref(s, min_len=m)


# ---- the rule on synthetic shots ----------------------------------------------------------------------------------------------
def test_detection_on_the_recipes_scenes():
    """128 x 192 cells, ISO 12800, 8 cells per frame, 12 seeds of 5 frames, the reference rule alone: no pair inside a shot is flagged
    at the defaults, and at most 2 % of the 132 ordered cuts (the last frame of one shot against the first of another) are missed."""
    seeds = range(12)
    sigs = [R.frame_sig_ref(R.scene_gray(seed, 5, 128, 192, 12800, 8.0), 12) for seed in seeds]
    inside = [s for sig in sigs for s in R.scores_ref(sig, 128, 192)]
    assert len(inside) == 48
    print("inside a shot: largest d_hist %.4f, largest d_grid %.4f" % (max(h for h, _ in inside), max(g for _, g in inside)))
    assert not [s for s in inside if s[0] > R.T_HIST or s[1] > R.T_GRID]
    across = [R.cut_score_ref(a["hist"][4], a["sum"][4], b["hist"][0], b["sum"][0], 128, 192) for i, a in enumerate(sigs) for j, b in enumerate(sigs) if i != j]
    missed = [s for s in across if not (s[0] > R.T_HIST or s[1] > R.T_GRID)]
    print("across a cut: median d_hist %.3f, median d_grid %.3f, missed %d of %d" % (np.median([h for h, _ in across]), np.median([g for _, g in across]),
                                                                                   len(missed), len(across)))
    assert len(across) == 132 and len(missed) <= 0.02 * len(across), missed
    # a reel of three of the shots: the cuts are found where they are
    reel = {k: np.concatenate([sigs[i][k] for i in (0, 1, 2)]) for k in ("hist", "sum")}
    assert R.find_cuts_ref(R.scores_ref(reel, 128, 192)) == [5, 10]


# ---- denoise ------------------------------------------------------------------------------------------------------------------
def test_denoise_cuts_arguments():
    from rvdd_release_amd import cuts, denoise
    assert "--cuts auto" in denoise.__doc__ and "--all_frames with --cuts" in denoise.__doc__ and "real footage" in denoise.__doc__
    assert "real footage" in cuts.__doc__
    assert denoise._parse([]).cuts is None
    assert denoise._parse(["--cuts", "auto"]).cuts == ("auto", 0.10, 0.12, 4)
    assert denoise._parse(["--cuts", "auto", "--cut_hist", "0.2", "--cut_grid", "0.3", "--cut_min_len", "9"]).cuts == ("auto", 0.2, 0.3, 9)
    assert denoise._parse(["--cuts", "auto", "--cut_min_len", "2"]).cuts[3] == 2
    assert denoise._parse(["--cuts", "auto", "--cut_min_len", "3", "--future_patch_depth", "1"]).cuts[3] == 3
    assert denoise._parse(["--cuts", "some/file.txt"]).cuts == ("file", "some/file.txt")
    for bad, what in ((["--cut_hist", "0.2"], "belong to --cuts auto"), (["--cut_min_len", "5"], "belong to --cuts auto"),
                      (["--cuts", "f.txt", "--cut_grid", "0.2"], "--cut_grid belongs to --cuts auto"),
                      (["--cuts", "auto", "--cut_min_len", "1"], "--cut_min_len must be at least 2"),
                      (["--cuts", "auto", "--cut_min_len", "2", "--future_patch_depth", "1"], "--cut_min_len must be at least 3"),
                      (["--cuts", "auto", "--cut_hist", "-1"], "thresholds >= 0")):
        with pytest.raises(SystemExit, match=what):
            denoise._parse(bad)


def test_cuts_file_and_the_shots_handed_to_deal_slots(tmp_path):
    from rvdd_release_amd import cuts, denoise
    videos = [("a", ["a/%02d.tif" % k for k in range(10)]), ("sub/b", ["b/%02d.tif" % k for k in range(6)]), ("c", ["c/0.tif", "c/1.tif"])]
    path = str(tmp_path / "cuts.txt")
    scores = [(0.1 * k, 1.0 / 3.0) for k in range(9)]
    with open(path, "w") as f:
        f.write("3 videos\n" + cuts.format_line("a", 10, [4, 8], scores) + "\n(some other line of a log)\n" + cuts.format_line("sub/b", 6, []) + "\n")
    lines = open(path).read().splitlines()
    assert json.loads(lines[1]) == {"video": "a", "frames": 10, "cuts": [4, 8], "scores": [list(s) for s in scores]}      # %.17g reads back exactly
    assert lines[3] == '{"video": "sub/b", "frames": 6, "cuts": []}'
    by_key = denoise.read_cuts_file(path)
    assert by_key == {"a": [4, 8], "sub/b": []}
    shots = denoise.split_shots(videos, by_key)
    assert [(k, f[0], len(f)) for k, f in shots] == [("a", "a/00.tif", 4), ("a", "a/04.tif", 4), ("a", "a/08.tif", 2), ("sub/b", "b/00.tif", 6), ("c", "c/0.tif", 2)]
    assert [p for _, f in shots for p in f] == [p for _, f in videos for p in f]                     # every frame once, in order
    # what deal_slots makes of them on two slots: FIRST at every shot's first frame, and a shot's frames count from 0
    steps = denoise.deal_slots([len(f) for _, f in shots], 2)
    firsts = sorted((v, k) for step in steps for c, v, k in step if c == denoise.FIRST)
    assert firsts == [(v, 0) for v in range(5)]
    assert sum(1 for step in steps for c, v, k in step if c != denoise.IDLE) == 18
    # no cuts at all: the videos themselves
    assert denoise.split_shots(videos, {}) == videos
    for bad, what in (({"zz": [3]}, r"video 'zz' is not in this run"), ({"a": [0]}, r"video 'a': cut 0 is outside 1 \.\. 9"),
                      ({"a": [4, 10]}, r"video 'a': cut 10 is outside 1 \.\. 9"), ({"c": [2]}, r"video 'c': cut 2 is outside 1 \.\. 1")):
        with pytest.raises(SystemExit, match=what):
            denoise.split_shots(videos, bad)
    with pytest.raises(SystemExit, match=r"--cuts .*nothing_here"):
        denoise.read_cuts_file(str(tmp_path / "nothing_here"))
    for text, what in (('{"video": "a", "cuts": [1.5]}', "line 1"), ('{"video": "a"}', "line 1"), ('{"video": "a", "cuts": [2]}\n{"video": "a", "cuts": [3]}', "appears twice"),
                       ('{"video": 3, "cuts": []}', "line 1"), ('{"video": "a", "cuts": [2]', "line 1")):
        with open(path, "w") as f:
            f.write(text + "\n")
        with pytest.raises(SystemExit, match=what):
            denoise.read_cuts_file(path)


# ---- header, binding, struct ----------------------------------------------------------------------------------------------------
def test_header_binding_and_struct_agree():
    from conftest import REPO
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import FRAME_SIG_BYTES
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rvdd.h")).read(), flags=re.S)
    for fn in ("rvdd_frame_sigs", "rvdd_cut_score"):
        assert re.search(r"\bint %s\(" % fn, txt) and fn in _lib.exported_symbols()
    assert re.search(r"typedef struct rvdd_frame_sig \{\s*uint32_t hist\[16\]\[64\];\s*uint64_t sum\[16\]\[16\];\s*\} rvdd_frame_sig;", txt)
    assert [f for f, _ in _lib.RvddFrameSig._fields_] == ["hist", "sum"] and C.sizeof(_lib.RvddFrameSig) == FRAME_SIG_BYTES == 6144
    lib = _lib.load()
    assert hasattr(lib, "rvdd_frame_sigs") and hasattr(lib, "rvdd_cut_score")
    mk = open(os.path.join(REPO, "rvdd-release_amd", "csrc", "Makefile")).read()
    assert re.search(r"^KERNELS = .*\bcuts\b", mk, flags=re.M) and re.search(r"^FLAGS_cuts = -ffp-contract=off$", mk, flags=re.M)
