"""`denoise --col_noise` and `python -m rvdd_release_amd.col_noise` without a device: the flags and every refusal, the pre-pass over a
recorded estimate, the calls of a run over a recording runtime with and without the flag, and the `cols:` line."""
import json
import re
import types

import numpy as np
import pytest
import torch

import cols_ref as R

ISO3200 = (8.0034, 2043.51144)
H = W = 32
TOP = 4095.0 / 64.0


class RecordingRuntime:
    """What denoise.run_group drives, recording every call and its arguments"""

    def __init__(self, B):
        self.B, self.calls, self.args = B, [], {}
        self.count = [0] * B

    def __getattr__(self, name):
        if name.startswith(("set_", "dpc_counts")):
            def call(*a, **k):
                self.calls.append(name)
                self.args.setdefault(name, []).append(a)
                return [(0, 0)] * self.B
            return call
        raise AttributeError(name)

    def video_push(self, frames, ctl, bit_depth, layout, out=None, container=None):
        self.calls.append("video_push")
        valid = []
        for b, c in enumerate(ctl):
            self.count[b] = 0 if c == 2 else 1 if c == 1 else self.count[b] + 1
            valid.append(self.count[b] >= 2)
        return torch.zeros(self.B, 3, H, W), valid

    def egress(self, rgb, layout, sample, depth, out=None):
        self.calls.append("egress")
        return torch.zeros(self.B, H, W, 3)


class Dataset:
    container, layout, dtype = None, "mosaic", np.uint16

    def __init__(self, lengths):
        self.videos = [("%03d" % v, ["%03d/%08d.tif" % (v, t) for t in range(n)]) for v, n in enumerate(lengths)]

    def read_frame(self, path):
        return np.zeros((H, W), np.uint16)

    def frame_size(self, path):
        return H, W


def _run(monkeypatch, flags, cmap, lengths=(4, 3, 5), B=2):
    from rvdd_release_amd import denoise
    opt = denoise._parse(["--batch_size", str(B)] + flags)
    opt.cols_map = cmap                                              # what prepasses leaves
    rt = RecordingRuntime(B)
    model = types.SimpleNamespace(device=torch.device("cpu"), training_unrollings=2,
                                  _netDenoise=types.SimpleNamespace(runtime_for=lambda B, H, W, pin=True: rt))
    monkeypatch.setattr(denoise, "write_frame", lambda *a, **k: None)
    data = Dataset(lengths)
    return rt, denoise.run_group(opt, model, data, data.videos, H, W, None, None)


def test_flags_and_every_refusal():
    from rvdd_release_amd import denoise
    with pytest.raises(SystemExit, match=r"--col_noise auto needs the sensor's noise curve.*--col_noise_curve a,b\[,floor\].*auto.*iso3200 / iso12800.*--dpc"):
        denoise._parse(["--col_noise", "auto"])
    curve = ["--col_noise_curve", "8,2000"]
    auto = ["--col_noise", "auto"]
    for bad, word in ((curve, "belong to --col_noise auto"), (["--col_noise_frames", "4"], "belong to --col_noise auto"),
                      (["--col_noise_gate", "3"], "belong to --col_noise auto"), (["--col_noise_sigma", "3"], "belong to --col_noise auto"),
                      (["--col_noise_max", "4"], "belong to --col_noise auto"),
                      # a FILE is a map that is already made
                      (["--col_noise", "m.tif", "--col_noise_frames", "8"], "--col_noise_frames belongs to --col_noise auto: --col_noise m.tif reads a map"),
                      (["--col_noise", "m.tif"] + curve, "--col_noise_curve belongs to --col_noise auto"),
                      (["--col_noise", "m.tif", "--col_noise_gate", "3"], "--col_noise_gate belongs"),
                      (["--col_noise", "m.tif", "--col_noise_sigma", "3"], "--col_noise_sigma belongs"),
                      (["--col_noise", "m.tif", "--col_noise_max", "3"], "--col_noise_max belongs"),
                      (auto + curve + ["--col_noise_frames", "0"], "--col_noise_frames must be >= 1"),
                      (auto + curve + ["--col_noise_gate", "0"], "--col_noise_gate is the gate"), (auto + curve + ["--col_noise_gate", "inf"], "--col_noise_gate is the gate"),
                      (auto + curve + ["--col_noise_gate", "nan"], "--col_noise_gate is the gate"),
                      (auto + curve + ["--col_noise_sigma", "-1"], "--col_noise_sigma is a number"), (auto + curve + ["--col_noise_sigma", "nan"], "--col_noise_sigma is a number"),
                      (auto + curve + ["--col_noise_max", "0"], "--col_noise_max"), (auto + curve + ["--col_noise_max", "inf"], "--col_noise_max"),
                      (auto + ["--col_noise_curve", "iso6400"], "iso3200, iso12800"), (auto + ["--col_noise_curve", "isox"], "iso3200, iso12800"),
                      (auto + ["--col_noise_curve", "1"], r"takes a,b\[,floor\]"), (auto + ["--col_noise_curve", "1,2,3,4"], r"takes a,b\[,floor\]"),
                      (auto + ["--col_noise_curve", "x,y"], r"takes a,b\[,floor\]"), (auto + ["--col_noise_curve", "inf,0"], "finite"),
                      (auto + ["--col_noise_curve", "1,nan"], "finite"), (auto + ["--col_noise_curve", "1,2,0"], "floor must be > 0")):
        with pytest.raises(SystemExit, match=word):
            denoise._parse(bad)
    assert denoise._parse([]).cols is None
    assert denoise._parse(["--col_noise", "m.tif"]).cols == ("file", "m.tif")
    assert denoise._parse(auto + curve).cols == ("auto", 32, 3.0, 3.0, TOP, "a,b", 8.0, 2000.0, 1.0)
    assert denoise._parse(auto + ["--col_noise_curve", "8,2000,4", "--col_noise_frames", "8", "--col_noise_gate", "2.5", "--col_noise_sigma", "0",
                                  "--col_noise_max", "12", "--bit_depth", "14"]).cols == ("auto", 8, 2.5, 0.0, 12.0, "a,b", 8.0, 2000.0, 4.0)
    assert denoise._parse(auto + ["--col_noise_curve", "auto", "--bit_depth", "10"]).cols == ("auto", 32, 3.0, 3.0, 1023.0 / 64.0, "auto", None, None, 1.0)
    assert denoise._parse(auto + ["--col_noise_curve", "iso3200"]).cols[5:] == ("iso3200",) + ISO3200 + (1.0,)
    # without a curve of its own the rule takes that of --dpc: its numbers, its floor, or its estimate
    assert denoise._parse(auto + ["--dpc", "4", "--dpc_iso", "3200"]).cols[5:] == ("dpc",) + ISO3200 + (1.0,)
    assert denoise._parse(auto + ["--dpc", "4", "--dpc_noise", "5,6,2"]).cols[5:] == ("dpc", 5.0, 6.0, 2.0)
    assert denoise._parse(auto + ["--dpc", "4", "--dpc_noise", "auto"]).cols[5:] == ("dpc", None, None, 1.0)
    assert denoise._parse(auto + ["--dpc", "4", "--dpc_iso", "3200", "--col_noise_curve", "1,2"]).cols[5:8] == ("a,b", 1.0, 2.0)
    for flag in ("--col_noise auto", "--col_noise FILE", "--col_noise_curve", "--col_noise_frames", "--col_noise_gate", "--col_noise_sigma", "--col_noise_max"):
        assert flag in denoise.__doc__, flag


def _recorded_estimate(monkeypatch, seen):
    """col_noise.estimate replaced by sixteen frames of eight significant columns of 5 DN and 24 of noise around zero"""
    from rvdd_release_amd import col_noise
    from rvdd_release_amd.util import _ops
    rng = np.random.default_rng(5)
    offsets = rng.normal(0.0, 2.0, (16, 2, 16)).astype(np.float32)
    offsets[:, 0, :8] += np.float32(5.0)
    state = np.ones((16, 2, 16), np.uint8)

    def estimate(rt, dataset, bit_depth, cfg, frames=32, max_videos=16):
        seen.append(("estimate", bit_depth, (cfg.k_gate, cfg.noise_a, cfg.noise_b, cfg.var_floor), frames))
        return offsets, state

    monkeypatch.setattr(col_noise, "estimate", estimate)
    monkeypatch.setattr(_ops, "ops_runtime", lambda device: None)
    return offsets, state


def test_prepass_finds_the_map_and_auto_shares_the_one_estimate_of_the_run(monkeypatch, capsys):
    from rvdd_release_amd import denoise
    seen = []

    def noise(dataset, dev, bit_depth, frames, flag='--dpc_noise'):
        seen.append(flag)
        return (7.0, 70.0)

    monkeypatch.setattr(denoise, "estimate_noise", noise)
    offsets, state = _recorded_estimate(monkeypatch, seen)
    data = Dataset((3,))
    auto = ["--col_noise", "auto"]
    for flags, flag in ((auto + ["--col_noise_curve", "auto"], "--col_noise_curve"), (auto + ["--dpc", "4", "--dpc_noise", "auto"], "--dpc_noise"),
                        (auto + ["--col_noise_curve", "auto", "--row_noise", "3", "--row_noise_curve", "auto", "--report", "r", "--report_noise", "auto"],
                         "--row_noise_curve")):
        del seen[:]
        opt = denoise._parse(flags + ["--col_noise_frames", "16"])
        denoise.prepasses(opt, data, torch.device("cpu"))
        assert seen == [flag, ("estimate", 12, (3.0, 7.0, 70.0, 1.0), 16)], (flags, seen)
        assert opt.cols[6:8] == (7.0, 70.0) and (opt.dpc is None or opt.dpc[2:4] == (7.0, 70.0))
        want = R.fit(offsets, state, 8, 3.0, TOP)
        assert np.array_equal(opt.cols_map.view(np.uint32), want["map"].view(np.uint32)) and (opt.cols_map[0, :8] != 0).all()
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("cols: ")][-1]
    m = re.fullmatch(r"cols: (\d+) applied, (\d+) insignificant, (\d+) unsupported, (\d+) clamped of 32 columns, map rms ([0-9.]+) DN "
                     r"\(the pooled estimate alone: ([0-9.]+) DN\), from 16 frames", line)
    assert m, line
    st = want["stats"]
    assert [int(m.group(i)) for i in (1, 2, 3, 4)] == [st["applied"] + st["clamped"], st["insignificant"], st["unsupported"], st["clamped"]]
    assert m.group(5) == "%.3f" % ((st["sum_q2"] / 32.0) ** 0.5 / 16.0) and m.group(6) == "%.3f" % st["floor_dn"] and int(m.group(1)) >= 8
    # without the flag the pre-pass leaves no map and estimates nothing
    del seen[:]
    opt = denoise._parse([])
    denoise.prepasses(opt, data, torch.device("cpu"))
    assert opt.cols_map is None and seen == []


def test_prepass_reads_a_file_and_says_what_is_wrong_with_one(tmp_path, monkeypatch, capsys):
    from rvdd_release_amd import col_noise, denoise, tiffio
    cmap = np.zeros((2, 16), np.float32)
    cmap[1, 3], cmap[0, 7] = 4.0, -3.0
    path = str(tmp_path / "cols.tif")
    col_noise.write_map(path, cmap)
    opt = denoise._parse(["--col_noise", path])
    denoise.prepasses(opt, Dataset((3,)), torch.device("cpu"))
    assert np.array_equal(opt.cols_map, cmap)
    assert "cols: 2 of 32 columns with an offset, map rms %.3f DN, from %s" % ((25.0 / 32.0) ** 0.5, path) in capsys.readouterr().out
    tiffio.write(path, np.zeros((2, 32), np.float32))
    with pytest.raises(SystemExit, match=r"--col_noise .*cols.tif: .*a column map is a one-row float image"):
        denoise.prepasses(denoise._parse(["--col_noise", path]), Dataset((3,)), torch.device("cpu"))
    with pytest.raises(SystemExit, match=r"--col_noise .*missing.tif"):
        denoise.prepasses(denoise._parse(["--col_noise", str(tmp_path / "missing.tif")]), Dataset((3,)), torch.device("cpu"))


def test_the_calls_with_the_flag(monkeypatch):
    cmap = np.full((2, 16), 2.0, np.float32)
    rt, written = _run(monkeypatch, ["--col_noise", "m.tif"], cmap)
    assert written == 3 + 2 + 4
    assert rt.calls.count("set_cols") == 2 and rt.args["set_cols"][0][0] is cmap and rt.args["set_cols"][1] == (None,)
    assert rt.calls.index("set_dpc") < rt.calls.index("set_cols") < rt.calls.index("set_match") < rt.calls.index("video_push")
    # one camera per run: a map of another width ends the run before any push
    with pytest.raises(SystemExit, match="--col_noise: the map is one of 36 mosaic columns.*32 x 32"):
        _run(monkeypatch, ["--col_noise", "m.tif"], np.zeros((2, 18), np.float32))


def test_without_the_flag_no_new_runtime_call_is_made(monkeypatch, capsys):
    rt, written = _run(monkeypatch, [], None)
    assert written == 9
    assert set(rt.calls) == {"set_option", "set_dpc", "set_match", "video_push", "egress"}, set(rt.calls)
    assert "cols:" not in capsys.readouterr().out


def test_the_command_estimates_fits_writes_and_prints_one_json_line(tmp_path, monkeypatch, capsys):
    from rvdd_release_amd import col_noise
    seen = []
    offsets, state = _recorded_estimate(monkeypatch, seen)
    monkeypatch.setattr(col_noise, "open_rawvideo", lambda opt, rest, who: Dataset((3,)))
    path = str(tmp_path / "cols.tif")
    r = col_noise.main(["--col_noise_curve", "iso3200", "--col_noise_frames", "16", "--col_noise_sigma", "2", "--out", path])
    assert seen == [("estimate", 12, (3.0, np.float32(ISO3200[0]), np.float32(ISO3200[1]), 1.0), 16)]
    want = R.fit(offsets, state, 8, 2.0, TOP)
    assert np.array_equal(col_noise.read_map(path).view(np.uint32), want["map"].view(np.uint32))
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line) == json.loads(col_noise.format_line(r)) and line == col_noise.format_line(r)
    assert set(r) == {"frames", "columns", "applied", "clamped", "insignificant", "unsupported", "rms_dn", "floor_dn"} and r["frames"] == 16 and r["columns"] == 32
    with pytest.raises(SystemExit, match="--out FILE is required"):
        col_noise.main(["--col_noise_curve", "iso3200"])
    with pytest.raises(SystemExit, match="needs the sensor's noise curve"):
        col_noise.main(["--out", path])
    with pytest.raises(SystemExit, match="--col_noise belongs to denoise"):
        col_noise.main(["--col_noise", "m.tif", "--out", path, "--col_noise_curve", "iso3200"])
