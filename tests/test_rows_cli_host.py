"""`denoise --row_noise` without a device: the flags and every refusal, the calls of a run over a recording runtime with and without
the flag, and the `rows:` line."""
import re
import types

import numpy as np
import pytest
import torch

import rows_ref as R

ISO3200 = (8.0034, 2043.51144)
H = W = 32


class RecordingRuntime:
    """What denoise.run_group drives, recording every call and its arguments; every pushed frame adds 30 applied rows (two of them
    clamped), 2 skipped ones and q = 8 (half a DN) per applied row to its slot."""

    def __init__(self, B):
        self.B, self.calls, self.args, self.rows_on = B, [], {}, False
        self.acc = [R.new_acc(1) for _ in range(B)]
        self.count = [0] * B

    def __getattr__(self, name):
        if name.startswith(("set_", "dpc_counts")):
            def call(*a, **k):
                self.calls.append(name)
                self.args.setdefault(name, []).append(a)
                if name == "set_rows":
                    self.rows_on = a[0] is not None
                return [(0, 0)] * self.B
            return call
        raise AttributeError(name)

    def video_push(self, frames, ctl, bit_depth, layout, out=None, container=None):
        self.calls.append("video_push")
        valid = []
        for b, c in enumerate(ctl):
            self.count[b] = 0 if c == 2 else 1 if c == 1 else self.count[b] + 1
            valid.append(self.count[b] >= 2)
            if c != 2 and self.rows_on:
                frame = {"applied": np.array([30], np.uint32), "skipped": np.array([2], np.uint32), "clamped": np.array([2], np.uint32),
                         "sum_q2": np.array([30 * 64], np.int64)}
                self.acc[b] = R.add(self.acc[b], frame)
        return torch.zeros(self.B, 3, H, W), valid

    def egress(self, rgb, layout, sample, depth, out=None):
        self.calls.append("egress")
        return torch.zeros(self.B, H, W, 3)

    def rows_read(self, slot):
        self.calls.append("rows_read")
        acc, self.acc[slot] = self.acc[slot], R.new_acc(1)
        return acc


class Dataset:
    container, layout, dtype = None, "mosaic", np.uint16

    def __init__(self, lengths):
        self.videos = [("%03d" % v, ["%03d/%08d.tif" % (v, t) for t in range(n)]) for v, n in enumerate(lengths)]

    def read_frame(self, path):
        return np.zeros((H, W), np.uint16)


def _run(monkeypatch, flags, lengths=(4, 3, 5), B=2):
    from rvdd_release_amd import denoise
    opt = denoise._parse(["--batch_size", str(B)] + flags)
    rt = RecordingRuntime(B)
    model = types.SimpleNamespace(device=torch.device("cpu"), training_unrollings=2,
                                  _netDenoise=types.SimpleNamespace(runtime_for=lambda B, H, W, pin=True: rt))
    monkeypatch.setattr(denoise, "write_frame", lambda *a, **k: None)
    data = Dataset(lengths)
    return rt, denoise.run_group(opt, model, data, data.videos, H, W, None, None)


def test_flags_and_every_refusal():
    from rvdd_release_amd import denoise
    with pytest.raises(SystemExit, match=r"--row_noise needs the sensor's noise curve.*--row_noise_curve a,b\[,floor\].*auto.*iso3200 / iso12800.*--dpc"):
        denoise._parse(["--row_noise", "3"])
    curve = ["--row_noise_curve", "8,2000"]
    for bad, word in ((["--row_noise_curve", "1,2"], "belong to --row_noise K"), (["--row_noise_max", "4"], "belong to --row_noise K"),
                      (["--row_noise", "0"] + curve, "--row_noise is the gate"), (["--row_noise", "-3"] + curve, "--row_noise is the gate"),
                      (["--row_noise", "inf"] + curve, "--row_noise is the gate"), (["--row_noise", "nan"] + curve, "--row_noise is the gate"),
                      (["--row_noise", "3", "--row_noise_curve", "iso6400"], "iso3200, iso12800"),
                      (["--row_noise", "3", "--row_noise_curve", "isox"], "iso3200, iso12800"),
                      (["--row_noise", "3", "--row_noise_curve", "1"], r"takes a,b\[,floor\]"),
                      (["--row_noise", "3", "--row_noise_curve", "1,2,3,4"], r"takes a,b\[,floor\]"),
                      (["--row_noise", "3", "--row_noise_curve", "x,y"], r"takes a,b\[,floor\]"),
                      (["--row_noise", "3", "--row_noise_curve", "inf,0"], "finite"), (["--row_noise", "3", "--row_noise_curve", "1,nan"], "finite"),
                      (["--row_noise", "3", "--row_noise_curve", "1,2,0"], "floor must be > 0"),
                      (["--row_noise", "3", "--row_noise_max", "0"] + curve, "--row_noise_max"),
                      (["--row_noise", "3", "--row_noise_max", "inf"] + curve, "--row_noise_max")):
        with pytest.raises(SystemExit, match=word):
            denoise._parse(bad)
    assert denoise._parse([]).rows is None
    top = 4095.0 / 64.0
    assert denoise._parse(["--row_noise", "3"] + curve).rows == (3.0, "a,b", 8.0, 2000.0, 1.0, top)
    assert denoise._parse(["--row_noise", "2.5", "--row_noise_curve", "8,2000,4", "--row_noise_max", "12", "--bit_depth", "14"]).rows == \
        (2.5, "a,b", 8.0, 2000.0, 4.0, 12.0)
    assert denoise._parse(["--row_noise", "3", "--row_noise_curve", "auto", "--bit_depth", "10"]).rows == (3.0, "auto", None, None, 1.0, 1023.0 / 64.0)
    assert denoise._parse(["--row_noise", "3", "--row_noise_curve", "iso3200"]).rows == (3.0, "iso3200") + ISO3200 + (1.0, top)
    a, b = denoise._parse(["--row_noise", "3", "--row_noise_curve", "iso12800", "--bit_depth", "10"]).rows[2:4]
    assert abs(a - 28.3015 * 1023 / 4095) < 1e-12 and abs(b - 6307.62081 * (1023 / 4095) ** 2) < 1e-9
    # without a curve of its own the stage takes that of --dpc: its numbers, its floor, or its estimate
    assert denoise._parse(["--row_noise", "3", "--dpc", "4", "--dpc_iso", "3200"]).rows == (3.0, "dpc") + ISO3200 + (1.0, top)
    assert denoise._parse(["--row_noise", "3", "--dpc", "4", "--dpc_noise", "5,6,2"]).rows == (3.0, "dpc", 5.0, 6.0, 2.0, top)
    assert denoise._parse(["--row_noise", "3", "--dpc", "4", "--dpc_noise", "auto"]).rows == (3.0, "dpc", None, None, 1.0, top)
    # ... and its own where it has one
    assert denoise._parse(["--row_noise", "3", "--dpc", "4", "--dpc_iso", "3200", "--row_noise_curve", "1,2"]).rows[1:4] == ("a,b", 1.0, 2.0)
    assert "--row_noise K" in denoise.__doc__ and "--row_noise_curve" in denoise.__doc__ and "--row_noise_max" in denoise.__doc__


def test_auto_shares_the_one_estimate_of_the_run(monkeypatch):
    from rvdd_release_amd import denoise
    seen = []

    def estimate(dataset, dev, bit_depth, frames, flag='--dpc_noise'):
        seen.append(flag)
        return (7.0, 70.0)

    monkeypatch.setattr(denoise, "estimate_noise", estimate)
    data = Dataset((3,))
    for flags, flag in ((["--row_noise", "3", "--row_noise_curve", "auto"], "--row_noise_curve"),
                        (["--row_noise", "3", "--dpc", "4", "--dpc_noise", "auto"], "--dpc_noise"),
                        (["--row_noise", "3", "--row_noise_curve", "auto", "--dpc", "4", "--dpc_noise", "auto", "--report", "r", "--report_noise", "auto"],
                         "--dpc_noise")):
        del seen[:]
        opt = denoise._parse(flags)
        denoise.prepasses(opt, data, torch.device("cpu"))
        assert seen == [flag] and opt.rows[2:4] == (7.0, 70.0), (flags, seen, opt.rows)
        assert opt.dpc is None or opt.dpc[2:4] == (7.0, 70.0)


def test_the_calls_with_the_flag_and_the_line(monkeypatch, capsys):
    rt, written = _run(monkeypatch, ["--row_noise", "3", "--row_noise_curve", "iso3200", "--row_noise_max", "20"])
    assert written == 3 + 2 + 4
    assert rt.calls.count("set_rows") == 2 and rt.calls.count("rows_read") == 3 and not rt.rows_on
    cfg = rt.args["set_rows"][0][0]
    assert (cfg.k_gate, cfg.var_floor, cfg.max_dn) == (3.0, 1.0, 20.0) and abs(cfg.noise_a - ISO3200[0]) < 1e-6 and abs(cfg.noise_b - ISO3200[1]) < 1e-3
    assert rt.args["set_rows"][1] == (None,)
    assert rt.calls.index("set_rows") < rt.calls.index("set_match") < rt.calls.index("video_push")
    lines = sorted((ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("rows: ")), key=lambda ln: ln[-5:])
    assert len(lines) == 3
    from rvdd_release_amd.runtime import rows_floor_rms
    floor = rows_floor_rms(*ISO3200, 1.0, 12, W // 2)
    assert abs(floor - 1.35 * ((ISO3200[0] * 2047.5 - ISO3200[1]) / 32.0) ** 0.5) < 1e-9
    for ln, (key, n) in zip(lines, (("000", 4), ("001", 3), ("002", 5))):
        m = re.fullmatch(r"rows: (\d+) applied, (\d+) skipped, (\d+) clamped rows, rms offset ([0-9.]+) DN \(the estimate alone, on flat footage "
                         r"without row noise: ([0-9.]+) DN\) in (\d+) frames \((\d+)\)", ln)
        assert m, ln
        assert [int(m.group(i)) for i in (1, 2, 3, 6)] == [30 * n, 2 * n, 2 * n, n] and m.group(7) == key
        assert m.group(4) == "0.500" and m.group(5) == "%.3f" % floor


def test_without_the_flag_no_new_runtime_call_is_made(monkeypatch, capsys):
    rt, written = _run(monkeypatch, [])
    assert written == 9
    assert set(rt.calls) == {"set_option", "set_dpc", "set_match", "video_push", "egress"}, set(rt.calls)
    assert "rows:" not in capsys.readouterr().out
