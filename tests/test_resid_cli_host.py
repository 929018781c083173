"""`denoise --report` without a device: the flags, the JSON lines of a run over a recording runtime, and that a run without the flag
makes no call it did not make before."""
import json
import types

import numpy as np
import pytest
import torch

import resid_ref as R

ISO3200 = (8.0034, 2043.51144)
H = W = 32


class RecordingRuntime:
    """What denoise.run_group drives, recording every call; the stage's accumulators are the restatement's sums of white noise of the
    ISO 3200 curve around a ramp, one frame's worth per measured output."""

    def __init__(self, B):
        self.B, self.calls, self.resid_on = B, [], False
        rgb = R.ramp_rgb(128, 192, 12)
        self.frame = R.resid_ref(R.noisy_of(rgb, 0, 12, *ISO3200, seed=3), rgb, 0, 12)
        self.acc = [R.new_acc(1) for _ in range(B)]
        self.count = [0] * B

    def __getattr__(self, name):
        if name.startswith(("set_", "dpc_counts")):
            def call(*a, **k):
                self.calls.append(name)
                if name == "set_resid":
                    self.resid_on = bool(a[0])
                return [(0, 0)] * self.B
            return call
        raise AttributeError(name)

    def video_push(self, frames, ctl, bit_depth, layout, out=None, container=None):
        self.calls.append("video_push")
        valid = []
        for b, c in enumerate(ctl):
            self.count[b] = 0 if c == 2 else 1 if c == 1 else self.count[b] + 1
            valid.append(self.count[b] >= 2)
            if valid[b] and self.resid_on:
                self.acc[b] = R.add(self.acc[b], self.frame)
        return torch.zeros(self.B, 3, H, W), valid

    def egress(self, rgb, layout, sample, depth, out=None):
        self.calls.append("egress")
        return torch.zeros(self.B, H, W, 3)

    def resid_read(self, slot):
        self.calls.append("resid_read")
        acc, self.acc[slot] = self.acc[slot], R.new_acc(1)
        return acc


class Dataset:
    container, layout, dtype = None, "mosaic", np.uint16

    def __init__(self, lengths):
        self.videos = [("%03d" % v, ["%03d/%08d.tif" % (v, t) for t in range(n)]) for v, n in enumerate(lengths)]

    def read_frame(self, path):
        return np.zeros((H, W), np.uint16)


def _run(tmp_path, monkeypatch, flags, lengths=(4, 3, 5), B=2):
    from rvdd_release_amd import denoise
    opt = denoise._parse(["--batch_size", str(B)] + flags)
    rt = RecordingRuntime(B)
    model = types.SimpleNamespace(device=torch.device("cpu"), training_unrollings=2,
                                  _netDenoise=types.SimpleNamespace(runtime_for=lambda B, H, W, pin=True: rt))
    monkeypatch.setattr(denoise, "write_frame", lambda *a, **k: None)
    data = Dataset(lengths)
    out = None if opt.report is None else {"file": open(opt.report[0], "w"), "total": None, "frames": 0}
    args = (opt, model, data, data.videos, H, W, None, None)
    written = denoise.run_group(*args) if out is None else denoise.run_group(*args, out)
    if out is not None:
        out["file"].close()
    return rt, written, out


def test_report_without_a_curve_is_refused_with_the_message():
    from rvdd_release_amd import denoise
    with pytest.raises(SystemExit, match=r"--report needs the noise curve.*--report_noise a,b.*auto.*iso3200 / iso12800.*--match_noise"):
        denoise._parse(["--report", "r.jsonl"])
    for bad, word in ((["--report_noise", "1,2"], "belongs to --report"), (["--report", "r", "--report_noise", "iso6400"], "iso3200, iso12800"),
                      (["--report", "r", "--report_noise", "1"], "takes a,b"), (["--report", "r", "--report_noise", "x,y"], "takes a,b"),
                      (["--report", "r", "--report_noise", "inf,0"], "finite"),
                      (["--report", "r", "--report_noise", "1,2", "--match_noise", "auto", "--match_iso", "3200"], "does not go with --match_noise")):
        with pytest.raises(SystemExit, match=word):
            denoise._parse(bad)
    assert denoise._parse([]).report is None
    assert denoise._parse(["--report", "r", "--report_noise", "2.5,100", "--bit_depth", "14"]).report == ("r", "a,b", 2.5, 100.0, 14)
    assert denoise._parse(["--report", "r", "--report_noise", "auto"]).report == ("r", "auto", None, None, 12)
    assert denoise._parse(["--report", "r", "--report_noise", "iso3200"]).report == ("r", "iso3200") + ISO3200 + (12,)
    a, b = denoise._parse(["--report", "r", "--report_noise", "iso12800", "--bit_depth", "10"]).report[2:4]
    assert abs(a - 28.3015 * 1023 / 4095) < 1e-12 and abs(b - 6307.62081 * (1023 / 4095) ** 2) < 1e-9
    # under the match the yardstick is the checkpoint's curve, in the 12-bit DN the network sees, whatever the frames' depth
    assert denoise._parse(["--report", "r", "--match_noise", "60,900", "--match_iso", "12800", "--bit_depth", "10"]).report == \
        ("r", "match_iso12800", 28.3015, 6307.62081, 12)
    assert "--report FILE" in denoise.__doc__ and "--report_noise" in denoise.__doc__


def test_report_lines_have_the_fields(tmp_path, monkeypatch):
    from rvdd_release_amd import footage
    path = str(tmp_path / "report.jsonl")
    rt, written, out = _run(tmp_path, monkeypatch, ["--report", path, "--report_noise", "iso3200"])
    lines = [json.loads(ln) for ln in open(path).read().splitlines()]
    assert written == 3 + 2 + 4 and [r["video"] for r in sorted(lines, key=lambda r: r["video"])] == ["000", "001", "002"]
    for rec in lines:
        n = {"000": 3, "001": 2, "002": 4}[rec["video"]]
        assert set(rec) == {"video", "frames", "curve"} | set(footage.REPORT_KEYS) and rec["frames"] == n
        assert rec["curve"] == {"a": ISO3200[0], "b": ISO3200[1], "bit_depth": 12, "source": "iso3200"}
        assert rec["samples"] > 0.9 * n * 4 * 128 * 192 and rec["bins"] >= 40 and abs(rec["ratio"] - 1) < 0.03 and abs(rec["rho"]) < 0.02
    assert out["frames"] == 9 and int(out["total"]["n"].sum()) == 9 * 4 * 128 * 192
    assert rt.calls.count("resid_read") == 3 and rt.calls.count("set_resid") == 2 and not rt.resid_on
    # a video whose residual has too few usable bins still gets its line, with the library's message
    rec = footage.report_record(R.new_acc(1), 0, ("f", "a,b", 1.0, 0.0, 12), video="v")
    assert rec["ratio"] is None and "usable" in rec["error"] and rec["frames"] == 0


def test_without_the_flag_no_new_runtime_call_is_made(tmp_path, monkeypatch):
    rt, written, out = _run(tmp_path, monkeypatch, [])
    assert written == 9 and out is None
    assert set(rt.calls) == {"set_option", "set_dpc", "set_match", "video_push", "egress"}, set(rt.calls)
