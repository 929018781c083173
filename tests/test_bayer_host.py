"""Bayer patterns other than GBRG, on the host: the pattern-aware CPU restatement of Hamilton-Adams (tests/bayer_ref.py)
against the reference's own HamiltonAdam(pattern) (tests/golden/op_hamilton_adams_bayer.npz, tools/make_golden_bayer.py),
the Python surface (HamiltonAdam, --bayer_pattern, synth) and the C ABI's declarations.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import bayer_ref as R
from conftest import GOLDEN, REPO

FIXTURE = os.path.join(GOLDEN, "op_hamilton_adams_bayer.npz")
REF = "/root/reference"


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_restatement_equals_the_reference_fixture(pattern):
    g = np.load(FIXTURE)
    got = R.hamilton_adams(torch.from_numpy(g["raw"]), pattern).numpy()
    assert got.shape == g[f"rgb_{pattern}"].shape
    assert np.array_equal(got, g[f"rgb_{pattern}"]), float(np.abs(got - g[f"rgb_{pattern}"]).max())


def test_fixture_patterns_differ_and_gbrg_is_the_old_fixture():
    g = np.load(FIXTURE)
    outs = [g[f"rgb_{p}"] for p in R.PATTERNS]
    assert all(not np.array_equal(outs[i], outs[j]) for i in range(4) for j in range(i + 1, 4))
    old = np.load(os.path.join(GOLDEN, "op_hamilton_adams.npz"))
    assert np.array_equal(R.hamilton_adams(torch.from_numpy(old["raw"]), "gbrg").numpy(), old["rgb"])


@pytest.mark.parametrize("pattern", sorted(R.CROPS))
def test_restatement_interior_identity(pattern):
    got, want = R.interior_identity(lambda x, p: R.hamilton_adams(x, p), pattern, torch.Generator().manual_seed(5))
    assert torch.equal(got, want)


def test_hamilton_adam_constructs_for_the_four_patterns_only():
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    for p in R.PATTERNS:
        assert HamiltonAdam(p).pattern == p
    for bad in ("GBRG", "rgbg", "xtrans", ""):
        with pytest.raises(NotImplementedError) as e:
            HamiltonAdam(bad)
        assert all(p in str(e.value) for p in R.PATTERNS), str(e.value)


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_remosaick_is_the_inverse_of_the_packing(pattern):
    """pack_in_one(remosaick(x)) samples channel colour_P(y, x) of x at every pixel; remosaick(HA(raw)) == raw."""
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    x = torch.randn(2, 3, 12, 18, generator=torch.Generator().manual_seed(3))
    y = HamiltonAdam(pattern).remosaick(x)
    assert y.shape == (2, 4, 6, 9)
    cfa = R.pack_in_one(y)
    ch = torch.tensor(R.RGB_OF_SITE)[R.colour_sites(12, 18, pattern)]
    assert torch.equal(cfa, x.gather(1, ch[None, None].expand(2, 1, 12, 18))[:, 0])
    assert torch.equal(y, R.remosaick(x, pattern))
    raw = torch.rand(1, 4, 7, 9, generator=torch.Generator().manual_seed(4)) * 2 - 1
    assert torch.equal(HamiltonAdam(pattern).remosaick(R.hamilton_adams(raw, pattern)), raw)


def test_gbrg_remosaick_is_the_reference_indexing():
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    import rvdd_oracle as O
    x = torch.randn(1, 3, 10, 14, generator=torch.Generator().manual_seed(9))
    assert torch.equal(HamiltonAdam("gbrg").remosaick(x), O.remosaick(x))


def test_synth_pattern_is_deterministic_and_default_is_gbrg():
    from rvdd_release_amd import synth
    a = synth.make_sequence(3, 16, 24, seed=5)
    assert torch.equal(a.raw, synth.make_sequence(3, 16, 24, seed=5, pattern="gbrg").raw)
    for p in R.PATTERNS[1:]:
        s1, s2 = synth.make_sequence(3, 16, 24, seed=5, pattern=p), synth.make_sequence(3, 16, 24, seed=5, pattern=p)
        assert torch.equal(s1.raw, s2.raw) and torch.equal(s1.gt, a.gt) and torch.equal(s1.flow_prev, a.flow_prev)
        assert not torch.equal(s1.raw, a.raw)
    with pytest.raises(ValueError):
        synth.make_sequence(2, 16, 16, pattern="xyz")


@pytest.mark.parametrize("pattern", R.PATTERNS)
def test_synth_mosaics_the_clean_frame_in_the_pattern(pattern):
    """Without noise (a DN level where sigma^2 = a u - b clips to 0) the raw frame is the pattern's re-mosaic of gt."""
    from rvdd_release_amd import synth
    real = dict(synth.ISO_PARAMS[3200])
    try:
        synth.ISO_PARAMS[3200] = dict(real, a=0.0, b=0.0)
        s = synth.make_sequence(2, 16, 20, seed=1, pattern=pattern)
    finally:
        synth.ISO_PARAMS[3200] = real
    assert (s.raw - R.remosaick(s.gt, pattern)).abs().max() < 1e-6


def test_options_carry_the_pattern_without_renaming_the_experiment():
    from rvdd_release_amd.options import make_opt, parse
    from rvdd_release_amd.models.recurrent_model import recurrentModel
    import argparse
    assert make_opt().bayer_pattern == "gbrg"
    assert make_opt(bayer_pattern="rggb").name == make_opt().name
    assert parse(["--bayer_pattern", "bggr"]).bayer_pattern == "bggr"
    with pytest.raises(SystemExit):
        parse(["--bayer_pattern", "rgbg"])
    p = recurrentModel.modify_commandline_options(argparse.ArgumentParser(), is_train=False)
    assert p.parse_args([]).bayer_pattern == "gbrg" and p.parse_args(["--bayer_pattern", "grbg"]).bayer_pattern == "grbg"


def test_header_declares_the_pattern_enum_option_and_entry_point():
    txt = open(os.path.join(REPO, "include", "rvdd.h")).read()
    for name, v in (("GBRG", 0), ("GRBG", 1), ("RGGB", 2), ("BGGR", 3)):
        assert re.search(rf"RVDD_BAYER_{name}\s*=\s*{v}\b", txt), name
    doc = txt[txt.index("Known names:"):txt.index("int rvdd_set_option(")]
    assert '"bayer_pattern"' in doc
    assert re.search(r"int rvdd_demosaic_ha_bayer\(rvdd_t\* h, const float\* raw, int32_t n, int32_t hh, int32_t ww, "
                     r"int32_t pattern,\s+float\* rgb, void\* stream\);", txt)
    assert "packed raw in the handle's Bayer pattern" in txt


def test_library_exports_the_pattern_entry_point():
    from rvdd_release_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rvdd_demosaic_ha_bayer")
    assert lib.rvdd_demosaic_ha_bayer.argtypes[5] is C.c_int32
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\sT\s+rvdd_demosaic_ha_bayer\b", out)
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"bayer_pattern must be 0 (GBRG), 1 (GRBG), 2 (RGGB) or 3 (BGGR)" in blob


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")), reason="reference tree not present")
def test_make_golden_bayer_regenerates_the_fixture(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_golden_bayer.py"), "--out", str(tmp_path)], cwd=REPO,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = np.load(os.path.join(tmp_path, "op_hamilton_adams_bayer.npz")), np.load(FIXTURE)
    assert set(a.files) == set(b.files) == {"raw"} | {f"rgb_{p}" for p in R.PATTERNS}
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
