"""The library's refusals against their own recorded past, without a GPU: tests/abi_refusals.cpp -- every entry point of ops.hip,
stream.hip and stages.hip from one valid argument set with one argument broken at a time, and the host-only entry points -- built
against this tree's objects and run, gives tests/golden/abi_refusals.txt line by line: function, case, return code and the sentence of
rvdd_last_error, byte for byte.  tools/make_golden_abi_refusals.py recorded the file from the commit BEFORE the checks got their shared
helpers; a deliberate change of a refusal records it anew, from the commit in front of that change."""
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rvdd-release_amd", "csrc")


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "hipcc")
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc to build tests/abi_refusals.cpp with")
    objs = subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, "print-objs"], check=True, capture_output=True, text=True).stdout.split()
    missing = [o for o in objs if not os.path.exists(os.path.join(CSRC, o))]
    if missing:
        pytest.skip("the library's objects are not built here (%s ...): make -C rvdd-release_amd/csrc" % missing[0])
    out = str(tmp_path_factory.mktemp("abi_refusals"))
    made = subprocess.run(["make", "-s", "-C", CSRC, "abi_refusals", "REFUSALS_DIR=" + out], capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    run = subprocess.run([os.path.join(out, "abi_refusals")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout.splitlines()


def test_every_refusal_is_the_recorded_one(lines):
    with open(os.path.join(GOLDEN, "abi_refusals.txt")) as f:
        gold = f.read().splitlines()
    differ = [(g, w) for g, w in zip(lines, gold) if g != w]
    print("%d refusals compared, %d differ" % (len(gold), len(differ)))
    assert not differ, differ[:5]
    assert len(lines) == len(gold), (len(lines), len(gold))


def test_the_record_is_one_of_refusals_only():
    """every recorded case was refused with a code, none reached the device, and the hand-written sentences all have their case"""
    with open(os.path.join(GOLDEN, "abi_refusals.txt")) as f:
        rows = [ln.split("\t") for ln in f.read().splitlines()]
    assert len(rows) >= 400 and all(len(r) == 4 for r in rows)
    assert all(int(r[2]) in (-1, -2) for r in rows), [r for r in rows if int(r[2]) not in (-1, -2)][:3]
    assert not [r for r in rows if "cannot select device" in r[3]]
    assert len({r[0] for r in rows}) >= 45      # the entry points
    for words in ("bit_depth must be 1..16", "is not an rvdd_bayer", "n must be >= 0", "is required", "2^31 - 1 blocks", "bad argument"):
        assert sum(words in r[3] for r in rows) >= 5, words
