#!/usr/bin/env python3
"""What the library of a tree of choice answers to the broken calls of tests/abi_refusals.cpp, recorded without a GPU:

    python3 tools/make_golden_abi_refusals.py --tree <checkout of the commit to record> [--out FILE]

Compiles THIS tree's tests/abi_refusals.cpp against the headers of --tree's rvdd-release_amd/csrc, links it with --tree's built
objects (`make print-objs` there names them), runs it and writes its lines -- function, case, return code, rvdd_last_error -- to
tests/golden/abi_refusals.txt.  The program hides every device from itself, so a call whose refusal is missing ends in "cannot select
device": such a line is reported and nothing is written.  Record from the commit whose refusals are to be kept, NOT from the tree that
folds them: tests/test_abi_refusals_host.py then holds the new code to the old code's every sentence."""
import argparse
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "abi_refusals.cpp")


def record(tree, hipcc="hipcc", arch="gfx950"):
    """the program's output for the built checkout `tree`, as text"""
    csrc = os.path.join(os.path.abspath(tree), "rvdd-release_amd", "csrc")
    objs = subprocess.run(["make", "-s", "--no-print-directory", "-C", csrc, "print-objs"], check=True, capture_output=True, text=True).stdout.split()
    missing = [o for o in objs if not os.path.exists(os.path.join(csrc, o))]
    if missing:
        raise SystemExit("%s is not built: %s missing (make -C %s)" % (tree, ", ".join(missing[:3]), csrc))
    with tempfile.TemporaryDirectory() as tmp:
        obj, prog = os.path.join(tmp, "abi_refusals.o"), os.path.join(tmp, "abi_refusals")
        subprocess.run([hipcc, "-O1", "-std=c++17", "-Wall", "-I" + csrc, "-c", SOURCE, "-o", obj], check=True)
        subprocess.run([hipcc, "--offload-arch=" + arch] + [os.path.join(csrc, o) for o in objs] + [obj, "-o", prog], check=True)
        return subprocess.run([prog], check=True, capture_output=True, text=True).stdout


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--tree", required=True, help="the built checkout whose library is recorded")
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "abi_refusals.txt"))
    args = p.parse_args(argv)
    text = record(args.tree, os.environ.get("HIPCC", "hipcc"))
    lines = text.splitlines()
    lost = [ln for ln in lines if "cannot select device" in ln or ln.split("\t")[2] == "0"]
    if lost:
        sys.exit("not a refusal, nothing written:\n" + "\n".join(lost))
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote %s: %d cases of %d functions, %d bytes" % (args.out, len(lines), len({ln.split("\t")[0] for ln in lines}), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
