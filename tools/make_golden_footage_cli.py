#!/usr/bin/env python3
"""What `denoise` makes of the command lines of tests/footage_cli_corpus.py, recorded from a tree of choice:

    PYTHONDONTWRITEBYTECODE=1 python3 tools/make_golden_footage_cli.py --tree <checkout of the commit to record> [--out FILE]

Writes tests/golden/footage_cli.json: per case what `footage_cli_corpus.entry` returns for the `rvdd_release_amd.denoise` of --tree
(default: this tree) -- the records `_parse` leaves or its refusal, and what `prepasses` asks, completes and prints over stubs of the
passes that read footage.  The corpus and `entry` are always this tree's; only the package under test is --tree's, whose library
must be built (the `match:` line comes from `rvdd_match_coeffs`).  Record from the commit whose behaviour is to be kept, NOT from
the tree that changes it: tests/test_footage_cli_golden_host.py then holds the new code to the old code's every answer."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--tree", default=REPO, help="the checkout whose rvdd_release_amd is recorded")
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "footage_cli.json"))
    args = p.parse_args(argv)
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.abspath(args.tree))
    import footage_cli_corpus as corpus
    from rvdd_release_amd import denoise
    assert os.path.abspath(denoise.__file__).startswith(os.path.abspath(args.tree) + os.sep), denoise.__file__
    rec = corpus.record(denoise)
    with open(args.out, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    refused = sum(isinstance(e, str) for e in rec["entries"])
    print("wrote %s: %d cases, %d refused by _parse, %d through prepasses, %d bytes"
          % (args.out, rec["cases"], refused, sum(not isinstance(e, str) and e[1] is not None for e in rec["entries"]), os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
