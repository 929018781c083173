"""The footage front end against its own recorded past: every command line of footage_cli_corpus.CASES read by `denoise._parse` and
taken through `denoise.prepasses` gives what tests/golden/footage_cli.json holds -- the refusal's sentence, the stage records, the
one estimate asked, what the map passes are handed, and every printed line in order.  tools/make_golden_footage_cli.py recorded the
file from the commit BEFORE the stage records had names; a deliberate change of the command line records it anew, from the commit in
front of that change."""
import json
import os

import footage_cli_corpus as corpus
from conftest import GOLDEN


def test_every_recorded_command_line_reads_as_recorded():
    from rvdd_release_amd import denoise
    with open(os.path.join(GOLDEN, "footage_cli.json")) as f:
        gold = json.load(f)
    assert gold["cases"] == len(corpus.CASES) == len(gold["entries"]) and 400 <= len(corpus.CASES) <= 1500
    differ = []
    for argv, want in zip(corpus.CASES, gold["entries"]):
        got = json.loads(json.dumps(corpus.entry(denoise, argv)))       # tuples -> lists, as the file holds them
        if got != want:
            differ.append((argv, want, got))
        if not isinstance(want, str) and want[1] is not None:
            assert len(want[1][0]) <= 1, (argv, want[1][0])                # ONE estimate per run, whoever asks
    print("%d command lines compared, %d differ" % (len(corpus.CASES), len(differ)))
    assert not differ, differ[:3]


def test_the_corpus_covers_what_it_says():
    """the families, the words and the passes are all there: refusals, lines that parse, lines that estimate, and every curve flag"""
    with open(os.path.join(GOLDEN, "footage_cli.json")) as f:
        entries = json.load(f)["entries"]
    refused = [e for e in entries if isinstance(e, str)]
    through = [e[1] for e in entries if not isinstance(e, str) and e[1] is not None]
    assert len(refused) >= 150 and len(through) >= 200
    assert {a for asked, _, _, _ in through for a in asked} == {"--dpc_noise", "--row_noise_curve", "--col_noise_curve", "--match_noise", "--report_noise"}
    for flag in ("--dpc_noise", "--match_noise", "--row_noise_curve", "--col_noise_curve", "--report_noise"):
        for word in corpus.WORDS:
            assert any(flag in c and c[c.index(flag) + 1] == word for c in corpus.CASES), (flag, word)
