"""Every frame of a video out of the stream (option "stream_all_frames"), host side: the slot dealing with the step that
outputs a video's last frame, and the public surface -- no new ctl value, the option known to the built library.  No GPU."""
import os
import re

import pytest

from conftest import REPO

SETS = [((4, 2, 5, 3, 3), 3), ((6, 3, 7, 4, 4), 3), ((3,), 1), ((2, 2), 4), ((1, 1, 1, 5), 2), ((6, 1, 7, 2, 4), 3)]


@pytest.mark.parametrize("lengths,slots", SETS)
def test_deal_slots_with_tail(lengths, slots):
    from rvdd_release_amd import _lib
    from rvdd_release_amd.denoise import deal_slots
    NEXT, FIRST, IDLE = _lib.PUSH_NEXT, _lib.PUSH_FIRST, _lib.PUSH_IDLE
    steps = deal_slots(lengths, slots, tail=1)
    assert all(len(s) == slots for s in steps)
    seen = {v: [] for v in range(len(lengths))}
    tails = []
    for b in range(slots):
        last = None
        for s in steps:
            c, v, k = s[b]
            assert c in (NEXT, FIRST, IDLE)
            if c == IDLE:
                if v >= 0:
                    # the tail of video v: straight behind its last frame, in its slot, numbered N
                    assert k == lengths[v] and last is not None and last[0] != IDLE and last[1:] == (v, k - 1)
                    tails.append(v)
                else:
                    assert (v, k) == (-1, -1)
            else:
                seen[v].append(k)
                assert (c == FIRST) == (k == 0)                          # FIRST exactly at k == 0
                if c == NEXT:
                    assert last is not None and last[0] != IDLE and last[1:] == (v, k - 1)      # NEXT never after IDLE
                else:
                    # a slot's FIRST never follows a frame directly: one IDLE lies between two videos of a slot
                    assert last is None or last[0] == IDLE
            last = (c, v, k)
        assert last is not None and last[0] == IDLE                         # no slot ends on a frame: its tail follows
    assert all(seen[v] == list(range(n)) for v, n in enumerate(lengths))      # every frame once, in order
    assert sorted(tails) == list(range(len(lengths)))                    # exactly one tail per video
    started = [v for s in steps for c, v, k in s if c == FIRST]
    assert started == list(range(len(lengths)))                          # dealt in order
    assert all(any(v >= 0 for _, v, _ in s) for s in steps)              # no step without work, the last one included


@pytest.mark.parametrize("lengths,slots", SETS)
def test_deal_slots_without_tail_is_unchanged(lengths, slots):
    from rvdd_release_amd import _lib
    from rvdd_release_amd.denoise import deal_slots
    plain = deal_slots(lengths, slots)
    assert deal_slots(lengths, slots, tail=0) == plain == deal_slots(lengths, slots, 0)
    assert all((v, k) == (-1, -1) for s in plain for c, v, k in s if c == _lib.PUSH_IDLE)
    # the tail costs each slot one step per video it carries, nothing else: the same frames in the same slots' order
    frames = lambda steps: [[(v, k) for s in steps for c, v, k in [s[b]] if c != _lib.PUSH_IDLE] for b in range(slots)]
    assert sorted(sum(frames(deal_slots(lengths, slots, tail=1)), [])) == sorted(sum(frames(plain), []))


def test_no_new_ctl_value_and_the_option_is_known():
    from rvdd_release_amd import _lib
    txt = open(os.path.join(REPO, "include", "rvdd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    push = {k: int(v) for k, v in re.findall(r"\b(RVDD_PUSH_[A-Z0-9_]+)\s*=\s*(-?\d+)", code)}
    assert push == {"RVDD_PUSH_NEXT": 0, "RVDD_PUSH_FIRST": 1, "RVDD_PUSH_IDLE": 2}
    blob = open(_lib.LIB_PATH, "rb").read()
    m = re.search(rb"unknown option '%s' \(known: ([a-z0-9_, ]+)\)", blob)
    assert m, "the library's unknown-option message was not found"
    assert "stream_all_frames" in m.group(1).decode().split(", ")
    doc = txt[txt.index("Known names:"):txt.index("int rvdd_set_option(")]
    assert "stream_all_frames" in set(re.findall(r'^ \*   "([a-z0-9_]+)"', doc, flags=re.M))
    # the sentence this option retires is gone, and what replaces it is said where the caller reads it
    push_doc = txt[txt.index("enum rvdd_push"):txt.index("int rvdd_video_push(")]
    assert "(no flush)" not in push_doc
    assert "the oldest frame of the slot's video not yet output" in " ".join(push_doc.replace(" *", " ").split())
    assert "DROPS that video's tail" in push_doc


def test_denoise_takes_all_frames():
    from rvdd_release_amd import denoise
    assert denoise._parse(["--all_frames"]).all_frames is True and denoise._parse([]).all_frames is False
