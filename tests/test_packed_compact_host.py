"""Compact packing on the host (data/packed.py, compact=True): the plan keeps the live sequences in slots 0 .. n-1 by
moving the highest live slot into a hole no video is left for, and compute_validation(..., compact=True) equals the serial
path -- with a fake model whose per-slot recurrent state follows 'moves' and whose output depends on that state and, as
the online flow does, on the previous output found through 'prev_index'."""
import os
import random
from collections import Counter, OrderedDict

import pytest
import torch

from packed_fakes import FakeDataset, FakeLoader, FakeModel, VIDEOS, _opt
from rvdd_release_amd import validate
from rvdd_release_amd.data.packed import PackedLoader, plan_packs

# the default mix of tools/packed_bench.py (seed 2024): frames per video; a video of T frames has T - 1 samples
BENCH_LENGTHS = [17, 35, 9, 9, 36, 13, 39, 32, 18, 40, 10, 37]


def _as_videos(sample_counts):
    videos, k = [], 0
    for c in sample_counts:
        videos.append(list(range(k, k + c)))
        k += c
    return videos


def _check_compact_pack(pack, plain, videos, B):
    """Every condition a compact plan has to meet, for one pack; -> the number of moves."""
    video_of = {i: v for v, vid in enumerate(videos) for i in vid}
    seen, firsts, moves_total = [], Counter(), 0
    slots = {}                           # slot -> (video, next sample expected), as the runtime's state would be
    assert len(pack) == len(plain)       # as many steps as the plan that idles its finished slots
    for row in pack:
        n = len(row)
        assert 1 <= n <= B
        assert len(row.prev_index) == n
        before = dict(slots)             # the previous step's batch: slot b held before[b]
        # moves: from a live slot (a video with samples left) to a hole (finished or never used), disjoint in a step
        used = set()
        for f, t in row.moves:
            assert 0 <= f < B and 0 <= t < B
            assert f not in used and t not in used and f != t
            used.update((f, t))
            assert f in slots and slots[f][1] is not None, (f, slots)
            assert t not in slots or slots[t][1] is None, (t, slots)
            slots[t] = slots.pop(f)
        moves_total += len(row.moves)
        for b, (i, first, live) in enumerate(row):
            assert live is True
            seen.append(i)
            v = video_of[i]
            if first:
                assert i == videos[v][0]
                assert row.prev_index[b] == -1
                firsts[v] += 1
            else:
                # the slot's state is this video's, at this sample; the previous output is where prev_index says
                assert slots[b] == (v, i), (b, i, slots.get(b))
                assert before[row.prev_index[b]] == (v, i)
            nxt = i + 1 if i + 1 in videos[v] else None
            slots[b] = (v, nxt)
        for b in [b for b in slots if b >= n]:      # a slot that sat the step out is undefined afterwards
            assert slots[b][1] is None, (b, slots[b])
            del slots[b]
    assert sorted(seen) == sorted(i for vid in videos for i in vid)       # every sample exactly once
    assert all(firsts[v] == 1 for v in range(len(videos)))                 # one FirstOfVideo per video
    assert moves_total <= max(B - 1, 0)
    return moves_total


@pytest.mark.parametrize("B", range(1, 10))
def test_compact_plan_conditions_random_sets(B):
    rng = random.Random(1000 + B)
    for _ in range(60):
        counts = [rng.randint(1, 25) for _ in range(rng.randint(1, 14))]
        videos = _as_videos(counts)
        sizes = [(4, 4)] * len(videos)
        (pack,) = plan_packs(videos, sizes, B, compact=True)
        (plain,) = plan_packs(videos, sizes, B)
        _check_compact_pack(pack, plain, videos, B)
        assert sum(len(row) for row in pack) == sum(counts)


def test_compact_plan_two_sizes():
    videos = _as_videos([4, 2, 6, 3, 5])
    sizes = [(4, 4), (2, 2), (4, 4), (2, 2), (4, 4)]
    packs = plan_packs(videos, sizes, 2, compact=True)
    plain = plan_packs(videos, sizes, 2)
    assert len(packs) == 2
    _check_compact_pack(packs[0], plain[0], [videos[0], videos[2], videos[4]], 2)
    _check_compact_pack(packs[1], plain[1], [videos[1], videos[3]], 2)


@pytest.mark.parametrize("B,steps,plain_slot_steps,moves,hist", [
    (4, 87, 348, 2, {1: 5, 2: 22, 3: 6, 4: 54}),
    (8, 52, 416, 4, {1: 5, 2: 9, 3: 3, 4: 1, 5: 3, 6: 6, 7: 4, 8: 21}),
])
def test_compact_plan_of_the_bench_mix(B, steps, plain_slot_steps, moves, hist):
    videos = _as_videos([T - 1 for T in BENCH_LENGTHS])
    sizes = [(360, 640)] * len(videos)
    (pack,) = plan_packs(videos, sizes, B, compact=True)
    (plain,) = plan_packs(videos, sizes, B)
    assert sum(len(row) for row in pack) == 283            # one slot-step per output frame
    assert sum(len(row) for row in plain) == plain_slot_steps
    assert len(pack) == len(plain) == steps
    assert _check_compact_pack(pack, plain, videos, B) == moves
    assert dict(Counter(len(row) for row in pack)) == hist


def test_compact_false_is_todays_plan():
    videos = [[0, 1, 2], [3], [4, 5], [6, 7]]
    want = [
        [(0, True, True), (3, True, True)],
        [(1, False, True), (4, True, True)],
        [(2, False, True), (5, False, True)],
        [(6, True, True), (5, False, False)],
        [(7, False, True), (5, False, False)],
    ]
    assert plan_packs(videos, [(4, 4)] * 4, 2) == [want]
    assert plan_packs(videos, [(4, 4)] * 4, 2, compact=False) == [want]
    (pack,) = plan_packs(videos, [(4, 4)] * 4, 2, compact=True)
    assert [list(r) for r in pack] == [want[0], want[1], want[2], [(6, True, True)], [(7, False, True)]]
    assert [r.moves for r in pack] == [[], [], [], [], []]
    # slot 0 ends first once the queue is empty: the live slot 1 moves into it
    (pack,) = plan_packs([[0], [1, 2, 3]], [(4, 4)] * 2, 2, compact=True)
    assert [list(r) for r in pack] == [[(0, True, True), (1, True, True)], [(2, False, True)], [(3, False, True)]]
    assert [r.moves for r in pack] == [[], [(1, 0)], []]
    assert [r.prev_index for r in pack] == [[-1, -1], [1], [0]]


def test_compact_loader_dicts(tmp_path):
    ds = FakeDataset(str(tmp_path))
    loader = PackedLoader(FakeLoader(ds), 3, compact=True)
    plain = PackedLoader(FakeLoader(ds), 3)
    assert loader.tail_waste() == 0 and plain.tail_waste() > 0
    assert loader.steps() == plain.steps()
    assert len(loader) == len(plain) == len(ds)
    total = 0
    for data in loader:
        n = data['n'].shape[0]
        total += n
        assert 1 <= n <= 3 and data['slots'] == 3
        assert data['gt'].shape[0] == n and data['flow'].shape[0] == n
        assert data['live'].tolist() == [True] * n and data['FirstOfVideo'].shape == (n,)
        assert len(data['index']) == len(data['n_path']) == len(data['gt_path']) == len(data['prev_index']) == n
        assert all(len(m) == 2 for m in data['moves'])
    assert total == len(ds)
    assert loader.moves() == sum(len(row.moves) for p in loader.packs for row in p)


class MovingModel(FakeModel):
    """FakeModel on a runtime of 'slots' slots: the per-slot recurrent state follows 'moves' (a source slot is undefined
    afterwards, as are the slots that sit a step out), and the output also depends on the previous output of the sequence,
    looked up through 'prev_index' as the online flow looks it up."""

    drop_moves = False
    ignore_prev_index = False

    def test(self):
        data = self.data
        n = data['n']
        for f, t in ([] if self.drop_moves else data.get('moves', [])):
            self.state[t] = self.state.pop(f)
        prev = getattr(self, 'denoised', None)
        pidx = data.get('prev_index')
        outs = []
        for b in range(n.shape[0]):
            v, f = float(n[b, 0, 0, 0]), float(n[b, 0, 0, 1])
            if self.first[b]:
                self.state[b] = (v, 0)
                carry = 0.0
            else:
                p = b if (pidx is None or self.ignore_prev_index) else pidx[b]
                carry = float(prev[p].flatten()[0])
            start, count = self.state[b]
            self.state[b] = (start, count + 1)
            H, W = 2 * n.shape[2], 2 * n.shape[3]
            outs.append(torch.full((3, H, W), 0.001 * (100 * v + 10 * f + count) + 0.37 * start + 0.25 * carry) - 0.5)
        self.denoised = torch.stack(outs)
        if 'slots' in data:
            for b in [b for b in self.state if b >= n.shape[0]]:
                self.state[b] = (-77.0, 1000)          # undefined: garbage that shows if it is ever used


# slots end in an order that needs moves at B = 3 and 4, one frame size so that it is one pack
TAIL_VIDEOS = OrderedDict([("000", (3, 4, 6)), ("001", (9, 4, 6)), ("002", (4, 4, 6)), ("003", (8, 4, 6)),
                           ("004", (2, 4, 6)), ("005", (7, 4, 6))])


def _run(tmp_path, tag, batch_size, compact, videos, model=None):
    ds = FakeDataset(str(tmp_path / "data"), videos)
    out = tmp_path / tag
    order, seen = [], {}

    def on_frame(i, d, vis, losses):
        order.append((i, d['n_path'], d['gt_path'], d['FirstOfVideo'], tuple(d['n'].shape)))
        seen[i] = vis['denoised'].clone()
        assert 'moves' not in d and 'slots' not in d

    res = validate.compute_validation(model or MovingModel(), FakeLoader(ds), _opt(), val_image_dir=str(out),
                                      batch_size=batch_size, compact=compact, on_frame=on_frame)
    files = {os.path.relpath(os.path.join(d, f), out): open(os.path.join(d, f), "rb").read()
             for d, _, fs in os.walk(out) for f in fs}
    return res, files, order, seen


@pytest.mark.parametrize("videos", [VIDEOS, TAIL_VIDEOS], ids=["two_sizes", "tail"])
@pytest.mark.parametrize("B", [2, 3, 4, 8])
def test_compact_validation_equals_serial(tmp_path, B, videos):
    want = _run(tmp_path, "serial", 1, False, videos)
    got = _run(tmp_path, f"compact{B}", B, True, videos)
    assert got[0] == want[0]                                  # returned losses, float for float
    assert got[1] == want[1]                                  # every TIFF and output.log, byte for byte
    assert sorted(got[2]) == sorted(want[2])                  # on_frame: each frame once, as the serial loader shows it
    assert sorted(got[3]) == sorted(want[3])
    for i in want[3]:
        assert torch.equal(got[3][i], want[3][i]), i


def test_compact_validation_needs_moves_and_prev_index(tmp_path):
    """The plan of TAIL_VIDEOS at B = 3 has moves; a model that drops them, or looks its previous output up in its own
    slot, gives other frames -- so the test above does check both."""
    ds = FakeDataset(str(tmp_path / "data"), TAIL_VIDEOS)
    assert PackedLoader(FakeLoader(ds), 3, compact=True).moves() > 0
    want = _run(tmp_path, "serial", 1, False, TAIL_VIDEOS)
    for tag, attr in (("nomove", "drop_moves"), ("noprev", "ignore_prev_index")):
        bad = MovingModel()
        setattr(bad, attr, True)
        got = _run(tmp_path, tag, 3, True, TAIL_VIDEOS, model=bad)
        assert any(not torch.equal(got[3][i], want[3][i]) for i in want[3]), tag


def test_val_compact_slots_flag():
    from rvdd_release_amd.options import make_opt, parse
    assert make_opt().val_compact_slots is False
    assert parse(["--val_batch_size", "4"]).val_compact_slots is False
    opt = parse(["--val_batch_size", "4", "--val_compact_slots"])
    assert opt.val_batch_size == 4 and opt.val_compact_slots is True
