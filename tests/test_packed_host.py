"""Packed validation on the host: the slot plan of data/packed.py and compute_validation(..., batch_size=B) against
the serial path, with a fake dataset and a fake model whose output is a deterministic function of (video, frame) and
of its own per-slot recurrence (so a wrong FirstOfVideo changes the output)."""
import os

import pytest
import torch

from packed_fakes import FakeDataset, FakeLoader, FakeModel, VIDEOS, _opt
from rvdd_release_amd import validate
from rvdd_release_amd.data.packed import PackedLoader, plan_packs, split_videos


def _video(ds, i):
    return os.path.dirname(ds.videos_gt_path[ds.where[i] + 1])


def test_split_videos_reads_index_only(tmp_path):
    ds = FakeDataset(str(tmp_path))
    vids = split_videos(ds, len(ds))
    assert [len(v) for v in vids] == [f - 1 for f, _, _ in VIDEOS.values()]
    assert ds.loads == 0


@pytest.mark.parametrize("B", [2, 3, 4, 8])
def test_plan_every_sample_once_and_first_of_video(tmp_path, B):
    ds = FakeDataset(str(tmp_path))
    loader = PackedLoader(FakeLoader(ds), B)
    seen = []
    for pack in loader.packs:
        slot_video = {}
        for row in pack:
            assert len(row) == B
            for b, (i, first, live) in enumerate(row):
                if not live:
                    continue
                seen.append(i)
                # FirstOfVideo exactly on a video's first sample in its slot
                assert first == (slot_video.get(b) != _video(ds, i))
                if first:
                    assert i == 0 or _video(ds, i - 1) != _video(ds, i)
                slot_video[b] = _video(ds, i)
    assert sorted(seen) == list(range(len(ds)))
    # one frame size per pack
    for pack in loader.packs:
        assert len({ds.size[ds.where[i] + 1] for row in pack for i, _, _ in row}) == 1


def test_plan_refill_order_and_tail():
    # four videos of one size, lengths 3, 1, 2, 2, through two slots
    videos = [[0, 1, 2], [3], [4, 5], [6, 7]]
    (pack,) = plan_packs(videos, [(4, 4)] * 4, 2)
    assert pack == [
        [(0, True, True), (3, True, True)],
        [(1, False, True), (4, True, True)],          # slot 1 refilled from the next unstarted video
        [(2, False, True), (5, False, True)],
        [(6, True, True), (5, False, False)],         # slot 1: nothing left -- repeats its last sample, not live
        [(7, False, True), (5, False, False)],
    ]


def test_plan_more_slots_than_videos_and_sizes():
    videos = [[0, 1], [2], [3, 4, 5]]
    packs = plan_packs(videos, [(4, 4), (2, 2), (4, 4)], 3)
    assert len(packs) == 2
    a, b = packs
    assert a == [[(0, True, True), (3, True, True), (0, True, False)],
                 [(1, False, True), (4, False, True), (0, False, False)],
                 [(1, False, False), (5, False, True), (0, False, False)]]
    assert b == [[(2, True, True), (2, True, False), (2, True, False)]]


def test_max_dataset_size_selects_serial_samples(tmp_path):
    ds = FakeDataset(str(tmp_path))
    loader = PackedLoader(FakeLoader(ds, max_dataset_size=9), 3)
    got = sorted(i for data in loader for i, live in zip(data['index'], data['live'].tolist()) if live)
    assert got == list(range(9))


def test_batched_dicts(tmp_path):
    ds = FakeDataset(str(tmp_path))
    data = next(iter(PackedLoader(FakeLoader(ds), 3)))
    assert data['n'].shape == (3, 8, 4, 6) and data['gt'].shape == (3, 6, 8, 12) and data['flow'].shape == (3, 1, 2, 4, 6)
    assert data['FirstOfVideo'].dtype == torch.bool and data['FirstOfVideo'].tolist() == [True] * 3
    assert data['live'].tolist() == [True] * 3
    assert len(data['n_path']) == 3 and len(data['gt_path']) == 3
    assert [os.path.basename(os.path.dirname(p)) for p in data['gt_path']] == ["000", "001", "003"]


def _run(tmp_path, tag, batch_size, max_size=float("inf")):
    ds = FakeDataset(str(tmp_path / "data"))
    out = tmp_path / tag
    seen = {}
    res = validate.compute_validation(FakeModel(), FakeLoader(ds, max_size), _opt(), val_image_dir=str(out),
                                      batch_size=batch_size,
                                      on_frame=lambda i, d, vis, losses: seen.setdefault(i, vis['denoised'].clone()))
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    return res, (out / "output.log").read_bytes(), files, seen


@pytest.mark.parametrize("B", [2, 3, 5])
def test_packed_validation_equals_serial(tmp_path, B):
    want = _run(tmp_path, "serial", 1)
    got = _run(tmp_path, f"packed{B}", B)
    assert got[0] == want[0]              # returned dict, float for float
    assert got[1] == want[1]              # output.log bytes: serial order
    assert got[2] == want[2]              # written file names
    assert sorted(got[3]) == sorted(want[3])
    for i in want[3]:
        assert torch.equal(got[3][i], want[3][i]), i
    tifs = [f for f in want[2] if f.endswith("_denoised.tif")]
    assert len(tifs) == sum(f - 1 for f, _, _ in VIDEOS.values())
    for f in tifs:
        assert (tmp_path / f"packed{B}" / f).read_bytes() == (tmp_path / "serial" / f).read_bytes(), f


def test_packed_validation_max_dataset_size(tmp_path):
    want = _run(tmp_path, "serial", 1, max_size=10)
    got = _run(tmp_path, "packed", 4, max_size=10)
    assert got[:3] == want[:3]


def test_val_batch_size_flag():
    from rvdd_release_amd.options import make_opt, parse
    assert make_opt().val_batch_size == 1
    assert parse(["--val_batch_size", "4"]).val_batch_size == 4
