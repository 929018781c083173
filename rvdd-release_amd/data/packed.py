"""Videos of any length packed into the B slots of one batch (`compute_validation(..., batch_size=B)`).

The runtime is fast when B sequences move in lockstep; a validation set is videos of different lengths.  `PackedLoader`
assigns videos to slots in dataset order and, when a slot's video ends, refills the slot from the next video that has not
started; the model restarts only that slot (`FirstOfVideo` per slot -> `RvddRuntime.reset(slots=...)`).  A sequence's
outputs do not depend on its slot or on what the other slots hold, so every frame is what the serial loader (B = 1) gives.

* Videos are what `validate.py` calls one: maximal runs of consecutive samples whose `dirname(gt_path)` is the same, read
  from the dataset's path index (`where`, `videos_gt_path`, `patch_depth`) without loading a frame.
* Videos of different frame sizes go to different packs (one runtime per size, as `runtime_for` keeps them), packs in
  the order their size first appears.  The size of a video is read from its first sample (`frame_size`), once per video.
* When no video is left for a slot, it repeats its last real sample with `live = False`: its output is to be discarded.
  (A slot that never got a video repeats the pack's first sample.)  Never zeros: an all-zero frame is no input the
  runtime's tests cover.
* `max_dataset_size` selects exactly the samples the serial loader yields: indices 0 .. len(loader) - 1.

Each step yields {'n', 'gt', 'flow': [B, ...], 'n_path', 'gt_path': B-lists, 'FirstOfVideo', 'live': [B] bool tensors,
'index': B-list of dataset indices}.

`compact=True` removes the tail: a step holds only live sequences, always in slots 0 .. n-1 (n <= B), and the runtime steps
those alone (`RvddRuntime.step(live=n)`).  While videos are left, a finished slot is refilled as above; once none is left,
the hole is filled by MOVING the highest live slot into it (`RvddRuntime.move_slots`), so the live slots stay a prefix.
Each step then yields the keys above with leading dimension n ('live' all true), and 'slots': B, 'moves': [(from, to)] to
apply before the step, 'prev_index': for every sequence its index in the previous step's batch (-1 on a first frame).
"""
from __future__ import annotations

import os
from typing import Dict, List, Tuple

import torch


def sample_video_key(dataset, i: int) -> str:
    """dirname(gt_path) of sample i (validate.py's video boundary) from the path index, without loading the sample."""
    if hasattr(dataset, "where") and hasattr(dataset, "videos_gt_path"):
        return os.path.dirname(dataset.videos_gt_path[dataset.where[i] + dataset.patch_depth - 1])
    return os.path.dirname(dataset[i]['gt_path'])


def frame_size(dataset, i: int) -> Tuple[int, ...]:
    """The packed raw size (h, w) of sample i (dataset.sample_size(i) where the dataset has one, else its 'n' tensor)."""
    if hasattr(dataset, "sample_size"):
        return tuple(dataset.sample_size(i))
    return tuple(dataset[i]['n'].shape[-2:])


def split_videos(dataset, count: int) -> List[List[int]]:
    """Sample indices 0 .. count-1 as runs of one video each, in dataset order."""
    videos, prev = [], None
    for i in range(count):
        key = sample_video_key(dataset, i)
        if key != prev:
            videos.append([])
            prev = key
        videos[-1].append(i)
    return videos


class CompactStep(list):
    """A step of a compact plan: n <= B entries (sample index, FirstOfVideo, True) for slots 0 .. n-1, plus `moves`
    [(from slot, to slot)] to apply before it and `prev_index` (each entry's index in the previous step, -1 = first frame)."""

    def __init__(self, entries, moves, prev_index):
        super().__init__(entries)
        self.moves = list(moves)
        self.prev_index = list(prev_index)


def _plan_compact(vids: List[List[int]], batch: int) -> List[CompactStep]:
    queue = list(vids)
    cur: List[List[int]] = []            # remaining samples of the video in each used slot; the live ones are a prefix
    steps = []
    while True:
        prev = list(range(len(cur)))     # where each slot's sequence sat in the last step
        for b in range(batch):
            if b < len(cur) and cur[b]:
                continue
            if not queue:
                continue
            if b == len(cur):
                cur.append([])
                prev.append(-1)
            elif b > len(cur):
                break
            cur[b] = list(queue.pop(0))  # a video that has not started: assigned to the hole, no move
            prev[b] = -1
        # no video left for the remaining holes: the highest live slot moves into the lowest hole (two pointers)
        moves = []
        lo, hi = 0, len(cur) - 1
        while True:
            while lo < len(cur) and cur[lo]:
                lo += 1
            while hi >= 0 and not cur[hi]:
                hi -= 1
            if lo >= hi:
                break
            moves.append((hi, lo))
            cur[lo], cur[hi] = cur[hi], []
            prev[lo] = prev[hi]
        n = hi + 1
        del cur[n:], prev[n:]
        if n == 0:
            break
        steps.append(CompactStep([(cur[b].pop(0), prev[b] < 0, True) for b in range(n)], moves, prev))
    return steps


def plan_packs(videos: List[List[int]], sizes: List[Tuple[int, ...]], batch: int, compact: bool = False):
    """-> packs, each a list of steps, each step B entries (sample index, FirstOfVideo, live).  Pure bookkeeping.
    `compact`: each step a `CompactStep` of its live entries only (see the module's text)."""
    if batch < 1:
        raise ValueError("batch must be >= 1")
    groups: Dict[Tuple[int, ...], List[List[int]]] = {}
    for v, s in zip(videos, sizes):
        groups.setdefault(s, []).append(v)
    if compact:
        return [_plan_compact(vids, batch) for vids in groups.values()]
    packs = []
    for vids in groups.values():
        queue = list(vids)
        cur: List[List[int]] = [[] for _ in range(batch)]       # remaining samples of each slot's video
        last: List[int] = [-1] * batch                          # last real sample of each slot
        steps = []
        while True:
            row = []
            for b in range(batch):
                first = False
                if not cur[b] and queue:
                    cur[b] = list(queue.pop(0))
                    first = True
                if cur[b]:
                    i = cur[b].pop(0)
                    last[b] = i
                    row.append((i, first, True))
                else:
                    row.append((last[b], False, False))
            if not any(live for _, _, live in row):
                break
            steps.append(row)
        # a slot that never got a video: the pack's first sample, latched on the first step and repeated after it
        filler = steps[0][0][0]
        for k, row in enumerate(steps):
            for b, (i, first, live) in enumerate(row):
                if i < 0:
                    row[b] = (filler, k == 0, False)
        packs.append(steps)
    return packs


def _stack(values):
    if all(torch.is_tensor(v) for v in values):
        return torch.stack(values)
    if all(isinstance(v, str) for v in values):
        return list(values)
    return values[0]            # e.g. the empty flow list of a --no_warp dataset


class PackedLoader:
    """Batched steps over videos packed into `batch` slots; `loader` = the serial loader (`create_dataset(opt)`)."""

    def __init__(self, loader, batch: int, compact: bool = False):
        self.loader = loader
        self.dataset = loader.dataset
        self.batch = int(batch)
        self.compact = bool(compact)
        count = len(loader)
        videos = split_videos(self.dataset, count)
        sizes = [frame_size(self.dataset, v[0]) for v in videos]
        self.packs = plan_packs(videos, sizes, self.batch, compact=self.compact)
        self.samples = count

    def __len__(self):
        return self.samples

    def steps(self) -> int:
        return sum(len(p) for p in self.packs)

    def tail_waste(self) -> int:
        """Slot-steps whose output is discarded."""
        return sum(not live for p in self.packs for row in p for _, _, live in row)

    def moves(self) -> int:
        """Slot moves of a compact plan (0 otherwise)."""
        return sum(len(getattr(row, 'moves', ())) for p in self.packs for row in p)

    def _iter_compact(self):
        for steps in self.packs:
            for row in steps:
                samples = [self.dataset[i] for i, _, _ in row]      # every entry is a new frame: nothing to hold
                out = {k: _stack([s[k] for s in samples]) for k in samples[0]}
                out['FirstOfVideo'] = torch.tensor([first for _, first, _ in row], dtype=torch.bool)
                out['live'] = torch.ones(len(row), dtype=torch.bool)
                out['index'] = [i for i, _, _ in row]
                out['slots'] = self.batch
                out['moves'] = list(row.moves)
                out['prev_index'] = list(row.prev_index)
                yield out

    def __iter__(self):
        if self.compact:
            yield from self._iter_compact()
            return
        for steps in self.packs:
            held: Dict[int, dict] = {}           # slot -> its last sample (a repeat costs no load)
            for row in steps:
                samples = []
                for b, (i, first, live) in enumerate(row):
                    if b not in held or held[b]['_index'] != i:
                        held[b] = dict(self.dataset[i], _index=i)
                    samples.append(held[b])
                out = {k: _stack([s[k] for s in samples]) for k in samples[0] if k != '_index'}
                out['FirstOfVideo'] = torch.tensor([first for _, first, _ in row], dtype=torch.bool)
                out['live'] = torch.tensor([live for _, _, live in row], dtype=torch.bool)
                out['index'] = [i for i, _, _ in row]
                yield out
