"""The stream's reference under test itself, on the CPU: stream_compose.compose() against a stand-in for the handle that records
every call, the traces written out here by hand from the specification in compose()'s docstring, and the ctl words of the schedules
push_schedule() walks."""
import numpy as np
import torch

import stream_compose as S


class Recorder:
    """The stand-alone entry points compose() calls, on the CPU.  Every tensor that comes back is filled with a number of its own,
    under which its name is kept, so that a clone keeps its name; a call is traced as "method name name ..." (None: "-", an unnamed
    tensor of zeros: "zeros")."""

    def __init__(self):
        self.names, self.trace = {}, []

    def new(self, name, *shape):
        self.names[len(self.names) + 1] = name
        return torch.full(shape, float(len(self.names)))

    def name(self, t):
        return "-" if t is None else self.names.get(int(t.reshape(-1)[0]), "zeros")

    def call(self, method, *tensors):
        self.trace.append(" ".join([method] + [self.name(t) for t in tensors]))

    def to_gpu(self, a):
        return torch.from_numpy(a.astype(np.int32))

    def ingest_raw(self, frames, bit_depth, layout):
        t = int(frames[0, 0, 0])                              # frame t of video() holds t
        assert frames.shape[0] == 1 and layout == "mosaic"
        self.trace.append("ingest_raw f%d" % t)
        hh, ww = frames.shape[1] // 2, frames.shape[2] // 2
        return self.new("p%d" % t, 1, 4, hh, ww), self.new("g%d" % t, 1, hh, ww)

    def dpc_map_apply(self, p, bit_depth, gray=None):
        self.call("dpc_map_apply", p, gray)
        return p

    def dpc(self, p, cfg, bit_depth, gray=None):
        self.call("dpc", p, gray)
        return self.new("dpc(%s)" % self.name(p), *p.shape)

    def match_raw(self, p, cfg):
        self.call("match_raw", p)
        return self.new("match(%s)" % self.name(p), *p.shape)

    def tvl1flow_batch(self, a, b):
        self.call("tvl1flow_batch", a, b)
        return self.new("flow(%s,%s)" % (self.name(a), self.name(b)), 1, 2, *a.shape[1:])

    def gray_of_rgb(self, x, bit_depth):
        self.call("gray_of_rgb", x)
        return self.new("gray(%s)" % self.name(x), 1, x.shape[2] // 2, x.shape[3] // 2)

    def reset(self):
        self.trace.append("reset")

    def step(self, prev, cur, nxt, fp, fn):
        for f in (fp, fn):                                    # a zero flow is sized from the ingested planes
            assert f is None or (tuple(f.shape) == (1, 2) + tuple(cur.shape[2:]) and f.dtype == torch.float32)
        self.call("step", prev, cur, nxt, fp, fn)
        return self.new("out%d" % sum(t.startswith("step") for t in self.trace), 1, 3, 2 * cur.shape[2], 2 * cur.shape[3])

    def unmatch_rgb(self, x, cfg):
        self.call("unmatch_rgb", x)
        return self.new("unmatch(%s)" % self.name(x), *x.shape)


def video(N):
    return np.stack([np.full((4, 6), t, np.uint16) for t in range(N)])


def traced(N, future, **kw):
    rt = Recorder()
    outs = S.compose(rt, video(N), future, to_gpu=rt.to_gpu, **kw)
    return rt.trace, [rt.name(o) for o in outs]


INGEST4 = ["ingest_raw f0", "ingest_raw f1", "ingest_raw f2", "ingest_raw f3"]


def test_plain():
    assert traced(4, 0) == (INGEST4 + [
        "tvl1flow_batch g1 g0", "reset", "step p0 p1 - flow(g1,g0) -",
        "tvl1flow_batch g2 g1", "step p1 p2 - flow(g2,g1) -",
        "tvl1flow_batch g3 g2", "step p2 p3 - flow(g3,g2) -"], ["out1", "out2", "out3"])


def test_all_frames_with_a_future_frame():
    assert traced(4, 1, all_frames=True) == (INGEST4 + [
        "tvl1flow_batch g0 g1", "reset", "step p0 p0 p1 zeros flow(g0,g1)",                                   # the head
        "tvl1flow_batch g1 g0", "tvl1flow_batch g1 g2", "reset", "step p0 p1 p2 flow(g1,g0) flow(g1,g2)",     # reset again at c = 1
        "tvl1flow_batch g2 g1", "tvl1flow_batch g2 g3", "step p1 p2 p3 flow(g2,g1) flow(g2,g3)",
        "tvl1flow_batch g3 g2", "step p2 p3 p3 flow(g3,g2) zeros"], ["out1", "out2", "out3", "out4"])        # the tail
    # without the option the same video gives the two centres between them, the first behind one reset
    assert traced(4, 1) == (INGEST4 + [
        "tvl1flow_batch g1 g0", "tvl1flow_batch g1 g2", "reset", "step p0 p1 p2 flow(g1,g0) flow(g1,g2)",
        "tvl1flow_batch g2 g1", "tvl1flow_batch g2 g3", "step p1 p2 p3 flow(g2,g1) flow(g2,g3)"], ["out1", "out2"])


def test_head_and_tail_in_one_step():
    assert traced(1, 1, all_frames=True) == (["ingest_raw f0", "reset", "step p0 p0 p0 zeros zeros"], ["out1"])
    assert traced(1, 0, all_frames=True) == (["ingest_raw f0", "reset", "step p0 p0 - zeros -"], ["out1"])
    assert traced(1, 0) == (["ingest_raw f0"], [])


def test_from_denoised_takes_the_previous_output_from_the_second_centre_on():
    assert traced(4, 0, from_denoised=True) == (INGEST4 + [
        "tvl1flow_batch g1 g0", "reset", "step p0 p1 - flow(g1,g0) -",
        "gray_of_rgb out1", "tvl1flow_batch g2 gray(out1)", "step p1 p2 - flow(g2,gray(out1)) -",
        "gray_of_rgb out2", "tvl1flow_batch g3 gray(out2)", "step p2 p3 - flow(g3,gray(out2)) -"], ["out1", "out2", "out3"])
    # with all_frames never the head's output: c = 1 still takes the noisy pair
    trace, _ = traced(3, 0, from_denoised=True, all_frames=True)
    assert trace[3:] == ["reset", "step p0 p0 - zeros -",
                         "tvl1flow_batch g1 g0", "reset", "step p0 p1 - flow(g1,g0) -",
                         "gray_of_rgb out2", "tvl1flow_batch g2 gray(out2)", "step p1 p2 - flow(g2,gray(out2)) -"]


def test_stages_in_their_order_and_every_output_mapped_back():
    m = ["match(dpc(p%d))" % t for t in range(3)]
    want = []
    for t in range(3):
        want += ["ingest_raw f%d" % t, "dpc_map_apply p%d g%d" % (t, t), "dpc p%d g%d" % (t, t), "match_raw dpc(p%d)" % t]
    want += ["tvl1flow_batch g0 g1", "reset", "step %s %s %s zeros flow(g0,g1)" % (m[0], m[0], m[1]), "unmatch_rgb out1",
             "tvl1flow_batch g1 g0", "tvl1flow_batch g1 g2", "reset", "step %s %s %s flow(g1,g0) flow(g1,g2)" % (m[0], m[1], m[2]), "unmatch_rgb out2",
             "tvl1flow_batch g2 g1", "step %s %s %s flow(g2,g1) zeros" % (m[1], m[2], m[2]), "unmatch_rgb out3"]      # the gray planes: the sensor's
    assert traced(3, 1, all_frames=True, dmap=True, dpc="rule", match="map") == (want, ["unmatch(out1)", "unmatch(out2)", "unmatch(out3)"])
    # the unmapped gray plane of the unmapped output
    trace, _ = traced(3, 0, match="map", from_denoised=True)
    assert trace[-5:] == ["unmatch_rgb out1", "gray_of_rgb unmatch(out1)", "tvl1flow_batch g2 gray(unmatch(out1))",
                          "step match(p1) match(p2) - flow(g2,gray(unmatch(out1))) -", "unmatch_rgb out2"]


def test_no_warp_has_no_flow_at_all():
    ingest = ["ingest_raw f0", "ingest_raw f1", "ingest_raw f2"]
    assert traced(3, 0, no_warp=True, all_frames=True) == (
        ingest + ["reset", "step p0 p0 - - -", "reset", "step p0 p1 - - -", "step p1 p2 - - -"], ["out1", "out2", "out3"])
    assert traced(3, 1, no_warp=True, all_frames=True) == (
        ingest + ["reset", "step p0 p0 p1 - -", "reset", "step p0 p1 p2 - -", "step p1 p2 p2 - -"], ["out1", "out2", "out3"])


def test_reset_each():
    assert traced(3, 0, reset_each=True) == (["ingest_raw f0", "ingest_raw f1", "ingest_raw f2",
                                              "tvl1flow_batch g1 g0", "reset", "step p0 p1 - flow(g1,g0) -",
                                              "tvl1flow_batch g2 g1", "reset", "step p1 p2 - flow(g2,g1) -"], ["out1", "out2"])


# ---- the pushes -------------------------------------------------------------------------------------------------------------------
class Pusher:
    """rvdd_video_push's bookkeeping without the option "stream_all_frames" and without a future frame: a slot's second frame is its
    first output.  Records (ctl, the frame each live slot got) per push; an output holds 100 * slot + the frame it came from."""

    def __init__(self, B):
        self.seen, self.pushes = [0] * B, []

    def video_push(self, frames, ctl, bit_depth, layout, container=None):
        assert container is None and layout == "mosaic" and frames.dtype == torch.int16
        self.pushes.append((list(ctl), [int(frames[s, 0, 0]) if c != S.IDLE else None for s, c in enumerate(ctl)]))
        self.seen = [0 if c == S.IDLE else 1 if c == S.FIRST else n + 1 for c, n in zip(ctl, self.seen)]
        out = torch.stack([torch.full((3, 2, 2), 100.0 * s + int(frames[s, 0, 0])) for s in range(len(ctl))])
        return out, [n >= 2 for n in self.seen]


def _videos(lengths):
    """video v, frame k: every sample 10 v + k"""
    return [np.stack([np.full((2, 2), 10 * v + k, np.uint16) for k in range(n)]) for v, n in enumerate(lengths)]


def _pushed(monkeypatch, steps, lengths):
    monkeypatch.setattr(S.stream_ref, "to_gpu", lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)))
    rt = Pusher(len(steps[0]))
    return rt, S.push_schedule(rt, _videos(lengths), steps)


def test_two_slot_schedule(monkeypatch):
    F, N, I = S.FIRST, S.NEXT, S.IDLE
    assert (N, F, I) == (0, 1, 2)                             # enum rvdd_video_ctl
    lengths = (3, 3, 2)
    steps = S.two_slot_schedule(_videos(lengths))
    rt, got = _pushed(monkeypatch, steps, lengths)
    assert rt.pushes == [([F, F], [0, 10]), ([N, N], [1, 11]), ([N, N], [2, 12]), ([I, I], [None, None]),
                         ([F, I], [20, None]), ([N, I], [21, None]), ([I, I], [None, None])]
    assert got.flags == [[False, False], [True, True], [True, True], [False, False], [False, False], [True, False], [False, False]]
    vals = lambda outs: [float(o[0, 0, 0, 0]) for o in outs]
    assert all(o.shape == (1, 3, 2, 2) for o in got.by_slot[0])
    assert vals(got.by_slot[0]) == [1, 2, 21] and vals(got.by_slot[1]) == [111, 112]
    assert [vals(got.by_video[v]) for v in range(3)] == [[1, 2], [111, 112], [21]]


def test_dealt_schedule_and_one_video_alone(monkeypatch):
    from rvdd_release_amd.denoise import deal_slots
    F, N, I = S.FIRST, S.NEXT, S.IDLE
    lengths = (3, 1, 2)
    calls = []
    rt, got = _pushed(monkeypatch, deal_slots(lengths, 2), lengths)
    assert rt.pushes == [([F, F], [0, 10]), ([N, F], [1, 20]), ([N, N], [2, 21])]
    assert got.flags == [[False, False], [True, False], [True, True]]
    assert [[float(o[0, 0, 0, 0]) for o in got.by_video[v]] for v in range(3)] == [[1, 2], [], [121]]
    # the tail of "stream_all_frames": the slot sits out the push behind its video's last frame, (IDLE, v, N), and gets no frame
    rt, got = _pushed(monkeypatch, deal_slots(lengths, 2, tail=1), lengths)
    assert rt.pushes == [([F, F], [0, 10]), ([N, I], [1, None]), ([N, F], [2, 20]), ([I, N], [None, 21]), ([I, I], [None, None])]
    # the hooks: before and behind every push
    S.push_schedule(Pusher(2), _videos(lengths), deal_slots(lengths, 2), between=lambda i, frames: calls.append(("before", i, tuple(frames.shape))),
                    after=lambda i, out: calls.append(("behind", i, tuple(out.shape))))
    assert calls == [(w, i, s) for i in range(3) for w, s in (("before", (2, 2, 2)), ("behind", (2, 3, 2, 2)))]
    # one video through one slot: FIRST, NEXT ..., and one IDLE only with a future frame and where it is asked for
    for future, idle, ctls in ((0, False, [F, N, N]), (1, False, [F, N, N]), (1, True, [F, N, N, I]), (0, True, [F, N, N])):
        rt = Pusher(1)
        outs, flags = S.push_alone(rt, _videos((3,))[0], future, idle=idle)
        assert [c for (c,), _ in rt.pushes] == ctls and flags == [False, True, True, False][:len(ctls)] and len(outs) == 2
