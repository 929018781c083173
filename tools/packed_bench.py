"""Serial vs packed vs compact validation throughput on videos of mixed lengths, one JSON line per configuration.

The loops are compute_validation's at the runtime level, on in-memory synthetic sequences (synth.make_sequence, seeded):
  serial   -- B = 1: per video rvdd_reset, per frame one step and one rvdd_psnr_l1 (its synchronisation included);
              with online flow one synchronous rvdd_tvl1flow per frame after the first (validate.py's
              compute_flows_from_denoised)
  packed   -- B slots, videos assigned in order and a slot refilled when its video ends (data/packed.py's plan), per
              step one reset_slots, one step, one rvdd_psnr_l1_batch; online flow = one asynchronous
              rvdd_tvl1flow_batch over the live slots that continue a video
  compact  -- the same B slots by the compact plan (plan_packs(..., compact=True)): a step covers the live slots only
              (rvdd_step_live), kept in the first slots by rvdd_move_slots once no video is left to refill a finished
              one; no slot-step is discarded
  lockstep -- the same B with B videos of equal length (bench.py's loop plus the per-step losses): the rate packing
              can at best reach
Reported: frames/s of each loop (frames = output frames of live slots), slot-steps/s of packed and lockstep, the
slot-steps wasted on the tail (packed) and discarded by compact, the moves of the compact plan, and whether every packed
and every compact output equals the serial one (torch.equal, an untimed pass); for the largest B also the time of one
rvdd_move_slots launch (one pair, four pairs) and of a step of n = 1 .. B live slots (device events).
Every shape is warmed up; serial, packed, compact and lockstep repetitions alternate; time = wall clock around a
synchronised loop.

  python tools/packed_bench.py [--config C2-256,C2-720p,C2-720p-online,C4-720p] [--reps 3] [--batches 4,8]
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rvdd_release_amd import synth  # noqa: E402
from rvdd_release_amd.data.packed import plan_packs  # noqa: E402
from rvdd_release_amd.runtime import RvddRuntime  # noqa: E402

# name -> (arch, weights stem, future, H, W, online flow)
CONFIGS = {
    "C2-256": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 256, 256, False),
    "C2-720p": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 720, 1280, False),
    "C2-720p-online": ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 720, 1280, True),
    "C4-720p": ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, 720, 1280, False),
}


def moving_target(den, raw_cur):
    """compute_flows_from_denoised's two images per sequence of a batch, formed one sequence at a time as validate.py
    forms them: channel means in [0, 1] of the current raw frame and of remosaick(previous output)."""
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    ha = HamiltonAdam('gbrg')
    tg = [((raw_cur[b] + 1.0) / 2.0).mean(dim=0) for b in range(raw_cur.shape[0])]
    mv = [((ha.remosaick(den[b:b + 1])[0] + 1.0) / 2.0).mean(dim=0) for b in range(den.shape[0])]
    return torch.stack(tg).contiguous(), torch.stack(mv).contiguous()


class Bench:
    def __init__(self, name, lengths, seed):
        arch, stem, fut, H, W, online = CONFIGS[name]
        from safetensors.torch import load_file
        self.sd = load_file(os.path.join(REPO, "weights", stem + ".safetensors"))
        self.arch, self.fut, self.H, self.W, self.online = arch, fut, H, W, online
        self.seqs = [synth.make_sequence(T + fut, H, W, iso=3200, seed=seed + v, device="cuda") for v, T in enumerate(lengths)]
        self.rts = {}

    def rt(self, B):
        if B not in self.rts:
            r = RvddRuntime(self.arch, self.fut, B, self.H, self.W, 0)
            r.load_state_dict(self.sd)
            if self.online and B > 1:
                r.set_option("tvl1_async", 1)
            self.rts[B] = r
        return self.rts[B]

    def frames(self, v):
        return self.seqs[v].raw.shape[0] - self.fut

    def serial(self, keep=None):
        rt, f = self.rt(1), self.fut
        n = 0
        for v, s in enumerate(self.seqs):
            rt.reset()
            out = None
            for t in range(1, self.frames(v)):
                fp = s.flow_prev[t][None]
                if self.online and t > 1:
                    tg, mv = moving_target(out, s.raw[t][None])
                    fp = rt.tvl1flow(tg[0], mv[0])[None]
                out = rt.step(s.raw[t - 1][None], s.raw[t][None], s.raw[t + 1][None] if f else None, fp,
                              s.flow_next[t][None] if f else None)
                rt.psnr_l1(out, s.gt[t][None])
                if keep is not None:
                    keep[(v, t)] = out[0].clone()
                n += 1
        return n

    def plan(self, B, compact=False):
        """-> (steps of data/packed.py's plan, sample index -> (video, t)); one "sample" per output frame."""
        videos, k = [], 0
        for v in range(len(self.seqs)):
            videos.append(list(range(k, k + self.frames(v) - 1)))
            k += self.frames(v) - 1
        where = [(v, t) for v in range(len(self.seqs)) for t in range(1, self.frames(v))]
        (plan,) = plan_packs(videos, [(self.H, self.W)] * len(videos), B, compact=compact)
        return plan, where

    def packed(self, B, check=None):
        """-> (live frames, slot-steps, wasted slot-steps, all equal to `check`)."""
        rt, f = self.rt(B), self.fut
        plan, where = self.plan(B)
        live_n, waste, same = 0, 0, True
        out = None
        for step, row in enumerate(plan):
            vt = [where[i] for i, _, _ in row]
            first = [fi for _, fi, _ in row]
            live = [li for _, _, li in row]
            if step and any(first):
                rt.reset(slots=first)
            elif step == 0:
                rt.reset()
            st = lambda g: torch.stack([g(self.seqs[v], t) for v, t in vt])
            fp = st(lambda s, t: s.flow_prev[t])
            if self.online and step:
                sel = [b for b in range(B) if live[b] and not first[b]]
                if sel:
                    tg, mv = moving_target(out[sel], torch.stack([self.seqs[vt[b][0]].raw[vt[b][1]] for b in sel]))
                    fp[sel] = rt.tvl1flow_batch(tg, mv)
            out = rt.step(st(lambda s, t: s.raw[t - 1]), st(lambda s, t: s.raw[t]), st(lambda s, t: s.raw[t + 1]) if f else None,
                          fp, st(lambda s, t: s.flow_next[t]) if f else None)
            rt.psnr_l1_batch(out, st(lambda s, t: s.gt[t]))
            live_n += sum(live)
            waste += B - sum(live)
            if check is not None:
                same = same and all(torch.equal(out[b], check[vt[b]]) for b in range(B) if live[b])
        return live_n, len(plan) * B, waste, same

    def compact(self, B, check=None):
        """-> (frames, slot-steps, moves, all equal to `check`): compute_validation(..., compact=True)'s loop."""
        rt, f = self.rt(B), self.fut
        plan, where = self.plan(B, compact=True)
        slot_steps, moves, same = 0, 0, True
        out = None
        rt.reset()
        for step, row in enumerate(plan):
            n = len(row)
            vt = [where[i] for i, _, _ in row]
            first = [fi for _, fi, _ in row]
            if row.moves:
                rt.move_slots(row.moves)
                moves += len(row.moves)
            if step and any(first):
                rt.reset(slots=[b for b in range(n) if first[b]])
            st = lambda g: torch.stack([g(self.seqs[v], t) for v, t in vt])
            fp = st(lambda s, t: s.flow_prev[t])
            if self.online and step:
                sel = [b for b in range(n) if not first[b]]
                if sel:      # a moved sequence finds its previous output where it sat in the last step
                    tg, mv = moving_target(out[[row.prev_index[b] for b in sel]],
                                           torch.stack([self.seqs[vt[b][0]].raw[vt[b][1]] for b in sel]))
                    fp[sel] = rt.tvl1flow_batch(tg, mv)
            out = rt.step(st(lambda s, t: s.raw[t - 1]), st(lambda s, t: s.raw[t]), st(lambda s, t: s.raw[t + 1]) if f else None,
                          fp, st(lambda s, t: s.flow_next[t]) if f else None, live=n)
            rt.psnr_l1_batch(out, st(lambda s, t: s.gt[t]))
            slot_steps += n
            if check is not None:
                same = same and all(torch.equal(out[b], check[vt[b]]) for b in range(n))
        return len(where), slot_steps, moves, same

    def move_ms(self, B, pairs, iters=10):
        """Device time of one rvdd_move_slots launch over `pairs`, there and back `iters` times."""
        rt = self.rt(B)
        back = [(t, f) for f, t in pairs]
        rt.move_slots(pairs)
        rt.move_slots(back)
        rt.timer_start()
        for _ in range(iters):
            rt.move_slots(pairs)
            rt.move_slots(back)
        return rt.timer_stop_ms() / (2 * iters)

    def live_step_ms(self, B, T):
        """Device time per step of n = 1 .. B live slots (the equal-length sequences, steps 2 .. T-1 of each run)."""
        rt, f = self.rt(B), self.fut
        res = {}
        for n in range(1, B + 1):
            eq = self.equal[:n]
            st = lambda g: torch.stack([g(s) for s in eq])
            rt.reset()
            for t in range(1, T):
                if t == 2:
                    rt.timer_start()
                rt.step(st(lambda s: s.raw[t - 1]), st(lambda s: s.raw[t]), st(lambda s: s.raw[t + 1]) if f else None,
                        st(lambda s: s.flow_prev[t]), st(lambda s: s.flow_next[t]) if f else None, live=n)
            res[str(n)] = round(rt.timer_stop_ms() / (T - 2), 3)
        return res

    def lockstep(self, B, T):
        """B videos of T frames each (the first B of a second set of equal-length sequences), all in lockstep."""
        rt, f = self.rt(B), self.fut
        eq = self.equal[:B]
        st = lambda g: torch.stack([g(s) for s in eq])
        rt.reset()
        out = None
        for t in range(1, T):
            fp = st(lambda s: s.flow_prev[t])
            if self.online and t > 1:
                tg, mv = moving_target(out, st(lambda s: s.raw[t]))
                fp = rt.tvl1flow_batch(tg, mv)
            out = rt.step(st(lambda s: s.raw[t - 1]), st(lambda s: s.raw[t]), st(lambda s: s.raw[t + 1]) if f else None,
                          fp, st(lambda s: s.flow_next[t]) if f else None)
            rt.psnr_l1_batch(out, st(lambda s: s.gt[t]))
        return B * (T - 1)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=",".join(CONFIGS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="4,8")
    ap.add_argument("--videos", type=int, default=12)
    ap.add_argument("--min-frames", type=int, default=9)
    ap.add_argument("--max-frames", type=int, default=40)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(a.seed)
    lengths = torch.randint(a.min_frames, a.max_frames + 1, (a.videos,), generator=g).tolist()
    batches = [int(b) for b in a.batches.split(",")]
    for name in a.config.split(","):
        bench = Bench(name, lengths, a.seed)
        T_eq = round(sum(lengths) / len(lengths))
        bench.equal = [synth.make_sequence(T_eq + bench.fut, bench.H, bench.W, iso=3200, seed=a.seed + 1000 + b, device="cuda")
                       for b in range(max(batches))]
        # untimed pass: warms up every shape and records the serial outputs the packed ones must equal
        ref = {}
        bench.serial(keep=ref)
        equal, equal_c = {}, {}
        for B in batches:
            equal[B] = bench.packed(B, check=ref)[3]
            equal_c[B] = bench.compact(B, check=ref)[3]
            bench.lockstep(B, T_eq)
        del ref
        ser, pk, ls = [], {B: [] for B in batches}, {B: [] for B in batches}
        cp = {B: [] for B in batches}
        for _ in range(a.reps):                  # alternate: serial, packed B, compact B, lockstep B ...
            n, dt = timed(bench.serial)
            ser.append(n / dt)
            for B in batches:
                (live, slots, waste, _), dt = timed(lambda: bench.packed(B))
                pk[B].append((live / dt, slots / dt, waste))
                (live, slots, moves, _), dt = timed(lambda: bench.compact(B))
                cp[B].append((live / dt, slots - live, moves))
                n, dt = timed(lambda: bench.lockstep(B, T_eq))
                ls[B].append(n / dt)
        med = lambda xs: sorted(xs)[len(xs) // 2]
        res = {"config": name, "arch": bench.arch, "H": bench.H, "W": bench.W, "online_flow": bench.online,
               "videos": len(lengths), "lengths": lengths, "frames": sum(l - 1 for l in lengths), "reps": a.reps,
               "serial_fps": round(med(ser), 1), "serial_fps_all": [round(x, 1) for x in ser]}
        for B in batches:
            res[f"B{B}"] = {
                "packed_fps": round(med([x[0] for x in pk[B]]), 1),
                "packed_fps_all": [round(x[0], 1) for x in pk[B]],
                "packed_slot_steps_per_s": round(med([x[1] for x in pk[B]]), 1),
                "lockstep_fps": round(med(ls[B]), 1),
                "lockstep_fps_all": [round(x, 1) for x in ls[B]],
                "lockstep_T": T_eq,
                "tail_waste_slot_steps": pk[B][0][2],
                "packed_equals_serial": bool(equal[B]),
                "packed_over_serial": round(med([x[0] for x in pk[B]]) / med(ser), 3),
                "packed_slot_rate_over_lockstep": round(med([x[1] for x in pk[B]]) / med(ls[B]), 3),
                "compact_fps": round(med([x[0] for x in cp[B]]), 1),
                "compact_fps_all": [round(x[0], 1) for x in cp[B]],
                "compact_discarded_slot_steps": cp[B][0][1],
                "compact_moves": cp[B][0][2],
                "compact_equals_serial": bool(equal_c[B]),
                "compact_over_serial": round(med([x[0] for x in cp[B]]) / med(ser), 3),
                "compact_over_packed": round(med([x[0] for x in cp[B]]) / med([x[0] for x in pk[B]]), 3),
            }
        Bm = max(batches)
        if Bm >= 2:
            res["move_ms"] = {"B": Bm, "one_pair": round(bench.move_ms(Bm, [(Bm - 1, 0)]), 3)}
            if Bm >= 8:
                res["move_ms"]["four_pairs"] = round(bench.move_ms(Bm, [(Bm - 1 - k, k) for k in range(4)]), 3)
            res["live_step_ms"] = {"B": Bm, "T": T_eq, "by_live": bench.live_step_ms(Bm, T_eq)}
        print(json.dumps(res), flush=True)
        for r in bench.rts.values():
            r.close()
        del bench
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
