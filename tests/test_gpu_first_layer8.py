"""The composed first layer over the 8 live input channels (conv3x3h.hip HGeo<8, 1, 5>: 25 one-group taps in 7 chunks of K,
option "pre5_cin8", the default without a future frame) against its 13-chunk form over all 16 channels of the pixel
(pre5_cin8 = 0) and against the CPU oracle.  Needs a real MI355X: -m gpu.

Tolerances: 7 against 13 chunks is the same linear map with K grouped differently -- the bars
test_gpu_parity.py::test_composed_first_layer_matches_two_convs uses for "the same map in another summation order" (5e-6 on
frames, 3e-5 on the features, which reach 8); against the oracle the project's 1e-4 of the frame's own max-abs."""
import functools

import pytest
import torch

import rvdd_oracle as O
from conftest import load_weights

pytestmark = pytest.mark.gpu

STEM, STEM_FUT = "recurrent-convunet+feat-iso3200", "recurrent-convunet+feat-future-iso12800"


@functools.lru_cache(maxsize=None)
def _weights(stem):
    return load_weights(stem)


@functools.lru_cache(maxsize=None)
def _sequences(B, H, W, T, seed0=8100):
    from rvdd_release_amd import synth
    return tuple(synth.make_sequence(T, H, W, iso=3200, seed=seed0 + b, device="cuda") for b in range(B))


def _run(seqs, H, W, steps, cin8, stem=STEM, fut=0, mag=1.0, profile=False):
    """`steps` recurrent steps of the sequences side by side -> (frames per step, final features, profile rows)."""
    from rvdd_release_amd.runtime import RvddRuntime
    st = lambda f: torch.stack([f(s) for s in seqs], 0)
    rt = RvddRuntime("convunet+feat", fut, len(seqs), H, W, 0)
    rt.set_option("pre5_cin8", cin8)
    rt.load_state_dict(_weights(stem))
    if profile:
        rt.profile_select(None, 1)
        rt.profile_enable(True)
    frames = []
    for t in range(1, steps + 1):
        frames.append(rt.step(st(lambda s: s.raw[t - 1] * mag) if t == 1 else None, st(lambda s: s.raw[t] * mag),
                              st(lambda s: s.raw[t + 1] * mag) if fut else None, st(lambda s: s.flow_prev[t]),
                              st(lambda s: s.flow_next[t]) if fut else None).clone())
    feat = rt.get_state()[1].clone()
    rows = rt.profile_read() if profile else None
    rt.close()
    return frames, feat, rows


def _oracle(seq, steps, mag=1.0, fut=0, stem=STEM):
    n = steps + 1 + fut      # frames the steps read
    return O.RecurrentOracle(_weights(stem), future=fut).run_sequence((seq.raw[:n] * mag).cpu(), seq.flow_prev[:n].cpu(),
                                                                      seq.flow_next[:n].cpu() if fut else None)


# one tile, every pixel on the border ring; ragged tiles; 572 tiles: every workgroup of a 256-CU launch walks at least two, so the
# next-tile prefetch and the XCD-partitioned walk run
@pytest.mark.parametrize("B,H,W", [(1, 16, 16), (3, 50, 66), (2, 208, 352)])
def test_seven_chunks_match_thirteen(B, H, W):
    seqs = _sequences(B, H, W, 4)
    f8, s8, _ = _run(seqs, H, W, 3, 1)
    f16, s16, _ = _run(seqs, H, W, 3, 0)
    for k, (a, b) in enumerate(zip(f8 + [s8], f16 + [s16])):
        d = float((a - b).abs().max())
        bar = 3e-5 if k == 3 else 5e-6
        print(f"[first_layer8] {B}x{H}x{W} {'features' if k == 3 else 'frame %d' % k}: max|7 - 13 chunks| = {d:.3e} (bar {bar:.0e})")
        assert torch.isfinite(a).all() and d < bar, (B, H, W, k, d)


def test_against_the_oracle_many_tiles():
    B, H, W = 2, 208, 352
    seqs = _sequences(B, H, W, 4)
    frames, _, _ = _run(seqs, H, W, 2, 1)
    for b in range(B):
        for t, ref in enumerate(_oracle(seqs[b], 2)):
            scale, err = float(ref.abs().max()), float((frames[t][b].cpu() - ref).abs().max())
            print(f"[first_layer8] oracle {H}x{W} seq {b} frame {t}: err {err:.3e}, frame max-abs {scale:.3e}")
            assert err < 1e-4 * scale, (b, t, err, scale)


@pytest.mark.parametrize("mag", [2.0 ** -12, 1e5])
def test_scaled_loop_form_against_the_oracle(mag):
    """Frames outside [2^-6, 2^12): the tile loop's block-floating-point form (the per-tile power of two in the split)."""
    H, W = 48, 80
    seqs = _sequences(1, H, W, 4)
    frames, _, _ = _run(seqs, H, W, 2, 1, mag=mag)
    for t, ref in enumerate(_oracle(seqs[0], 2, mag=mag)):
        got = frames[t][0].cpu()
        assert torch.isfinite(got).all(), (mag, t)
        scale, err = float(ref.abs().max()), float((got - ref).abs().max())
        print(f"[first_layer8] mag {mag:g} frame {t}: err {err:.3e}, frame max-abs {scale:.3e}")
        assert err < 1e-4 * scale, (mag, t, err, scale)


def test_two_runs_same_bits_and_slot_placement():
    B, H, W = 3, 50, 66
    seqs = _sequences(B, H, W, 4)
    fa, sa, _ = _run(seqs, H, W, 3, 1)
    fb, sb, _ = _run(seqs, H, W, 3, 1)
    for a, b in zip(fa + [sa], fb + [sb]):
        assert torch.equal(a, b)
    # the same sequence in slot 0 and in slot 2
    fc, sc, _ = _run((seqs[0], seqs[1], seqs[0]), H, W, 3, 1)
    for a in fc + [sc]:
        assert torch.equal(a[0], a[2])
    for a, c in zip(fa + [sa], fc + [sc]):
        assert torch.equal(a[0], c[0])


def _launches(rows):
    return {r["name"]: r["launches"] for r in rows if r["name"].startswith("conv5x5h_kernel")}


def test_dispatch_follows_channels_and_option():
    H, W = 50, 66
    seqs = _sequences(1, H, W, 5)
    _, _, rows = _run(seqs, H, W, 3, 1, profile=True)
    assert _launches(rows) == {"conv5x5h_kernel<8>": 3}, _launches(rows)
    _, _, rows = _run(seqs, H, W, 3, 0, profile=True)
    assert _launches(rows) == {"conv5x5h_kernel<16>": 3}, _launches(rows)
    # a future frame makes 9 channels: the 13-chunk form whatever the option says, and the option changes no bit
    outs = []
    for cin8 in (1, 0):
        f, s, rows = _run(seqs, H, W, 3, cin8, stem=STEM_FUT, fut=1, profile=True)
        assert _launches(rows) == {"conv5x5h_kernel<16>": 3}, (cin8, _launches(rows))
        outs.append(f + [s])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
