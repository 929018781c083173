"""The random-weight helper (tests/random_weights.py) and the reference it is used with, on the CPU: shapes, determinism, and
that the f32 oracle under these weights is live, finite and within 5e-6 of its own f64 run -- the condition that keeps the
bound of tests/test_gpu_random_weights.py (R * e_ref, R <= 8) meaningful."""
import pytest
import torch

import rvdd_oracle as O
import random_weights as RW
from conftest import load_weights

STEMS = ["recurrent-convunet-iso3200", "recurrent-convunet-future-iso3200", "recurrent-convunet+feat-iso3200",
         "recurrent-convunet+feat-future-iso12800", "recurrent-ConvNeXtUnet-iso3200",
         "recurrent-ConvNeXtUnet+feat-future-iso3200"]
# one stem of each architecture with and without a future frame (the shapes do not depend on the ISO)
SHAPE_STEMS = STEMS + ["recurrent-ConvNeXtUnet-iso12800", "recurrent-ConvNeXtUnet+feat-future-iso12800",
                       "recurrent-convunet+feat-future-iso3200", "recurrent-convunet-future-iso12800"]


@pytest.mark.parametrize("profile", ["he", "pow2"])
@pytest.mark.parametrize("stem", SHAPE_STEMS)
def test_keys_and_shapes_are_the_checkpoints(stem, profile):
    want = load_weights(stem)
    got = RW.random_state_dict(stem, 3, profile)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].shape == v.shape and got[k].dtype == torch.float32, k
        assert torch.isfinite(got[k]).all(), k


@pytest.mark.parametrize("profile", ["he", "pow2"])
@pytest.mark.parametrize("stem", ["recurrent-convunet+feat-iso3200", "recurrent-ConvNeXtUnet+feat-future-iso3200"])
def test_same_seed_same_tensors(stem, profile):
    a, b, c = (RW.random_state_dict(stem, s, profile) for s in (11, 11, 12))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert all(not torch.equal(a[k], c[k]) for k in a if a[k].abs().max() > 0)


def test_pow2_profiles_hit_the_edges_they_are_for():
    """fc1 * 2^k moves the ConvBlock's power of two s1 = floor(log2(1 / max|w|)) to -k (+0/1): beyond 15 for |k| = 17, at
    14 or 15 for |k| = 14; the two LayerNorm blocks break 6.86 |ln_w| < 32768; the zero layers are zero."""
    import math
    he = RW.random_state_dict(STEMS[5], 1, "he")
    p2 = RW.random_state_dict(STEMS[5], 1, "pow2")
    seen = set()
    for bi, b in enumerate(RW.NEXT_BLOCKS):
        k = RW.NEXT_K[bi % 7]
        if b == RW.NEXT_FC1_ZERO:
            assert p2[b + ".block.2.weight"].abs().max() == 0
            continue
        s1 = math.floor(math.log2(1.0 / float(p2[b + ".block.2.weight"].abs().max())))
        s0 = math.floor(math.log2(1.0 / float(he[b + ".block.2.weight"].abs().max())))
        assert s1 == s0 - k and s0 in (-1, 0, 1), (b, s0, s1)
        seen.add(abs(s1) > 15)
        if abs(k) == 17:
            assert abs(s1) > 15, (b, s1)
        if abs(k) == 14:
            assert 13 <= abs(s1) <= 15, (b, s1)
    assert seen == {True, False}
    for b in RW.NEXT_LN_BIG:
        assert 6.86 * float(p2[b + ".block.1.weight"].abs().max()) >= 32768.0
    assert "proj.weight" in " ".join(k for k in p2 if k.startswith(RW.NEXT_LN_BIG[1]))
    u = RW.random_state_dict(STEMS[2], 1, "pow2")
    assert u[RW.UNET_ZERO + ".weight"].abs().max() == 0
    assert float(u["EncoderConvs.0.blocks.0.0.weight"].abs().max()) > 2.0 ** 17
    assert float(u["EncoderConvs.1.blocks.0.0.weight"].abs().max()) < 2.0 ** -20


_cache = {}


def _oracle_pair(stem, profile, seed, zero_layers=True):
    key = (stem, profile, seed, zero_layers)
    if key not in _cache:
        sd = RW.random_state_dict(stem, seed, profile, zero_layers)
        x, f = RW.net_inputs(2, O.net_input_nc(sd), 50, 66, 100 + seed, O.net_has_feat(sd))
        with torch.no_grad():
            o32 = O.net_forward(sd, x, f)
            o64 = O.net_forward(RW.to64(sd), x.double(), None if f is None else f.double())
        _cache[key] = (o32, o64)
    return _cache[key]


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("profile", ["he", "pow2"])
@pytest.mark.parametrize("stem", STEMS)
def test_reference_is_live_and_its_f32_noise_is_small(stem, profile, seed):
    o32, o64 = _oracle_pair(stem, profile, seed)
    for a, b, what in zip(o32, o64, ("out", "feat_out")):
        if a is None:
            assert b is None
            continue
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), what
        # live: no map is constant, for either sequence; and most channels of it move (a ReLU may leave a few dead)
        spread = a.flatten(2).max(2).values - a.flatten(2).min(2).values
        live = spread > 1e-3 * a.abs().max()
        assert live.any(1).all() and live.float().mean() >= 0.75, (what, float(live.float().mean()))
        e_ref = RW.rel_err(a, b)
        print(f"{stem} {profile} seed {seed} {what}: max|f64| = {float(b.abs().max()):.3g}, e_ref = {e_ref:.3g}")
        assert e_ref <= 5e-6, (what, e_ref)


@pytest.mark.parametrize("stem", STEMS[:4])
def test_convunet_pow2_is_he_bit_for_bit_in_f64(stem):
    """Scaling a conv (weight and bias) by 2^k and the conv behind it by 2^-k commutes with ReLU and is exact in f64: without
    its zero layer the pow2 profile computes the bits of the he profile."""
    he = _oracle_pair(stem, "he", 1)[1]
    p2 = _oracle_pair(stem, "pow2", 1, zero_layers=False)[1]
    for a, b in zip(he, p2):
        assert (a is None and b is None) or torch.equal(a, b)
