"""Dense random weights in the shapes of the trained checkpoints, for the tests that compare the nets with an f64 run of
the oracle (test_random_weights_host.py, test_gpu_random_weights.py).  A helper module: no fixtures, no pytest settings.

Trained weights probe the weight-dependent code weakly (many taps and channels near zero, magnitudes in a narrow band).
Here every tap, channel and bias counts, and the `pow2` profiles move the per-layer powers of two of the split-f16 banks,
the scaled GELU and the split / f32 decision of the ConvBlocks across their whole range while the f64 result of the
convunet stays bit for bit that of the `he` profile.

Draws come from one CPU torch.Generator per call, keys visited in sorted order: the same values on every machine."""
import torch

from conftest import load_weights

# the ConvBlocks in the order of kNxNames (csrc/runtime_internal.h)
NEXT_BLOCKS = (
    "preprocessing_layer.blocks.0", "encoder_convs.0.blocks.0", "encoder_convs.0.blocks.1", "encoder_downs.0.postconv",
    "encoder_convs.1.blocks.0", "encoder_convs.1.blocks.1", "encoder_downs.1.postconv", "encoder_convs.2.blocks.0",
    "encoder_convs.2.blocks.1", "encoder_downs.2.postconv", "encoder_convs.3.blocks.0", "encoder_convs.3.blocks.1",
    "bottleneck.blocks.0", "bottleneck.blocks.1", "decoder_ups.0.postconv", "decoder_convs.0.blocks.0",
    "decoder_convs.0.blocks.1", "decoder_ups.1.postconv", "decoder_convs.1.blocks.0", "decoder_convs.1.blocks.1",
    "decoder_ups.2.postconv", "decoder_convs.2.blocks.0", "decoder_convs.2.blocks.1", "postprocessing.0.blocks.0",
    "postprocessing.0.blocks.1")
NEXT_K = (0, 14, -14, 17, -17, 6, -3)                 # fc1 * 2^k, fc2 * 2^-k: |14| at the edge of |s1| <= 15, |17| beyond it
NEXT_LN_BIG = ("encoder_convs.1.blocks.1",            # LayerNorm weight * 6000, layerscale / 6000: worst_y >= 32768
               "decoder_convs.2.blocks.0")            # ... and one behind a concat (a 96 -> 48 projection in front)
NEXT_FC1_ZERO = "bottleneck.blocks.0"                 # an all-zero fc1: pow2_scale with mx == 0
UNET_K = (20, -20, 11, -7, 3)                         # first conv of a pair * 2^k, second * 2^-k
UNET_PAIRS = tuple((f"{g}.{i}.blocks.0.0", f"{g}.{i}.blocks.1.0")
                   for g, n in (("EncoderConvs", 4), ("DecoderConvs", 3)) for i in range(n))
UNET_ZERO = "EncoderConvs.2.blocks.1.0"               # an all-zero 3x3 bank (mx == 0)

# rel_err(hip, f64) <= R * e_ref per kernel family (test_gpu_random_weights.py has the table and how each value came about)
R_CAP = 8
R = {"split-f16 conv": 8, "direct f32": 6, "Winograd f32": 3, "ConvBlock split": 5, "ConvBlock f32": 3,
     "composed first layer": 8}
assert all(v <= R_CAP for v in R.values())

_shapes = {}


def checkpoint_shapes(stem):
    """{key: shape} of checkpoint `stem` (read once per process)."""
    if stem not in _shapes:
        _shapes[stem] = {k: tuple(v.shape) for k, v in load_weights(stem).items()}
    return _shapes[stem]


def is_next(stem):
    return "ConvNeXt" in stem


def _he(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    sd = {}
    for k in sorted(shapes):
        shp = shapes[k]
        n = torch.randn(shp, generator=gen, dtype=torch.float32)
        if len(shp) == 4:
            fan_in = shp[1] * shp[2] * shp[3]         # 49 for the depth-wise 7x7 ([48, 1, 7, 7])
            sd[k] = n * (2.0 / fan_in) ** 0.5
        elif k.endswith(".layerscale.layerscale"):
            sd[k] = 0.3 * n
        elif k.endswith(".block.1.weight"):           # LayerNorm
            sd[k] = 1.0 + 0.5 * n
        elif k.endswith(".bias"):
            sd[k] = 0.1 * n
        else:
            raise KeyError(f"random_state_dict: no rule for {k} {shp}")
    return sd


def random_state_dict(stem, seed, profile, zero_layers=True):
    """Tensors with exactly the keys and shapes of checkpoint `stem`.  profile "he" or "pow2" (module docstring);
    zero_layers=False leaves out the all-zero layers of "pow2" (what remains of the convunet's is then an exact
    power-of-two rescaling of "he")."""
    sd = _he(checkpoint_shapes(stem), seed)
    if profile == "he":
        return sd
    if profile != "pow2":
        raise ValueError(profile)
    if is_next(stem):
        for bi, b in enumerate(NEXT_BLOCKS):
            if b + ".block.2.weight" not in sd:
                continue                              # preprocessing_layer of a net without features
            k = NEXT_K[bi % len(NEXT_K)]
            sd[b + ".block.2.weight"] = sd[b + ".block.2.weight"] * 2.0 ** k
            sd[b + ".block.2.bias"] = sd[b + ".block.2.bias"] * 2.0 ** k
            sd[b + ".block.4.weight"] = sd[b + ".block.4.weight"] * 2.0 ** -k
        for b in NEXT_LN_BIG:
            sd[b + ".block.1.weight"] = sd[b + ".block.1.weight"] * 6000.0
            sd[b + ".layerscale.layerscale"] = sd[b + ".layerscale.layerscale"] / 6000.0
        if zero_layers:
            sd[NEXT_FC1_ZERO + ".block.2.weight"] = torch.zeros_like(sd[NEXT_FC1_ZERO + ".block.2.weight"])
    else:
        for i, (a, b) in enumerate(UNET_PAIRS):
            k = UNET_K[i % len(UNET_K)]
            sd[a + ".weight"] = sd[a + ".weight"] * 2.0 ** k
            sd[a + ".bias"] = sd[a + ".bias"] * 2.0 ** k
            sd[b + ".weight"] = sd[b + ".weight"] * 2.0 ** -k
        if zero_layers:
            sd[UNET_ZERO + ".weight"] = torch.zeros_like(sd[UNET_ZERO + ".weight"])
    return sd


def to64(sd):
    return {k: v.double() for k, v in sd.items()}


def rel_err(got, want64):
    """max|got - want| / max|want| in f64."""
    want64 = want64.double()
    return float((got.detach().cpu().double() - want64).abs().max() / want64.abs().max())


def net_inputs(B, cin, H, W, seed, feat):
    """x uniform in [-1, 1], feat_in = |N(0, 1)| (None without feature recurrence)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, cin, H, W, generator=gen) * 2 - 1
    f = torch.randn(B, 48, H, W, generator=gen).abs() if feat else None
    return x, f
