"""Parity of the HIP path (through the C ABI) with the golden fixtures captured
from the reference and with the CPU oracle.  Needs a real MI355X: -m gpu.

Tolerances (fp32, the HIP kernels sum in a different order than oneDNN):
  demosaic                      bit-exact
  warp / flow upsample          max-abs 2e-5 on O(1) data
  U-Net forward, sequences      max-abs 1e-4, parity PSNR >= 100 dB,
                                task PSNR within 0.01 dB (north-star bar)
"""
import os

import numpy as np
import pytest
import torch

import rvdd_oracle as O
from conftest import GOLDEN, VARIANTS, WEIGHTS, load_weights
from gpu_support import parity_psnr

pytestmark = pytest.mark.gpu

ARCH = {"basic-iso3200": "convunet", "basic-future-iso3200": "convunet", "feat-iso3200": "convunet+feat",
        "feat-future-iso12800": "convunet+feat", "next-iso3200": "next",
        "next-feat-future-iso3200": "next+feat"}
NETSTR = {"convunet": "convunet-mode=fixedfeatures", "convunet+feat": "convunet-mode=fixedfeatures+feat",
          "next": "newunet", "next+feat": "newunet-mode=feat"}
BUILT = [n for n in sorted(VARIANTS) if not ARCH[n].startswith("next") or os.environ.get("RVDD_TEST_NEXT", "1") == "1"]


def _npz(name):
    return {k: torch.from_numpy(v) for k, v in np.load(os.path.join(GOLDEN, name)).items()}


@pytest.fixture(params=["auto", "winograd", "f32"])
def conv_kernel(request, monkeypatch):
    """Which kernel runs the 3x3 convs.  "auto" is the default: EVERY 3x3 conv of the convunet on the F16 matrix pipe with
    split f32 operands (conv3x3h.hip) at every size -- the 16-channel first layer and UpConv's fused upsample included;
    "f32" picks among the f32-MFMA kernels by launch size, so small frames run the direct
    kernel; "winograd" forces the Winograd f32 kernel at every size: ragged tiles in x and y, the zero_pad_features
    output placement, the 16-channel first layer and the fused 1x1 epilogue all run at the fixture sizes the
    reference pinned.  Read by rvdd_create (RVDD_CONV)."""
    if request.param in ("winograd", "f32"):
        monkeypatch.setenv("RVDD_CONV", request.param)
    else:
        monkeypatch.delenv("RVDD_CONV", raising=False)
    return request.param


@pytest.fixture(scope="module")
def ops():
    from rvdd_release_amd.util._ops import ops_runtime
    return ops_runtime(0)


def test_library_is_the_hip_one():
    from rvdd_release_amd import _lib
    lib = _lib.load()
    assert b"gfx950" in lib.rvdd_version()


def test_demosaic_bit_exact(ops):
    g = _npz("op_hamilton_adams.npz")
    rgb = ops.demosaic(g["raw"].cuda()).cpu()
    assert torch.equal(rgb, g["rgb"])


def test_demosaic_module_surface():
    from rvdd_release_amd.util.Hamilton_Adam_demo import HamiltonAdam
    g = _npz("op_hamilton_adams.npz")
    ha = HamiltonAdam('gbrg')
    rgb = ha(g["raw"].cuda())
    assert torch.equal(rgb.cpu(), g["rgb"])
    assert torch.equal(ha.remosaick(rgb[:, :3]).cpu(), g["remosaick"])


def test_warp_bicubic(ops):
    from rvdd_release_amd.util.flow_utils import warp
    g = _npz("op_warp_bicubic.npz")
    y, mask = warp(g["x"].cuda(), g["flow"].cuda(), "bicubic")
    assert (y.cpu() - g["y"]).abs().max() < 2e-5
    assert torch.equal(mask, g["mask"])
    with pytest.raises(NotImplementedError):
        warp(g["x"].cuda(), g["flow"].cuda(), "bilinear")


def test_upsample_flow(ops):
    from rvdd_release_amd.util.flow_utils import upsample_factor_2
    g = _npz("op_upsample_flow.npz")
    up = upsample_factor_2(g["flow"].cuda(), multiply_by=2)
    assert up.shape == g["up"].shape
    assert (up.cpu() - g["up"]).abs().max() < 1e-5


def test_psnr(ops):
    from rvdd_release_amd.util.util import psnr
    a = torch.rand(1, 3, 40, 56) * 2 - 1
    b = a + 0.01 * torch.randn_like(a)
    assert abs(float(psnr(a.cuda(), b.cuda(), 2.0)) - O.psnr(a, b, 2.0)) < 1e-3


@pytest.mark.parametrize("name", BUILT)
def test_net_forward_golden(name, conv_kernel):
    from rvdd_release_amd.networks import define_net_arch
    stem, fut, _ = VARIANTS[name]
    g = _npz(f"net_{name}.npz")
    net = define_net_arch(3 * (2 + fut), 3, NETSTR[ARCH[name]], gpu_ids=[0])
    net.load_state_dict(load_weights(stem))
    for tag in ("20x28", "16x24"):
        fin = g.get(f"feat_in_{tag}")
        if fin is not None:
            net.set_rec_features([fin.cuda()])
        out = net(g[f"x_{tag}"].cuda()).cpu()
        assert (out - g[f"out_{tag}"]).abs().max() < 1e-4, tag
        if fin is not None:
            f = net.get_current_features()[0].cpu()
            assert (f - g[f"feat_out_{tag}"]).abs().max() < 1e-4, tag


def test_feat_net_requires_features():
    from rvdd_release_amd.networks import define_net_arch
    net = define_net_arch(6, 3, "convunet-mode=fixedfeatures+feat", gpu_ids=[0])
    net.load_state_dict(load_weights("recurrent-convunet+feat-iso3200"))
    with pytest.raises(Exception, match="Old features is None"):
        net(torch.zeros(1, 6, 16, 16).cuda())


@pytest.mark.parametrize("name", BUILT)
def test_sequence_golden_model_surface(name, conv_kernel):
    """Drives the model exactly like validate.py:64-88 drives the reference's."""
    from rvdd_release_amd.models import create_model
    from rvdd_release_amd.options import make_opt
    stem, fut, _ = VARIANTS[name]
    g = _npz(f"seq_{name}.npz")
    opt = make_opt(netDenoiser=NETSTR[ARCH[name]], feature_rec=ARCH[name].endswith("+feat"),
                   future_patch_depth=fut, path2epoch=os.path.join(WEIGHTS, stem), gpu_ids=[0])
    model = create_model(opt)
    model.setup(opt)
    opt.isTrain = False
    model.isTrain = False
    model.eval()
    T = g["raw"].shape[0]
    k = 0
    for t in range(1, T - fut):
        frames = [g["raw"][t - 1], g["raw"][t]] + ([g["raw"][t + 1]] if fut else [])
        flows = [g["flow_prev"][t]] + ([g["flow_next"][t]] if fut else [])
        data = {"n": torch.cat(frames, 0)[None], "flow": torch.stack(flows, 0)[None],
                "gt": torch.cat((g["gt"][t - 1], g["gt"][t]), 0)[None], "n_path": [f"seq/{t:03d}.tif"],
                "gt_path": [f"seq/{t:03d}.tif"], "FirstOfVideo": t == 1}
        model.set_input(data)
        model.test()
        model.compute_losses()
        den = model.get_current_visuals()["denoised"][0].cpu()
        losses = model.get_current_losses()
        assert (den - g["denoised"][k]).abs().max() < 1e-4, (t, float((den - g["denoised"][k]).abs().max()))
        assert parity_psnr(den, g["denoised"][k]) > 100.0
        assert abs(losses["PSNR"] - float(g["PSNR"][k])) < 0.01
        assert abs(losses["L1"] - float(g["L1"][k])) < 1e-3
        assert losses["Denoiser"] == losses["L1"]
        k += 1
    if "feat_last" in g:
        _, feat = model._rt.get_state()
        assert (feat[0].cpu() - g["feat_last"]).abs().max() < 1e-4
    assert model.get_image_paths() == [f"seq/{T - 1 - fut:03d}.tif"]
    assert model.optimizers[0].param_groups[0]['lr'] == opt.lr


@pytest.mark.parametrize("arch,stem,fut,B,H,W", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 2, 72, 104),      # ragged tiles, batch 2
    ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, 1, 36, 52),  # zero_pad_features path
    ("convunet", "recurrent-convunet-iso3200", 0, 1, 256, 256),               # BASELINE config C1 size
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 2, 136, 248),     # shaped like the 1/8 level of 1080p: Winograd
                                                                              # by size, ragged in x at every level
    ("convunet", "recurrent-convunet-future-iso3200", 1, 3, 20, 28),          # smallest golden size, batch 3
    # one sequence of 80 / 48 tiles at level 0: 3 x tiles <= 256 CUs, so EVERY conv launch of the step takes the output-channel
    # split (conv3x3h MT = 1, cout_split_applies) and meets the oracle itself, not only its MT = 3 sibling
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, 1, 128, 160),
    ("convunet", "recurrent-convunet-iso3200", 0, 1, 96, 128),
])
def test_sequence_vs_oracle(arch, stem, fut, B, H, W, conv_kernel):
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if arch.startswith("next") and "next-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    sd = load_weights(stem)
    T = 4 + fut
    seqs = [synth.make_sequence(T, H, W, iso=12800 if "12800" in stem else 3200, seed=40 + b) for b in range(B)]
    want = [O.RecurrentOracle(sd, future=fut).run_sequence(s.raw, s.flow_prev, s.flow_next) for s in seqs]
    raw = torch.stack([s.raw for s in seqs], 0).cuda()           # [B,T,4,h,w]
    fp = torch.stack([s.flow_prev for s in seqs], 0).cuda()
    fn = torch.stack([s.flow_next for s in seqs], 0).cuda()
    rt = RvddRuntime(arch, fut, B, H, W, 0)
    rt.load_state_dict(sd)
    for t in range(1, T - fut):
        out = rt.step(raw[:, t - 1], raw[:, t], raw[:, t + 1] if fut else None, fp[:, t],
                      fn[:, t] if fut else None).cpu()
        for b in range(B):
            d = (out[b] - want[b][t - 1]).abs().max()
            assert d < 1e-4, (t, b, float(d))
            gt = seqs[b].gt[t][None]
            assert abs(O.psnr(out[b][None], gt) - O.psnr(want[b][t - 1][None], gt)) < 0.01


@pytest.mark.parametrize("arch,stem,fut", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0),
    ("convunet", "recurrent-convunet-future-iso3200", 1),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1),
    ("next", "recurrent-ConvNeXtUnet-iso3200", 0),
])
def test_odd_shapes_vs_oracle(arch, stem, fut, conv_kernel):
    """Frames that are tiny, very wide or very tall, none a multiple of 8 or of a kernel's tile: every level ragged,
    zero-pad placement at every decoder stage, whole levels smaller than one tile.  Batch 3, two frame-steps each.
    (tools/shape_sweep.py runs the long form of this: 11 shapes x B in {1, 3}.)"""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if arch.startswith("next") and conv_kernel != "auto":
        pytest.skip("the conv kernel choice does not enter ConvNeXtUnet")
    sd = load_weights(stem)
    T, B = 3 + fut, 3
    for H, W in ((16, 16), (18, 34), (22, 130), (130, 22), (50, 66)):
        seqs = [synth.make_sequence(T, H, W, iso=3200, seed=900 + b) for b in range(B)]
        want = [O.RecurrentOracle(sd, future=fut).run_sequence(s.raw, s.flow_prev, s.flow_next) for s in seqs]
        raw = torch.stack([s.raw for s in seqs], 0).cuda()
        fp = torch.stack([s.flow_prev for s in seqs], 0).cuda()
        fn = torch.stack([s.flow_next for s in seqs], 0).cuda()
        rt = RvddRuntime(arch, fut, B, H, W, 0)
        rt.load_state_dict(sd)
        for t in range(1, T - fut):
            out = rt.step(raw[:, t - 1], raw[:, t], raw[:, t + 1] if fut else None, fp[:, t], fn[:, t] if fut else None).cpu()
            for b in range(B):
                d = (out[b] - want[b][t - 1]).abs().max()
                assert d < 1e-4, (H, W, t, b, float(d))
        rt.close()


def test_state_roundtrip_and_reset():
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    H, W = 48, 64
    s = synth.make_sequence(4, H, W, seed=3)
    raw, fp = s.raw.cuda(), s.flow_prev.cuda()
    rt = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
    rt.load_state_dict(sd)
    o1 = rt.step(raw[0][None], raw[1][None], None, fp[1][None], None).clone()
    den, feat = rt.get_state()
    assert torch.equal(den, o1)
    o2 = rt.step(None, raw[2][None], None, fp[2][None], None).clone()
    # restoring the state replays the same frame bit for bit
    rt.set_state(den, feat)
    o2b = rt.step(None, raw[2][None], None, fp[2][None], None)
    assert torch.equal(o2, o2b)
    # FirstOfVideo: reset + same inputs == first output again
    rt.reset()
    o1b = rt.step(raw[0][None], raw[1][None], None, fp[1][None], None)
    assert torch.equal(o1, o1b)


@pytest.mark.parametrize("conv", [0, 2])
@pytest.mark.parametrize("B,H,W", [(1, 36, 52), (2, 72, 104), (1, 256, 256)])
def test_fused_upsample_equals_upsample_then_conv(B, H, W, conv):
    """UpConv (networks/unet.py:88-147): the bilinear x2 upsample interpolated inside the conv kernel's input fetch
    (the split-f16 kernel's halo fetch, conv = 0; the Winograd f32 kernel's patch load, conv = 2) gives the same bits
    as the upsample kernel followed by the same conv kernel (same operations in the same order), at sizes with ragged
    tiles, clamped borders and the zero_pad_features placement."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    seqs = [synth.make_sequence(3, H, W, iso=3200, seed=90 + b, device="cuda") for b in range(B)]
    outs = []
    for fused in (1, 0):
        rt = RvddRuntime("convunet+feat", 0, B, H, W, 0)
        rt.set_option("conv_kernel", conv)
        rt.set_option("fuse_upsample", fused)
        rt.load_state_dict(sd)
        st = lambda f: torch.stack([f(s) for s in seqs], 0)
        o = [rt.step(st(lambda s: s.raw[0]), st(lambda s: s.raw[1]), None, st(lambda s: s.flow_prev[1]), None).clone(),
             rt.step(None, st(lambda s: s.raw[2]), None, st(lambda s: s.flow_prev[2]), None).clone()]
        outs.append(o)
        rt.close()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("arch,stem,B,H,W", [("convunet", "recurrent-convunet-iso3200", 1, 256, 256),
                                              ("convunet+feat", "recurrent-convunet+feat-iso3200", 2, 50, 66),
                                              ("convunet", "recurrent-convunet-iso3200", 3, 18, 34),
                                              ("convunet+feat", "recurrent-convunet+feat-iso3200", 1, 136, 248)])
def test_one_kernel_prestage_equals_three_kernels(arch, stem, B, H, W):
    """The pre-stage of a small frame-step without a future frame (bound of the network input, green plane, network input) in
    ONE kernel (netin.hip netin_small_kernel, option small_prestage, the default where it applies) against its three
    kernels: same bits in frames and recurrent features over four steps (the first, whose bound also covers the previous raw
    frame, included), ragged tiles, clamped borders, flows pointing outside, a frame
    1e4 times brighter (the bound's words steer the block floating point of the convs behind it)."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights(stem)
    seqs = [synth.make_sequence(6, H, W, iso=3200, seed=700 + b, device="cuda") for b in range(B)]
    for scale in (1.0, 1e4):
        outs = []
        for small in (1, 0):
            rt = RvddRuntime(arch, 0, B, H, W, 0)
            rt.set_option("small_prestage", small)
            rt.load_state_dict(sd)
            st = lambda f: torch.stack([f(s) for s in seqs], 0)
            o = []
            for t in range(1, 5):
                fl = st(lambda s: s.flow_prev[t]).clone()
                fl[:, :, :, -3:] += 200.0
                o.append(rt.step(st(lambda s: s.raw[t - 1]) * scale if t == 1 else None, st(lambda s: s.raw[t]) * scale, None, fl, None).clone())
            feat = rt.get_state()[1]
            o.append(feat.clone() if feat is not None else torch.zeros(1, device="cuda"))
            outs.append(o)
            rt.set_option("small_prestage", 1)
            rt.close()
        for a, b in zip(*outs):
            assert torch.equal(a, b), (scale, float((a - b).abs().max()))
        assert torch.isfinite(outs[0][3]).all()


def test_step_on_channel_slices_without_copies():
    """rvdd_step_strided: the model hands the runtime `n[:, 0:4]`, `n[:, 4:8]`, `n[:, 8:12]` and `flow[:, k]` of the
    dataset's tensors; with B > 1 those are strided over the batch.  Same bits as the dense call, and no copy."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime, _batch_strided
    sd = load_weights("recurrent-convunet+feat-future-iso12800")
    B, H, W = 3, 40, 56
    seqs = [synth.make_sequence(4, H, W, iso=12800, seed=80 + b, device="cuda") for b in range(B)]
    n = torch.stack([torch.cat((s.raw[0], s.raw[1], s.raw[2]), 0) for s in seqs], 0)          # [B,12,h,w]
    fl = torch.stack([torch.stack((s.flow_prev[1], s.flow_next[1]), 0) for s in seqs], 0)      # [B,2,2,h,w]
    t, stride = _batch_strided(n[:, 4:8], (B, 4, H // 2, W // 2), "raw_cur", 0)
    assert t.data_ptr() == n[:, 4:8].data_ptr() and stride == 12 * (H // 2) * (W // 2)       # a view, not a copy
    outs = []
    for dense in (False, True):
        rt = RvddRuntime("convunet+feat", 1, B, H, W, 0)
        rt.load_state_dict(sd)
        c = (lambda x: x.contiguous()) if dense else (lambda x: x)
        outs.append(rt.step(c(n[:, 0:4]), c(n[:, 4:8]), c(n[:, 8:12]), c(fl[:, 0]), c(fl[:, 1])).clone())
        rt.close()
    assert torch.equal(outs[0], outs[1])
    rt = RvddRuntime("convunet", 0, 2, 32, 48, 0)
    rt.load_state_dict(load_weights("recurrent-convunet-iso3200"))
    z = torch.zeros(2, 4, 16, 24, device="cuda")
    rc = rt.lib.rvdd_step_strided(rt.h, z.data_ptr(), z.data_ptr(), None, z.data_ptr(), None, 5, 0, z.data_ptr(), 0)
    assert rc != 0 and b"batch stride" in rt.lib.rvdd_last_error(rt.h)


def test_two_devices_in_one_process():
    """A process that drives two GPUs: per-device kernel attributes, every entry point on its handle's device
    whatever the caller's current device is, and a tensor on the wrong device refused.  Needs two visible GPUs."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    H, W = 64, 96
    s = synth.make_sequence(3, H, W, seed=12)
    outs = []
    for dev in (0, 1):
        rt = RvddRuntime("convunet+feat", 0, 1, H, W, dev)
        rt.load_state_dict(sd)
        torch.cuda.set_device(1 - dev)                           # the caller's current device is the OTHER one
        d = f"cuda:{dev}"
        o = rt.step(s.raw[0][None].to(d), s.raw[1][None].to(d), None, s.flow_prev[1][None].to(d), None)
        assert torch.cuda.current_device() == 1 - dev            # and stays what it was
        outs.append(o.cpu())
        with pytest.raises(RuntimeError, match="lives on"):
            rt.step(None, s.raw[2][None].to(f"cuda:{1 - dev}"), None, s.flow_prev[2][None].to(d), None)
        rt.close()
    torch.cuda.set_device(0)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("arch,stem", [("convunet+feat", "recurrent-convunet+feat-future-iso12800"),
                                       ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso12800")])
def test_graph_replay_equals_eager(arch, stem):
    """rvdd_set_option("graphs", 1): frame-steps captured into hipGraphs and replayed (one graph per distinct set of
    caller buffers, the first frame of a video its own) give the same bits as launch-by-launch execution, across
    a reset and with buffers that repeat."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights(stem)
    H, W, T = 48, 64, 6
    s = synth.make_sequence(T, H, W, iso=12800, seed=31, device="cuda")
    outs = {}
    for graphs in (0, 1):
        rt = RvddRuntime(arch, 1, 1, H, W, 0)
        rt.load_state_dict(sd)
        rt.set_option("graphs", graphs)
        buf = torch.empty(2, 1, 3, H, W, device="cuda")           # two output buffers, reused alternately
        got = []
        for rep in range(2):                                       # the second pass replays every graph of the first
            rt.reset()
            for t in range(1, T - 1):
                o = rt.step(s.raw[t - 1][None] if t == 1 else None, s.raw[t][None], s.raw[t + 1][None],
                            s.flow_prev[t][None], s.flow_next[t][None], out=buf[t & 1])
                got.append(o.clone())
        outs[graphs] = got
        rt.close()
    assert len(outs[0]) == 2 * (T - 2)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    for k in range(T - 2):
        assert torch.equal(outs[1][k], outs[1][k + T - 2])         # replayed pass == captured pass


def test_error_paths():
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    rt = RvddRuntime("convunet+feat", 0, 1, 32, 32, 0)
    z = torch.zeros(1, 4, 16, 16).cuda()
    f = torch.zeros(1, 2, 16, 16).cuda()
    with pytest.raises(RuntimeError, match="not finalized"):
        rt.step(z, z, None, f, None)
    bad = dict(sd)
    bad["bogus.weight"] = torch.zeros(3)
    with pytest.raises(RuntimeError, match="unexpected state_dict key"):
        rt.load_state_dict(bad)
    rt2 = RvddRuntime("convunet+feat", 0, 1, 32, 32, 0)
    part = {k: v for k, v in sd.items() if k != "PostConvs.1.bias"}
    with pytest.raises(RuntimeError, match="missing state_dict key"):
        rt2.load_state_dict(part)
    rt3 = RvddRuntime("convunet+feat", 0, 1, 32, 32, 0)
    rt3.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="raw_prev is required"):
        rt3.step(None, z, None, f, None)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt3.step(z.cpu(), z, None, f, None)
    with pytest.raises(RuntimeError, match="too large"):       # 5120x2880: a 48-channel map of 2.8 GB
        RvddRuntime("convunet+feat", 0, 1, 2880, 5120, 0)
    with pytest.raises(RuntimeError, match="even and >= 16"):
        RvddRuntime("convunet+feat", 0, 1, 33, 32, 0)


def test_full_size_720p_vs_oracle_and_invariants():
    """BASELINE config C2 at its real size: two output frames against the oracle, and the
    size-independent properties of the path -- run-to-run determinism, batch independence
    (sequence b of a B=2 run == the same sequence run alone, bit for bit), Winograd == direct
    kernel within fp32 noise."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    H, W, T = 720, 1280, 3
    seqs = [synth.make_sequence(T, H, W, iso=3200, seed=2000 + b, device="cuda") for b in range(2)]

    def run(B, which, steps=T - 1):
        rt = RvddRuntime("convunet+feat", 0, B, H, W, 0)
        rt.load_state_dict(sd)
        outs = []
        for t in range(1, 1 + steps):
            raw_p = torch.stack([seqs[b].raw[t - 1] for b in which], 0)
            raw_c = torch.stack([seqs[b].raw[t] for b in which], 0)
            fl = torch.stack([seqs[b].flow_prev[t] for b in which], 0)
            outs.append(rt.step(raw_p if t == 1 else None, raw_c, None, fl, None).clone())
        _, feat = rt.get_state()
        rt.close()
        return outs, feat

    both, feat_both = run(2, [0, 1])
    again, _ = run(2, [0, 1])
    alone, feat_alone = run(1, [1])
    for t in range(T - 1):
        assert torch.equal(both[t], again[t])                       # deterministic
        assert torch.equal(both[t][1], alone[t][0])                 # batch independent
    assert torch.equal(feat_both[1], feat_alone[0])

    orc = O.RecurrentOracle(sd, future=0)
    s0 = seqs[0]
    for t in range(1, T):
        want = orc.step(s0.raw[t - 1][None].cpu(), s0.raw[t][None].cpu(), None, s0.flow_prev[t][None].cpu(), None,
                        first=(t == 1))[0]
        got = both[t - 1][0].cpu()
        assert (got - want).abs().max() < 1e-4 and parity_psnr(got, want) > 120.0
        gt = s0.gt[t][None].cpu()
        assert abs(O.psnr(got[None], gt) - O.psnr(want[None], gt)) < 0.01

    os.environ["RVDD_CONV"] = "direct"
    try:
        direct, _ = run(1, [1], steps=1)
    finally:
        del os.environ["RVDD_CONV"]
    assert (direct[0] - alone[0]).abs().max() < 1e-4 and parity_psnr(direct[0].cpu(), alone[0].cpu()) > 120.0


@pytest.mark.parametrize("arch,stem,fut,iso", [
    ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1, 12800),       # BASELINE config C3
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, 3200),        # BASELINE config C4
])
def test_full_size_720p_future_configs_vs_oracle(arch, stem, fut, iso):
    """BASELINE configs C3 and C4 at their real size (1280x720, future frame): two output frames against the
    oracle (max-abs < 1e-4, parity PSNR > 120 dB, task PSNR within 0.01 dB) and run-to-run determinism."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if arch.startswith("next") and "next-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    sd = load_weights(stem)
    H, W, T = 720, 1280, 4
    s0 = synth.make_sequence(T, H, W, iso=iso, seed=3000 + fut, device="cuda")

    def run():
        rt = RvddRuntime(arch, fut, 1, H, W, 0)
        rt.load_state_dict(sd)
        outs = [rt.step(s0.raw[t - 1][None] if t == 1 else None, s0.raw[t][None], s0.raw[t + 1][None],
                        s0.flow_prev[t][None], s0.flow_next[t][None]).clone() for t in (1, 2)]
        _, feat = rt.get_state()
        rt.close()
        return outs, feat

    got, feat = run()
    again, feat2 = run()
    for a, b in zip(got, again):
        assert torch.equal(a, b)
    assert torch.equal(feat, feat2)
    orc = O.RecurrentOracle(sd, future=fut)
    c = lambda x: x[None].cpu()
    for t in (1, 2):
        want = orc.step(c(s0.raw[t - 1]), c(s0.raw[t]), c(s0.raw[t + 1]), c(s0.flow_prev[t]), c(s0.flow_next[t]),
                        first=(t == 1))[0]
        g = got[t - 1][0].cpu()
        assert (g - want).abs().max() < 1e-4 and parity_psnr(g, want) > 120.0, (t, float((g - want).abs().max()))
        gt = c(s0.gt[t])
        assert abs(O.psnr(g[None], gt) - O.psnr(want[None], gt)) < 0.01


def test_batch_of_four_720p_invariants():
    """B = 4 (the bench batch).  At 720p the 1/8-resolution level switches from the direct kernel (B <= 2) to the
    Winograd kernel (B >= 4: enough 8x32-pixel units to fill the chip), so a sequence of a B = 4 run equals the
    same sequence run alone TO FP32 TOLERANCE (max-abs < 1e-4, parity > 120 dB), not bit for bit; what does hold
    bit for bit is position independence inside the batch (the same sequence in slots 0 and 2) and, with the
    kernel choice pinned (conv_kernel = winograd at every size), equality with the run alone."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    H, W = 720, 1280
    seqs = [synth.make_sequence(3, H, W, iso=3200, seed=2100 + b, device="cuda") for b in range(2)]

    def run(which, conv=0, seq_major=0):
        rt = RvddRuntime("convunet+feat", 0, len(which), H, W, 0)
        rt.set_option("conv_kernel", conv)
        rt.set_option("seq_major", seq_major)
        rt.load_state_dict(sd)
        outs = []
        for t in (1, 2):
            st = lambda f: torch.stack([f(seqs[b]) for b in which], 0)
            outs.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]), None,
                                st(lambda s: s.flow_prev[t]), None).clone())
        rt.close()
        return outs

    four = run([0, 1, 0, 1])
    alone = run([1])
    for t in range(2):
        assert torch.equal(four[t][0], four[t][2]) and torch.equal(four[t][1], four[t][3])
        d = (four[t][1] - alone[t][0]).abs().max()
        assert d < 1e-4 and parity_psnr(four[t][1].cpu(), alone[t][0].cpu()) > 120.0, float(d)
    four_w = run([0, 1, 0, 1], conv=2)
    alone_w = run([1], conv=2)
    for t in range(2):
        assert torch.equal(four_w[t][1], alone_w[t][0])
    # the other schedule of the same work (full-resolution stages one sequence at a time, serpentine order over the
    # frames): the same kernels on the same tiles, so the same bits
    four_s = run([0, 1, 0, 1], seq_major=1)
    for t in range(2):
        assert torch.equal(four_s[t], four[t])


@pytest.mark.parametrize("arch,stem,fut", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1),
])
def test_1080p_frame_vs_oracle(arch, stem, fut):
    """1920x1080, B = 2, at full scale: the levels are 1080 / 540 / 270 / 135 rows by 1920 / 960 / 480 / 240 columns,
    so the Winograd tiles (8x32 pixels) are ragged in y at every level below the first and in x AND y at the 1/8
    level, which runs the Winograd kernel at this batch; for ConvNeXtUnet the 16x16 tiles of the depth-wise kernel are
    ragged at every level and the 135-row level is zero-padded against its 136-row skip (new_unet.py:56-66).
    One step: sequence 0 against the oracle, both deterministic."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights(stem)
    H, W = 1080, 1920
    seqs = [synth.make_sequence(3, H, W, iso=3200, seed=5000 + b, device="cuda") for b in range(2)]
    st = lambda f: torch.stack([f(s) for s in seqs], 0)
    nxt = (lambda f: st(f)) if fut else (lambda f: None)
    outs = []
    for _ in range(2):
        rt = RvddRuntime(arch, fut, 2, H, W, 0)
        rt.load_state_dict(sd)
        outs.append(rt.step(st(lambda s: s.raw[0]), st(lambda s: s.raw[1]), nxt(lambda s: s.raw[2]), st(lambda s: s.flow_prev[1]),
                            nxt(lambda s: s.flow_next[1])).clone())
        rt.close()
    assert torch.equal(outs[0], outs[1])
    c = lambda x: x[None].cpu()
    s0 = seqs[0]
    want = O.RecurrentOracle(sd, future=fut).step(c(s0.raw[0]), c(s0.raw[1]), c(s0.raw[2]) if fut else None, c(s0.flow_prev[1]),
                                                  c(s0.flow_next[1]) if fut else None, first=True)[0]
    got = outs[0][0].cpu()
    assert (got - want).abs().max() < 1e-4 and parity_psnr(got, want) > 120.0, float((got - want).abs().max())


def test_4k_frame_borders():
    """A frame above 5.59 Mpx (one 48-channel map > 2^30 bytes): the padding-1 border of the 3x3 convs comes from
    the buffer range check, which must hold whatever the size of the map.  One step of config C2's net on a
    3840x2176 frame against the oracle, whole frame (borders included), Winograd and direct kernel."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    H, W = 2176, 3840
    s0 = synth.make_sequence(2, H, W, iso=3200, seed=4000, device="cuda")
    outs = {}
    for conv in (0, 1):
        rt = RvddRuntime("convunet+feat", 0, 1, H, W, 0)
        rt.set_option("conv_kernel", conv)
        rt.load_state_dict(sd)
        outs[conv] = rt.step(s0.raw[0][None], s0.raw[1][None], None, s0.flow_prev[1][None], None)[0].cpu()
        rt.close()
    c = lambda x: x[None].cpu()
    want = O.RecurrentOracle(sd, future=0).step(c(s0.raw[0]), c(s0.raw[1]), None, c(s0.flow_prev[1]), None, first=True)[0]
    for conv, got in outs.items():
        d = (got - want).abs()
        assert d.max() < 1e-4, (conv, float(d.max()))
        # the outermost ring of pixels is where a wrong (non-zero) halo read would show
        ring = torch.cat((d[:, :2].flatten(), d[:, -2:].flatten(), d[:, :, :2].flatten(), d[:, :, -2:].flatten()))
        assert ring.max() < 1e-4 and parity_psnr(got, want) > 120.0


def test_4k_frame_next_batch_of_two():
    """ConvNeXtUnet at 3840x2176 (a 48-channel map of 1.6 GB; the oracle does not finish a frame of this size in the suite's time, and the
    net is not crop-invariant -- its upsampling is align_corners=True -- so no crop of the oracle's stands in).  Size-independent properties
    instead: two copies of one sequence in a batch give the same bits in both slots and the bits of the sequence alone (every offset that
    involves the batch index or the image size: halo DMA, projection epilogues, feature warp, pooled maps), the frames are finite, and they
    denoise: PSNR against the clean frame within 1 dB of what the same net reaches on the 720p corner of the same scene."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if "next-iso3200" not in BUILT:
        pytest.skip("ConvNeXt weights not converted")
    sd = load_weights("recurrent-ConvNeXtUnet+feat-future-iso3200")
    H, W = 2176, 3840
    s0 = synth.make_sequence(3, H, W, iso=3200, seed=4100, device="cuda")

    def run(B, h, w, crop):
        rt = RvddRuntime("next+feat", 1, B, h, w, 0)
        rt.load_state_dict(sd)
        st = lambda x: torch.stack([crop(x)] * B, 0).contiguous()
        out = rt.step(st(s0.raw[0]), st(s0.raw[1]), st(s0.raw[2]), st(s0.flow_prev[1]), st(s0.flow_next[1])).clone()
        rt.close()
        return out

    full = lambda x: x
    two = run(2, H, W, full)
    assert torch.isfinite(two).all()
    assert torch.equal(two[0], two[1])
    one = run(1, H, W, full)
    assert torch.equal(one[0], two[0])
    psnr = lambda a, b: float(10 * torch.log10(4.0 / ((a - b) ** 2).mean()))
    p_full = psnr(two[0], s0.gt[1])
    # the same scene's top-left 1280x720 (raw 640x360) through the same net
    small = run(1, 720, 1280, lambda x: x[..., :360, :640] if x.shape[-1] == W // 2 else x[..., :720, :1280])
    p_small = psnr(small[0], s0.gt[1][:, :720, :1280])
    assert p_full > 30.0 and abs(p_full - p_small) < 1.0, (p_full, p_small)


def test_all_twenty_checkpoints_load_strictly_and_run():
    """Every checkpoint of the reference's trained-nets/ passes the runtime's strict key/shape table
    (handle.hip expected_keys) under the architecture its name states and produces a finite frame."""
    import glob
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    stems = sorted(os.path.basename(p)[:-12] for p in glob.glob(os.path.join(WEIGHTS, "*.safetensors")))
    assert len(stems) == 20
    H, W = 32, 48
    s = synth.make_sequence(3, H, W, seed=5, device="cuda")
    for stem in stems:
        fut = 1 if "-future" in stem else 0
        arch = ("next" if "ConvNeXt" in stem else "convunet") + ("+feat" if "+feat" in stem else "")
        if arch.startswith("next") and "next-iso3200" not in BUILT:
            continue
        rt = RvddRuntime(arch, fut, 1, H, W, 0)
        rt.load_state_dict(load_weights(stem))
        if "no_warp" in stem:
            rt.set_option("no_warp", 1)
        out = rt.step(s.raw[0][None], s.raw[1][None], s.raw[2][None] if fut else None, s.flow_prev[1][None],
                      s.flow_next[1][None] if fut else None)
        assert torch.isfinite(out).all() and out.abs().max() < 4, stem
        # a checkpoint of another family is refused by name, not silently half-loaded
        other = RvddRuntime("convunet" if arch != "convunet" else "convunet+feat", fut, 1, H, W, 0)
        with pytest.raises(RuntimeError, match="state_dict key"):
            other.load_state_dict(load_weights(stem))
        other.close()
        rt.close()


def test_empty_and_odd_inputs(ops):
    """Zero-sized batches are accepted and launch nothing; odd (non multiple of the tile) sizes of the single ops."""
    assert ops.demosaic(torch.zeros(0, 4, 8, 12).cuda()).shape == (0, 3, 16, 24)
    assert ops.warp(torch.zeros(0, 3, 9, 11).cuda(), torch.zeros(0, 2, 9, 11).cuda()).shape == (0, 3, 9, 11)
    assert ops.upsample_factor_2(torch.zeros(0, 2, 5, 7).cuda(), 2.0).shape == (0, 2, 10, 14)
    u8 = ops.ppipe(torch.zeros(0, 3, 6, 10).cuda(), 1.2, 2.0, 3.0, 3200, -1)
    assert u8.shape == (0, 6, 10, 3)
    gen = torch.Generator().manual_seed(9)
    x = torch.rand(2, 3, 7, 13, generator=gen) * 2 - 1                       # odd H and W, C = 3
    fl = (torch.rand(2, 2, 7, 13, generator=gen) - 0.5) * 6
    got = ops.warp(x.cuda(), fl.cuda()).cpu()
    assert (got - O.warp(x, fl)).abs().max() < 2e-5
    raw = torch.rand(3, 8, 5, 9, generator=gen) * 2 - 1                      # two packed frames, odd raw size
    assert torch.equal(ops.demosaic(raw.cuda()).cpu(), O.hamilton_adams(raw))


@pytest.mark.parametrize("name,stem,fut", [("nowarp-iso3200", "non_recurrent-convunet-no_warp-iso3200", 0),
                                           ("nowarp-future-iso3200", "non_recurrent-convunet-no_warp-future-iso3200", 1)])
def test_no_warp_model_surface(name, stem, fut):
    """scripts/test-non_recurrent-no_warp-*.sh: `--no_warp`, the dataset hands over no flows."""
    from rvdd_release_amd.models import create_model
    from rvdd_release_amd.options import make_opt
    g = _npz(f"seq_{name}.npz")
    opt = make_opt(netDenoiser="convunet-mode=fixedfeatures", future_patch_depth=fut, no_warp=True,
                   path2epoch=os.path.join(WEIGHTS, stem), gpu_ids=[0])
    assert opt.name == "recurrent-convunet-mode=fixedfeatures-i3o3"          # no "-warp" in the run name (base_options.py:131)
    model = create_model(opt)
    model.setup(opt)
    opt.isTrain = model.isTrain = False
    model.eval()
    T = g["raw"].shape[0]
    for k, t in enumerate(range(1, T - fut)):
        frames = [g["raw"][t - 1], g["raw"][t]] + ([g["raw"][t + 1]] if fut else [])
        data = {"n": torch.cat(frames, 0)[None], "flow": [], "gt": torch.cat((g["gt"][t - 1], g["gt"][t]), 0)[None],
                "n_path": [f"seq/{t:03d}.tif"], "gt_path": [f"seq/{t:03d}.tif"], "FirstOfVideo": t == 1}
        model.set_input(data)
        model.test()
        model.compute_losses()
        den = model.get_current_visuals()["denoised"][0].cpu()
        assert (den - g["denoised"][k]).abs().max() < 1e-4
        assert abs(model.get_current_losses()["PSNR"] - float(g["PSNR"][k])) < 0.01
    # the option is per runtime: a warping model on another runtime still insists on its flows
    from rvdd_release_amd.runtime import RvddRuntime
    rt = RvddRuntime("convunet", 0, 1, 32, 48, 0)
    rt.load_state_dict(load_weights("recurrent-convunet-iso3200"))
    z = g["raw"][0][None].cuda()
    with pytest.raises(RuntimeError, match="flow_prev is required"):
        rt.step(z, z, None, None, None)
    with pytest.raises(RuntimeError, match="unknown option"):
        rt.set_option("bogus", 1)


def test_prev_noisy_frame_model_surface():
    from rvdd_release_amd.models import create_model
    from rvdd_release_amd.options import make_opt
    g = _npz("seq_prevnoisy-feat-iso3200.npz")
    opt = make_opt(netDenoiser="convunet-mode=fixedfeatures+feat", feature_rec=True, prev_noisy_frame=True,
                   path2epoch=os.path.join(WEIGHTS, "recurrent-convunet+feat-iso3200"), gpu_ids=[0])
    model = create_model(opt)
    model.setup(opt)
    opt.isTrain = model.isTrain = False
    model.eval()
    for k, t in enumerate(range(1, g["raw"].shape[0])):
        data = {"n": torch.cat((g["raw"][t - 1], g["raw"][t]), 0)[None], "flow": g["flow_prev"][t][None, None],
                "gt": torch.cat((g["gt"][t - 1], g["gt"][t]), 0)[None], "n_path": [f"seq/{t:03d}.tif"],
                "gt_path": [f"seq/{t:03d}.tif"], "FirstOfVideo": t == 1}
        model.set_input(data)
        model.test()
        model.compute_losses()
        den = model.get_current_visuals()["denoised"][0].cpu()
        assert (den - g["denoised"][k]).abs().max() < 1e-4
        assert abs(model.get_current_losses()["PSNR"] - float(g["PSNR"][k])) < 0.01
    # the state that is handed on is the noisy frame: Hamilton-Adams of the last raw frame, bit for bit
    lastden, _ = model._rt.get_state()
    assert torch.equal(lastden.cpu(), O.hamilton_adams(g["raw"][-1][None]))


@pytest.mark.parametrize("name,stem,fut", [("warpraw-iso3200", "recurrent-convunet-iso3200", 0),
                                           ("warpraw-future-iso3200", "recurrent-convunet-future-iso3200", 1)])
def test_warp_raw_model_surface(name, stem, fut):
    from rvdd_release_amd.models import create_model
    from rvdd_release_amd.options import make_opt
    g = _npz(f"seq_{name}.npz")
    opt = make_opt(netDenoiser="convunet-mode=fixedfeatures", future_patch_depth=fut, warp_raw=True,
                   path2epoch=os.path.join(WEIGHTS, stem), gpu_ids=[0])
    model = create_model(opt)
    model.setup(opt)
    opt.isTrain = model.isTrain = False
    model.eval()
    T = g["raw"].shape[0]
    for k, t in enumerate(range(1, T - fut)):
        frames = [g["raw"][t - 1], g["raw"][t]] + ([g["raw"][t + 1]] if fut else [])
        flows = [g["flow_prev"][t]] + ([g["flow_next"][t]] if fut else [])
        data = {"n": torch.cat(frames, 0)[None], "flow": torch.stack(flows, 0)[None],
                "gt": torch.cat((g["gt"][t - 1], g["gt"][t]), 0)[None], "n_path": [f"seq/{t:03d}.tif"],
                "gt_path": [f"seq/{t:03d}.tif"], "FirstOfVideo": t == 1}
        model.set_input(data)
        model.test()
        model.compute_losses()
        den = model.get_current_visuals()["denoised"][0].cpu()
        assert (den - g["denoised"][k]).abs().max() < 1e-4
        assert abs(model.get_current_losses()["PSNR"] - float(g["PSNR"][k])) < 0.01
    # with feature recurrence the reference fails on tensor shapes in this mode; here: a clear error
    from rvdd_release_amd.runtime import RvddRuntime
    with pytest.raises(RuntimeError, match="feature recurrence"):
        RvddRuntime("convunet+feat", 0, 1, 32, 48, 0).set_option("warp_raw", 1)


def test_model_runtime_survives_denoiser_calls_at_other_sizes():
    """The denoiser keeps the runtimes of the last two frame sizes; the one that holds a video's recurrent state
    (handed to recurrentModel.forward) is pinned: direct calls of the net at other sizes must not evict it, and the
    video continues bit for bit.  A runtime that WAS closed says so."""
    from rvdd_release_amd.models import create_model
    from rvdd_release_amd.options import make_opt
    from rvdd_release_amd.runtime import RvddRuntime
    g = _npz("seq_feat-iso3200.npz")
    stem = "recurrent-convunet+feat-iso3200"

    def frames(model, disturb):
        outs = []
        for t in range(1, 4):
            data = {"n": torch.cat((g["raw"][t - 1], g["raw"][t]), 0)[None], "flow": g["flow_prev"][t][None, None],
                    "gt": torch.cat((g["gt"][t - 1], g["gt"][t]), 0)[None], "n_path": ["a"], "gt_path": ["a"],
                    "FirstOfVideo": t == 1}
            model.set_input(data)
            model.test()
            if disturb:
                net = model._netDenoise
                saved = net.get_current_features()
                for (H, W) in ((16, 24), (24, 16), (40, 40)):
                    net.get_rec_nil_features(1, H, W)
                    net(torch.zeros(1, 6, H, W).cuda())
                net.set_rec_features(saved)
            model.compute_losses()                        # on the pinned runtime, still alive
            outs.append(model.get_current_visuals()["denoised"].clone())
        return outs

    def make():
        opt = make_opt(netDenoiser="convunet-mode=fixedfeatures+feat", feature_rec=True, path2epoch=os.path.join(WEIGHTS, stem), gpu_ids=[0])
        m = create_model(opt)
        m.setup(opt)
        opt.isTrain = m.isTrain = False
        return m.eval() or m

    a, b = frames(make(), False), frames(make(), True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    rt = RvddRuntime("convunet+feat", 0, 1, 32, 48, 0)
    rt.load_state_dict(load_weights(stem))
    rt.close()
    with pytest.raises(RuntimeError, match="is closed"):
        rt.reset()


@pytest.mark.parametrize("arch,stem,fut,opt", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0, ("conv_kernel", 4)),
    ("convunet", "recurrent-convunet-future-iso3200", 1, ("conv_kernel", 2)),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1, ("next_split", 0)),
])
def test_split_f16_matrix_path_matches_f32_kernels(arch, stem, fut, opt):
    """The default path multiplies its dense convs on the F16 matrix pipe with every f32 operand split into two f16
    halves (three MFMAs per product, f32 accumulation: conv3x3h.hip, convnext.hip SPLIT); the option selects the
    kernels that multiply f32 operands on the f32 matrix pipe.  Same frames to fp32 rounding noise -- max-abs < 2e-5,
    parity PSNR > 120 dB -- over four recurrent steps at sizes with ragged tiles and zero-padded levels, batches."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if arch.startswith("next") and "next-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    sd = load_weights(stem)
    for B, H, W in ((2, 72, 104), (1, 180, 320), (3, 50, 66)):
        T = 5 + fut
        seqs = [synth.make_sequence(T, H, W, iso=3200, seed=700 + b, device="cuda") for b in range(B)]
        st = lambda f: torch.stack([f(s) for s in seqs], 0)
        outs = []
        for exact in (0, 1):
            rt = RvddRuntime(arch, fut, B, H, W, 0)
            if exact:
                rt.set_option(*opt)
            rt.load_state_dict(sd)
            o = []
            for t in range(1, T - fut):
                o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]),
                                 st(lambda s: s.raw[t + 1]) if fut else None, st(lambda s: s.flow_prev[t]),
                                 st(lambda s: s.flow_next[t]) if fut else None).clone())
            outs.append(o)
            rt.close()
        for a, b in zip(*outs):
            assert (a - b).abs().max() < 2e-5 and parity_psnr(a.cpu(), b.cpu()) > 120.0, (B, H, W, float((a - b).abs().max()))


@pytest.mark.parametrize("arch,stem,fut", [
    ("convunet+feat", "recurrent-convunet+feat-iso3200", 0),
    ("convunet", "recurrent-convunet-future-iso3200", 1),
    ("next+feat", "recurrent-ConvNeXtUnet+feat-future-iso3200", 1),
])
@pytest.mark.parametrize("mag", [1.0e5, 2.0 ** 20, 2.0 ** -8, 2.0 ** -12])
def test_split_path_any_magnitude(arch, stem, fut, mag):
    """The reference's convs are fp32 at any magnitude (networks/unet.py:26-76, new_unet.py:74-103).  The default path
    multiplies f16 halves, whose exponent range is 2^-14 .. 65504 -- and must not care: the split-f16 convs carry one
    power of two per map and sequence (block floating point, rvdd_internal.h: amax words written by the producing kernel),
    the ConvNeXt MLP's operands are bounded by its LayerNorm whatever the frames are (checked against the weights at
    load).  Frames 1e5 / 2^20 times brighter and 2^-8 / 2^-12 times dimmer than the [-1, 1] the reference feeds, three
    recurrent steps (so the recurrent features and the previous output carry the magnitude too): every frame within
    1e-4 of the oracle RELATIVE to the frame's own max-abs, and never a NaN or an infinity."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if arch.startswith("next") and "next-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    sd = load_weights(stem)
    H, W, T = 64, 96, 4 + fut
    s = synth.make_sequence(T, H, W, iso=3200, seed=5, device="cuda")
    raw = s.raw * mag
    rt = RvddRuntime(arch, fut, 1, H, W, 0)
    rt.load_state_dict(sd)
    outs = []
    for t in range(1, T - fut):
        outs.append(rt.step(raw[t - 1][None] if t == 1 else None, raw[t][None], raw[t + 1][None] if fut else None,
                            s.flow_prev[t][None], s.flow_next[t][None] if fut else None).clone().cpu())
    rt.close()
    want = O.RecurrentOracle(sd, future=fut).run_sequence(raw.cpu(), s.flow_prev.cpu(), s.flow_next.cpu())
    for t, (got, ref) in enumerate(zip(outs, want)):
        assert torch.isfinite(got).all(), (mag, t)
        scale = float(ref.abs().max())
        err = float((got[0] - ref).abs().max())
        assert err < 1e-4 * scale, (arch, mag, t, err, scale)


@pytest.mark.parametrize("arch,stem", [("convunet", "recurrent-convunet-iso3200"), ("convunet+feat", "recurrent-convunet+feat-iso3200")])
def test_set_state_previous_output_of_another_magnitude(arch, stem):
    """rvdd_set_state(lastden) hands in a previous output the runtime did not produce: the bound of max |network input| that the
    block floating point of the first convs rests on (netin_bound_kernel: raw frames + the words PostConvs left) must follow it.
    A previous output 4096 times brighter than the raw frames, alone and with features of that magnitude: the next frame within
    1e-4 of the oracle relative to its max-abs."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights(stem)
    feat = arch.endswith("feat")
    H, W = 64, 96
    s = synth.make_sequence(3, H, W, iso=3200, seed=9, device="cuda")
    rt = RvddRuntime(arch, 0, 1, H, W, 0)
    rt.load_state_dict(sd)
    orc = O.RecurrentOracle(sd, future=0)
    rt.step(s.raw[0][None], s.raw[1][None], None, s.flow_prev[1][None], None)
    orc.step(s.raw[0][None].cpu(), s.raw[1][None].cpu(), None, s.flow_prev[1][None].cpu(), None, first=True)
    den, f = rt.get_state()
    for with_feat in ((False, True) if feat else (False,)):
        big_den = den * 4096.0
        big_f = f * 4096.0 if with_feat else None
        rt.set_state(big_den, big_f)
        orc.lastden = big_den.cpu()
        if feat:
            orc.lastfeat = (big_f if with_feat else f).cpu()
        got = rt.step(None, s.raw[2][None], None, s.flow_prev[2][None], None).clone().cpu()
        ref = orc.step(s.raw[1][None].cpu(), s.raw[2][None].cpu(), None, s.flow_prev[2][None].cpu(), None, first=False)
        assert torch.isfinite(got).all()
        scale = float(ref.abs().max())
        assert float((got - ref).abs().max()) < 1e-4 * scale, (arch, with_feat, float((got - ref).abs().max()), scale)
        rt.set_state(den, f if feat else None)           # back to the state after step 1 for the next variant
        orc.lastden = den.cpu()
        if feat:
            orc.lastfeat = f.cpu()
    rt.close()


def test_split_path_mixed_magnitudes_in_one_batch():
    """Block floating point is per map AND per sequence: three sequences of one batch a factor 1e5 and 2^-10 apart.  Each is
    within 1e-4 of its own oracle relative to its own max-abs, and bit for bit what it is when it runs alone (a workgroup whose
    tiles span sequences that need the scaling and sequences that do not takes the scaled form of the tile loop for all of
    them: a multiplication by 1.0 for the in-domain ones, the same bits as the unscaled form)."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    H, W, T = 48, 80, 4
    mags = (1.0, 1.0e5, 2.0 ** -10)
    seqs = [synth.make_sequence(T, H, W, iso=3200, seed=60 + b, device="cuda") for b in range(3)]
    raws = [s.raw * m for s, m in zip(seqs, mags)]

    def run(idx):
        rt = RvddRuntime("convunet+feat", 0, len(idx), H, W, 0)
        rt.load_state_dict(sd)
        st = lambda f: torch.stack([f(b) for b in idx], 0)
        outs = [rt.step(st(lambda b: raws[b][t - 1]) if t == 1 else None, st(lambda b: raws[b][t]), None,
                        st(lambda b: seqs[b].flow_prev[t]), None).clone() for t in range(1, T)]
        rt.close()
        return outs

    together = run([0, 1, 2])
    for b in range(3):
        alone = run([b])
        want = O.RecurrentOracle(sd, future=0).run_sequence(raws[b].cpu(), seqs[b].flow_prev.cpu(), None)
        for t in range(T - 1):
            assert torch.equal(together[t][b], alone[t][0]), (b, t, float((together[t][b] - alone[t][0]).abs().max()))
            scale = float(want[t].abs().max())
            assert float((together[t][b].cpu() - want[t]).abs().max()) < 1e-4 * scale, (b, t, mags[b])


def test_many_sequences_per_workgroup():
    """Small frames, a large batch: a workgroup's tiles span more than four sequences (the kernel then takes the scaled form of
    its tile loop without looking the words up front) -- 40 sequences of 64x64, one of them 1e4 times brighter: every sequence
    equal, bit for bit, to the same sequence in a batch of its own, the bright one and two others within 1e-4 of the oracle."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights("recurrent-convunet+feat-iso3200")
    B, H, W, T = 40, 64, 64, 3
    seqs = [synth.make_sequence(T, H, W, iso=3200, seed=300 + (b % 5), device="cuda") for b in range(B)]
    mag = [1.0e4 if b == 17 else 1.0 for b in range(B)]

    def run(idx):
        rt = RvddRuntime("convunet+feat", 0, len(idx), H, W, 0)
        rt.load_state_dict(sd)
        st = lambda f: torch.stack([f(b) for b in idx], 0)
        outs = [rt.step(st(lambda b: seqs[b].raw[t - 1] * mag[b]) if t == 1 else None, st(lambda b: seqs[b].raw[t] * mag[b]), None,
                        st(lambda b: seqs[b].flow_prev[t]), None).clone() for t in range(1, T)]
        rt.close()
        return outs

    big = run(list(range(B)))
    for b in (0, 17, 39):
        small = run([b])
        want = O.RecurrentOracle(sd, future=0).run_sequence((seqs[b].raw * mag[b]).cpu(), seqs[b].flow_prev.cpu(), None)
        for t in range(T - 1):
            assert torch.equal(big[t][b], small[t][0]), (b, t)
            assert float((big[t][b].cpu() - want[t]).abs().max()) < 1e-4 * float(want[t].abs().max()), (b, t)
    # the same frames in different slots: the same bits
    assert torch.equal(big[1][0], big[1][5]) and torch.equal(big[1][3], big[1][38])


def test_composed_first_layer_matches_two_convs():
    """preprocessing_layer has no activation (networks/unet.py:742), so it and the first source of EncoderConvs[0][0] (:743) are
    one linear map of the network input: the default path runs them as ONE 5x5 conv with host-composed filters plus a fix of the
    border ring (the reference zero-pads BETWEEN the two convs).  Against the two convs one after the other (option "fuse_pre"
    0): the same map in another summation order -- max-abs < 5e-6 on frames and < 3e-5 on the features, over three recurrent
    steps, with and without a future frame, at sizes with ragged tiles, one-tile images (every pixel within two of the border)
    and batches; and the border ring itself (rows / columns 0, 1 and the last two) no worse than the interior."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    for stem, fut in (("recurrent-convunet+feat-iso3200", 0), ("recurrent-convunet+feat-future-iso12800", 1)):
        sd = load_weights(stem)
        for B, H, W in ((1, 16, 16), (2, 72, 104), (1, 180, 320), (3, 50, 66)):
            T = 4 + fut
            seqs = [synth.make_sequence(T, H, W, iso=3200, seed=1200 + b, device="cuda") for b in range(B)]
            st = lambda f: torch.stack([f(s) for s in seqs], 0)
            outs = []
            for fuse in (1, 0):
                rt = RvddRuntime("convunet+feat", fut, B, H, W, 0)
                rt.set_option("fuse_pre", fuse)
                rt.load_state_dict(sd)
                o = []
                for t in range(1, T - fut):
                    o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]),
                                     st(lambda s: s.raw[t + 1]) if fut else None, st(lambda s: s.flow_prev[t]),
                                     st(lambda s: s.flow_next[t]) if fut else None).clone())
                o.append(rt.get_state()[1])
                outs.append(o)
                rt.close()
            for k, (a, b) in enumerate(zip(*outs)):
                d = (a - b).abs()
                bar = 3e-5 if k == len(outs[0]) - 1 else 5e-6      # (features reach 8: 3e-5 is 4e-6 of their range)
                assert float(d.max()) < bar, (stem, B, H, W, k, float(d.max()))
                ring = torch.ones_like(d, dtype=torch.bool)
                ring[..., 2:-2, 2:-2] = False
                if (~ring).any():
                    assert float(d[ring].max()) <= max(4 * float(d[~ring].max()), 1e-6), (stem, B, H, W, k, float(d[ring].max()), float(d[~ring].max()))



def test_pipelined_convblock_equals_phased():
    """convblock_pipe_kernel (the default: waves 0-3 run the depth-wise conv and the LayerNorm of tile t + 1 while waves
    4-7 run the MLP of tile t, hand-over through the halo buffers behind two workgroup barriers, the front waves' own
    LDS-counter barrier around their halo requests) against convblock_kernel (option next_pipe = 0: the same phases one
    after the other in all eight waves): the same arithmetic per pixel in the same order, so the same bits -- plain,
    pooling and 1x1-output variants, sizes with one tile, ragged tiles, more tiles than workgroups' first round, batches."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if "next-feat-future-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    arch, fut = "next+feat", 1
    sd = load_weights(VARIANTS["next-feat-future-iso3200"][0])
    for B, H, W in ((1, 16, 16), (3, 22, 130), (2, 130, 22), (1, 50, 66), (2, 72, 104), (1, 256, 256), (4, 360, 640)):
        T = 4
        seqs = [synth.make_sequence(T, H, W, iso=3200, seed=660 + b, device="cuda") for b in range(B)]
        st = lambda f: torch.stack([f(s) for s in seqs], 0)
        outs = []
        for pipe in (1, 0):
            rt = RvddRuntime(arch, fut, B, H, W, 0)
            rt.set_option("next_pipe", pipe)
            rt.set_option("next_projfuse", 0)        # the projection halves exist in the pipelined kernel only: same schedule on both sides
            rt.load_state_dict(sd)
            o = []
            for t in range(1, T - fut):
                o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]),
                                 st(lambda s: s.raw[t + 1]), st(lambda s: s.flow_prev[t]), st(lambda s: s.flow_next[t])).clone())
            outs.append((o, rt.get_state()[1].clone()))
            rt.close()
        for a, b in zip(outs[0][0], outs[1][0]):
            assert torch.equal(a, b), (B, H, W, float((a - b).abs().max()))
        assert torch.equal(outs[0][1], outs[1][1]), (B, H, W)


@pytest.mark.parametrize("arch,stem,fut", [("convunet", "recurrent-convunet-iso3200", 0), ("convunet+feat", "recurrent-convunet+feat-future-iso12800", 1)])
def test_conv_output_channel_split_same_bits(arch, stem, fut):
    """Launches of the split-f16 conv kernel with at most a third of a 16x16 tile per compute unit (the coarse levels of a small
    sequence) give each tile to THREE workgroups of 16 output channels (conv3x3h.hip MT = 1; option cout_split 0: one workgroup,
    48 channels): the same sums per output channel in the same order -- frames and features bit for bit.  Sizes whose levels
    fall on both sides of the threshold, ragged tiles, zero-padded decoder levels (odd level sizes), batches; every epilogue
    (plain, pooling, two-pass, fused upsample, bottleneck sum) takes the split at some level."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    sd = load_weights(stem)
    for B, H, W in ((1, 256, 256), (1, 64, 96), (2, 72, 104), (1, 36, 52), (3, 22, 130), (1, 360, 640)):
        T = 3 + fut
        seqs = [synth.make_sequence(T, H, W, iso=3200, seed=690 + b, device="cuda") for b in range(B)]
        st = lambda f: torch.stack([f(s) for s in seqs], 0)
        outs = []
        try:
            for split in (1, 0):
                rt = RvddRuntime(arch, fut, B, H, W, 0)
                rt.set_option("cout_split", split)
                rt.load_state_dict(sd)
                o = []
                for t in range(1, T - fut):
                    o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]),
                                     st(lambda s: s.raw[t + 1]) if fut else None, st(lambda s: s.flow_prev[t]),
                                     st(lambda s: s.flow_next[t]) if fut else None).clone())
                outs.append((o, rt.get_state()[1]))
                rt.close()
        finally:
            from rvdd_release_amd.util._ops import ops_runtime
            ops_runtime(0).set_option("cout_split", 1)          # harmless: the option is per handle
        for a, b in zip(outs[0][0], outs[1][0]):
            assert torch.equal(a, b), (arch, B, H, W, float((a - b).abs().max()))
        if outs[0][1] is not None:
            assert torch.equal(outs[0][1], outs[1][1]), (arch, B, H, W)


def test_projection_halves_equal_projection_kernel():
    """The 96 -> 48 projection behind cat((x_dec, x_enc)) (networks/new_unet.py:321-329, 85-88) as two 48 -> 48 halves in the
    epilogues of the blocks that form x_enc and x_dec (the default) against proj1x1_kernel on the concatenated maps (option
    next_projfuse = 0): the same linear map, the halves on the F16 matrix pipe with operands split per pixel in block floating
    point, summed in another order -- frames and recurrent features within 5e-6 of each other's maximum (observed: 2.2e-6 after two
    recurrent steps; the split-f16 and the f32-MFMA blocks differ by as much).  Sizes where every
    decoder level fuses, where zero_pad_features keeps some levels on the kernel (odd level sizes), ragged tiles, batches."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if "next-feat-future-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    arch, fut = "next+feat", 1
    sd = load_weights(VARIANTS["next-feat-future-iso3200"][0])
    for B, H, W in ((1, 16, 16), (3, 24, 136), (2, 130, 22), (1, 50, 66), (2, 72, 104), (1, 256, 256), (2, 360, 640)):
        T = 4
        seqs = [synth.make_sequence(T, H, W, iso=3200, seed=670 + b, device="cuda") for b in range(B)]
        st = lambda f: torch.stack([f(s) for s in seqs], 0)
        outs = []
        for fuse in (1, 0):
            rt = RvddRuntime(arch, fut, B, H, W, 0)
            rt.set_option("next_projfuse", fuse)
            rt.load_state_dict(sd)
            o = []
            for t in range(1, T - fut):
                o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]),
                                 st(lambda s: s.raw[t + 1]), st(lambda s: s.flow_prev[t]), st(lambda s: s.flow_next[t])).clone())
            outs.append((o, rt.get_state()[1].clone()))
            rt.close()
        for a, b in zip(outs[0][0] + [outs[0][1]], outs[1][0] + [outs[1][1]]):
            assert float((a - b).abs().max()) <= 5e-6 * max(1.0, float(b.abs().max())), (B, H, W, float((a - b).abs().max()))
    # the feature warp's half (warp48_proj_kernel) on flows that leave the frame and differ from pixel to pixel: clamped taps, pixel
    # pairs whose footprints do not line up -- against warp48_kernel + the projection kernel
    B, H, W, T = 2, 72, 104, 4
    gen = torch.Generator(device="cpu").manual_seed(5)
    seqs = [synth.make_sequence(T, H, W, iso=3200, seed=680 + b, device="cuda") for b in range(B)]
    st = lambda f: torch.stack([f(s) for s in seqs], 0)
    wild = lambda fl: fl * 6.0 + (torch.randn(fl.shape, generator=gen) * 9.0).cuda()
    fp = {t: wild(st(lambda s: s.flow_prev[t])) for t in range(1, T - fut)}
    outs = []
    for fuse in (1, 0):
        rt = RvddRuntime(arch, fut, B, H, W, 0)
        rt.set_option("next_projfuse", fuse)
        rt.load_state_dict(sd)
        o = [rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]), st(lambda s: s.raw[t + 1]), fp[t],
                     st(lambda s: s.flow_next[t])).clone() for t in range(1, T - fut)]
        outs.append(o + [rt.get_state()[1].clone()])
        rt.close()
    for a, b in zip(*outs):      # (frames of this chaos are rougher and the rounding of the two summation orders shows more: observed 9e-6)
        assert torch.isfinite(a).all() and float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def test_pooling_epilogue_equals_maxpool_kernel():
    """MaxPool2d(2) in front of each DownConv (networks/new_unet.py:200-204) written from the epilogue of the fused
    ConvBlock ahead of it (the default) against the separate pooling kernel (option next_pool = 0): a maximum has no
    rounding, so the outputs and the recurrent features are bit-identical -- at sizes whose levels have odd heights
    and widths (floor semantics), ragged tiles, levels smaller than a tile, and batches."""
    from rvdd_release_amd import synth
    from rvdd_release_amd.runtime import RvddRuntime
    if "next-feat-future-iso3200" not in BUILT:
        pytest.skip("ConvNeXt path not built")
    arch, fut = "next+feat", 1
    sd = load_weights(VARIANTS["next-feat-future-iso3200"][0])
    for B, H, W in ((1, 16, 16), (3, 22, 130), (2, 130, 22), (1, 50, 66), (2, 72, 104), (1, 180, 320)):
        T = 4
        seqs = [synth.make_sequence(T, H, W, iso=3200, seed=650 + b, device="cuda") for b in range(B)]
        st = lambda f: torch.stack([f(s) for s in seqs], 0)
        outs = []
        for pool in (1, 0):
            rt = RvddRuntime(arch, fut, B, H, W, 0)
            rt.set_option("next_pool", pool)
            rt.set_option("next_projfuse", 0)        # (they ride in the pooling blocks' epilogues: same schedule on both sides)
            rt.load_state_dict(sd)
            o = []
            for t in range(1, T - fut):
                o.append(rt.step(st(lambda s: s.raw[t - 1]) if t == 1 else None, st(lambda s: s.raw[t]),
                                 st(lambda s: s.raw[t + 1]), st(lambda s: s.flow_prev[t]), st(lambda s: s.flow_next[t])).clone())
            outs.append((o, rt.get_state()[1].clone()))
            rt.close()
        for a, b in zip(outs[0][0], outs[1][0]):
            assert torch.equal(a, b), (B, H, W, float((a - b).abs().max()))
        assert torch.equal(outs[0][1], outs[1][1]), (B, H, W)
