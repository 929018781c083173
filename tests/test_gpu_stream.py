"""Raw footage on the device: rvdd_ingest_raw against its numpy restatement, rvdd_video_push against the existing entry
points it composes (ingest -> TV-L1 batch -> reset -> step), slot independence, the ctl errors, and the denoise command
line against validate.main on the same frames on disk.  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from conftest import WEIGHTS
from gpu_support import files_of, make_runtime as _runtime, ops_rt, same
from stream_compose import CASES, FIRST, IDLE, NEXT, compose, mid_stream_schedule, push_alone as _stream_alone, push_schedule
from stream_compose import synth_video as _video
from stream_ref import ingest_ref, mosaic_of, quantised_dn, to_gpu

pytestmark = pytest.mark.gpu


# ---- 5. the ingest kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hh,ww", [(18, 26), (128, 128), (360, 640)])
@pytest.mark.parametrize("bit_depth", [10, 12, 14])
def test_ingest_raw_is_the_restatement(hh, ww, bit_depth):
    rt = ops_rt()
    rng = np.random.default_rng(hh * 100 + bit_depth)
    top = 2 ** bit_depth - 1
    for n in (1, 8):
        cells = rng.integers(0, top + 1, size=(n, hh, ww, 4)).astype(np.float32)
        cells[0, 0, 0, :] = 0
        cells[-1, -1, -1, :] = top
        cells[0, hh // 2, :4, :] = np.array([[0, top, top, 0], [top, top, top, top], [1, 0, 0, 0], [top - 1, top, 0, 1]], np.float32)
        for layout in ("mosaic", "packed_hwc"):
            host = mosaic_of(cells) if layout == "mosaic" else cells
            for dtype in (np.uint16, np.float32):
                frames = host.astype(dtype)
                want_p, want_g = (torch.from_numpy(a) for a in ingest_ref(frames, layout, bit_depth))
                dev = to_gpu(frames)
                p, g = rt.ingest_raw(dev, bit_depth, layout)
                assert torch.equal(p.cpu(), want_p) and torch.equal(g.cpu(), want_g), (n, layout, dtype)
                p1, g1 = rt.ingest_raw(dev, bit_depth, layout, want_gray=False)
                p2, g2 = rt.ingest_raw(dev, bit_depth, layout, want_packed=False)
                assert g1 is None and p2 is None and torch.equal(p1.cpu(), want_p) and torch.equal(g2.cpu(), want_g)
                if dtype == np.uint16 and hasattr(torch, "uint16"):
                    p3, g3 = rt.ingest_raw(dev.view(torch.uint16), bit_depth, layout)
                    assert torch.equal(p3, p) and torch.equal(g3, g)
        # frames that do not start on a 16-byte boundary take the one-cell form: same bits
        odd = to_gpu(np.concatenate([np.zeros(1, np.uint16), mosaic_of(cells).astype(np.uint16).ravel()]))[1:].view(n, 2 * hh, 2 * ww)
        p, g = rt.ingest_raw(odd, bit_depth, "mosaic")
        want_p, want_g = (torch.from_numpy(a) for a in ingest_ref(mosaic_of(cells), "mosaic", bit_depth))
        assert torch.equal(p.cpu(), want_p) and torch.equal(g.cpu(), want_g)


def test_ingest_raw_bad_arguments():
    rt = ops_rt()
    f = torch.zeros(1, 32, 32, dtype=torch.int16, device="cuda")
    for bd in (0, 17, -1):
        with pytest.raises(RuntimeError, match=r"\(-1\).*bit_depth"):
            rt.ingest_raw(f, bd)
    for dtype, layout in ((2, 0), (-1, 0), (0, 2), (0, -1)):
        rc = rt.lib.rvdd_ingest_raw(rt.h, f.data_ptr(), dtype, layout, 1, 16, 16, 12, None, None, None)
        assert rc == -1 and (b"dtype" in rt.lib.rvdd_last_error(rt.h) or b"layout" in rt.lib.rvdd_last_error(rt.h))
    with pytest.raises(RuntimeError, match="uint16"):
        rt.ingest_raw(f.to(torch.int32))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        rt.ingest_raw(f.cpu())


# ---- 6. the stream is the composition ------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,stem,future,options", CASES, ids=[f"{c[1]}-{'-'.join(c[3]) or 'plain'}" for c in CASES])
def test_stream_is_the_composition(arch, stem, future, options):
    H, W, T = 64, 96, 6
    video = _video(T, H, W, seed=31 + future)
    a = _runtime(arch, stem, future, 1, H, W, **options)
    b = _runtime(arch, stem, future, 1, H, W, **{k: v for k, v in options.items() if k != "stream_reset_each"})
    got, flags = _stream_alone(a, video, future)
    want = compose(b, video, future, no_warp=bool(options.get("no_warp")), reset_each=bool(options.get("stream_reset_each")))
    assert flags == [False] * (1 + future) + [True] * (T - 1 - future)
    assert len(got) == len(want) == T - 1 - future
    same(got, want)
    a.set_option("tvl1_async", 0)            # the deferred check of the pushes' flow batches: nothing gave up
    if options.get("stream_reset_each"):
        # ... and the option matters: the same pushes without it carry the recurrence on, which is another output
        c = _runtime(arch, stem, future, 1, H, W)
        other, _ = _stream_alone(c, video, future)
        assert torch.equal(other[0], got[0]) and not torch.equal(other[-1], got[-1])


# ---- 7. slots are independent --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("future", [0, 1])
def test_slots_are_independent(future):
    from rvdd_release_amd.denoise import deal_slots
    H, W, B = 64, 96, 3
    stem = "recurrent-convunet+feat-future-iso12800" if future else "recurrent-convunet+feat-iso3200"
    lengths = (6, 3, 7, 4, 4)
    videos = [_video(n, H, W, seed=40 + v) for v, n in enumerate(lengths)]
    rt = _runtime("convunet+feat", stem, future, B, H, W)
    steps = deal_slots(lengths, B)
    pushed = push_schedule(rt, videos, steps)
    for step, valid in zip(steps, pushed.flags):
        assert valid == [c != IDLE and k >= 1 + future for c, _, k in step], step
    rt.set_option("tvl1_async", 0)
    alone = _runtime("convunet+feat", stem, future, 1, H, W)
    for v, n in enumerate(lengths):
        want, _ = _stream_alone(alone, videos[v], future)
        assert len(want) == n - 1 - future
        same(pushed.by_video[v], want, v)


def test_slots_are_independent_720p_batch_8():
    """The launch shapes the benchmark uses: 720p, B = 8, a future frame; a FIRST mid-stream in one slot."""
    H, W, B, future, T = 720, 1280, 8, 1, 4
    stem = "recurrent-convunet+feat-future-iso12800"
    videos = [_video(T, H, W, seed=50 + v, iso=12800, device="cuda") for v in range(B)]
    short = _video(3, H, W, seed=70, iso=12800, device="cuda")
    rt = _runtime("convunet+feat", stem, future, B, H, W)
    steps = mid_stream_schedule(B, T)
    pushed = push_schedule(rt, videos + [short], steps)
    for step, valid in zip(steps, pushed.flags):
        assert valid == [c != IDLE and k >= 2 for c, _, k in step], step
    rt.set_option("tvl1_async", 0)
    del rt
    alone = _runtime("convunet+feat", stem, future, 1, H, W)
    for b in (0, 5, 7):
        want, _ = _stream_alone(alone, videos[b], future)
        assert len(want) == T - 2
        same(pushed.by_video[b], want, b)


# ---- 8. ctl errors ---------------------------------------------------------------------------------------------------------
def test_ctl_errors_change_nothing():
    H, W, B = 64, 96, 2
    stem = "recurrent-convunet+feat-iso3200"
    videos = [_video(4, H, W, seed=60 + v) for v in range(2)]
    rt = _runtime("convunet+feat", stem, 0, B, H, W)
    frames = lambda t: to_gpu(np.stack([videos[0][t], videos[1][t]]))

    def push(t, ctl):
        return rt.video_push(frames(t), ctl, 12, "mosaic")

    with pytest.raises(RuntimeError, match=r"\(-2\).*slot 0"):           # NEXT before any FIRST (ctl = None: all NEXT)
        push(0, None)
    with pytest.raises(RuntimeError, match=r"\(-2\).*slot 1"):
        push(0, [FIRST, NEXT])
    got = {0: [], 1: []}
    out, valid = push(0, [FIRST, FIRST])
    assert valid == [False, False]
    out, valid = push(1, [NEXT, IDLE])
    assert valid == [True, False]
    got[0].append(out[0:1].clone())
    with pytest.raises(RuntimeError, match=r"\(-2\).*slot 1.*idle"):     # NEXT after IDLE: nothing is changed ...
        push(2, [NEXT, NEXT])
    for bad in ([NEXT, 3], [7, IDLE]):
        with pytest.raises(RuntimeError, match=r"\(-1\).*ctl"):
            push(2, bad)
    out, valid = push(2, [NEXT, FIRST])                                  # ... so the stream goes on with the right bits
    assert valid == [True, False]
    got[0].append(out[0:1].clone())
    # slot 1 restarts its video at frame 2 here: a video of its own, frames 2 .. 3
    out, valid = push(3, [NEXT, NEXT])
    assert valid == [True, True]
    got[0].append(out[0:1].clone())
    got[1].append(out[1:2].clone())
    for bd, dtype, layout in ((0, 0, 0), (17, 0, 0), (12, 2, 0), (12, 0, 5)):
        v = (__import__("ctypes").c_uint8 * B)()
        rc = rt.lib.rvdd_video_push(rt.h, frames(0).data_ptr(), dtype, layout, bd, None, out.data_ptr(), v, None)
        assert rc == -1, (bd, dtype, layout)
    alone = _runtime("convunet+feat", stem, 0, 1, H, W)
    want0, _ = _stream_alone(alone, videos[0], 0)
    want1, _ = _stream_alone(alone, videos[1][2:], 0)
    assert len(want0) == 3 and len(want1) == 1
    assert all(torch.equal(g, w) for g, w in zip(got[0], want0)) and torch.equal(got[1][0], want1[0])
    with pytest.raises(RuntimeError, match="slots of"):
        rt.video_push(to_gpu(np.zeros((B, 32, 32), np.uint16)))


def test_push_refuses_sizes_tvl1_does_not_take():
    stem = "recurrent-convunet-iso3200"
    rt = _runtime("convunet", stem, 0, 1, 16, 64)                        # 8 x 32 cells: below TV-L1's 16 x 16
    f = to_gpu(np.zeros((1, 16, 64), np.uint16))
    with pytest.raises(RuntimeError, match=r"\(-1\).*rvdd_tvl1flow_batch"):
        rt.video_push(f, [FIRST])
    rt.set_option("no_warp", 1)
    for t in range(3):
        out, valid = rt.video_push(f, [FIRST if t == 0 else NEXT])
        assert valid == [t >= 1]
    assert torch.isfinite(out).all()


# ---- 10. a handle that has streamed steps as before ----------------------------------------------------------------------
def test_streamed_handle_still_steps_like_a_fresh_one():
    from rvdd_release_amd import synth
    H, W = 64, 96
    stem = "recurrent-convunet+feat-iso3200"
    seq = synth.make_sequence(4, H, W, iso=3200, seed=77)
    raw, fl = seq.raw.cuda(), seq.flow_prev.cuda()

    def steps(rt):
        rt.reset()
        return [rt.step(raw[t - 1][None], raw[t][None], None, fl[t][None], None).clone() for t in range(1, 4)]

    a = _runtime("convunet+feat", stem, 0, 1, H, W)
    _stream_alone(a, _video(5, H, W, seed=78), 0)
    got, want = steps(a), steps(_runtime("convunet+feat", stem, 0, 1, H, W))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # and the stream goes on afterwards (its kept frames were not touched): FIRST starts a video as on any handle
    v = _video(3, H, W, seed=79)
    again, _ = _stream_alone(a, v, 0)
    fresh, _ = _stream_alone(_runtime("convunet+feat", stem, 0, 1, H, W), v, 0)
    assert len(again) == 2 and all(torch.equal(g, w) for g, w in zip(again, fresh))


# ---- 9. on disk, against validate.py ---------------------------------------------------------------------------------------
def _write_three_ways(root, cells_per_video):
    """Whole-DN 12-bit frames: the reference layout ([h,w,4] float32, a dummy ground truth, NO flow folder), the same frames
    as 4-channel uint16, and as 1-channel uint16 mosaics."""
    from rvdd_release_amd import tiffio
    for v, cells in enumerate(cells_per_video):
        key = "%03d" % v
        dirs = {k: os.path.join(root, k, key) for k in ("noisy_f32", "gt_rgb", "noisy_u16x4", "noisy_mosaic")}
        for d in dirs.values():
            os.makedirs(d)
        for t in range(cells.shape[0]):
            code = "%08d" % (3 * t)
            tiffio.write(os.path.join(dirs["noisy_f32"], code + ".tiff"), cells[t])
            tiffio.write(os.path.join(dirs["gt_rgb"], code + ".tiff"), np.full((2 * cells.shape[1], 2 * cells.shape[2], 3), 1000, np.uint16))
            tiffio.write(os.path.join(dirs["noisy_u16x4"], code + ".tiff"), cells[t].astype(np.uint16))
            tiffio.write(os.path.join(dirs["noisy_mosaic"], code + ".tiff"), mosaic_of(cells[t:t + 1])[0].astype(np.uint16))


@pytest.mark.parametrize("future", [0, 1])
def test_denoise_main_writes_what_validate_writes(tmp_path, future):
    from rvdd_release_amd import denoise, synth, validate
    from rvdd_release_amd.library import iio_read
    H, W = 64, 96
    iso = 12800 if future else 3200
    name = "recurrent-convunet+feat-future-iso12800" if future else "recurrent-convunet+feat-iso3200"
    net = "convunet-mode=fixedfeatures+feat"
    lengths = (4, 3, 5, 3)
    cells = [quantised_dn(synth.make_sequence(n, H, W, iso=iso, seed=90 + v).raw) for v, n in enumerate(lengths)]
    root = str(tmp_path / "data")
    _write_three_ways(root, cells)
    model_flags = ["--netDenoiser", net, "--path2epoch", os.path.join(WEIGHTS, name), "--feature_rec", "--future_patch_depth", str(future)]
    ck = tmp_path / "ck"
    validate.main(model_flags + ["--val_dataroot", root, "--nFolder", "noisy_f32", "--gt_linear_RGB_Folder", "gt_rgb", "--suffix", "t",
                                 "--checkpoints_dir", str(ck), "--val_videos", ",".join("%03d" % v for v in range(len(lengths)))])
    assert os.path.isdir(os.path.join(root, "flow"))                     # validate's --check_data pass computed the flow files
    want = {k: b for k, b in files_of(str(ck / f"recurrent-{net}-warp-i3o3-t" / "val_visuals")).items() if k.endswith("_denoised.tif")}
    assert len(want) == sum(n - 1 - future for n in lengths)
    for folder in ("noisy_f32", "noisy_u16x4", "noisy_mosaic"):
        for B in (1, 3):
            res = tmp_path / f"res_{folder}_{B}"
            srgb = folder == "noisy_mosaic" and B == 3
            stats = denoise.main(model_flags + ["--dataroot", root, "--nFolder", folder, "--results_dir", str(res), "--batch_size", str(B)]
                                 + (["--srgb", "%d,1.3,1.9,1.5" % iso] if srgb else []))
            got = files_of(str(res))
            tifs = {k: b for k, b in got.items() if k.endswith("_denoised.tif")}
            assert sorted(tifs) == sorted(want), (folder, B)
            assert all(tifs[k] == want[k] for k in want), (folder, B, [k for k in want if tifs[k] != want[k]])
            assert stats["frames"] == len(want)
            if srgb:
                pngs = sorted(k for k in got if k.endswith("_srgb.png"))
                assert [k[:-len("_srgb.png")] for k in pngs] == sorted(k[:-len("_denoised.tif")] for k in want)
                for k in pngs[:3]:
                    img = torch.from_numpy(iio_read(str(res / (k[:-len("_srgb.png")] + "_denoised.tif")))).cuda()
                    u8 = ops_rt().ppipe(img[None], 1 / 1.3, 1.9, 1.5, iso, 8, "hwc")
                    assert np.array_equal(iio_read(str(res / k)), u8[0].cpu().numpy()), k
            else:
                assert not any(k.endswith(".png") for k in got)
    assert not os.path.isdir(os.path.join(root, "flow", "noisy_mosaic"))  # denoise wrote nothing beside its results
