"""The validation driver of the reference (validate.py) on the HIP runtime.

* `compute_validation(model, val_dataset, opt, ...)` -- validate.py:54-114: per output frame `set_input` /
  `test` / `compute_losses`, `FirstOfVideo` latched on a change of video folder, losses averaged over the
  dataset and returned as {'L1_valLoss', 'PSNR_valLoss', 'Denoiser_valLoss', 'lr'}.
* `compute_flows_from_denoised(data, model, opt)` -- validate.py:16-38 (`--val_flow_from_denoised`): the flow
  towards the previous DENOISED frame, recomputed online: remosaick -> TV-L1 on the device (`rvdd_tvl1flow`).
* `compute_validation(..., batch_size=B)` (`--val_batch_size B`): the same frames, files, log lines and losses with the
  videos packed into B batch slots (data/packed.py) -- a slot restarts when its video ends, the others carry on.
* `compute_validation(..., batch_size=B, compact=True)` (`--val_compact_slots`): the same again, but a step holds only the
  live sequences, kept in the first slots by moving a sequence into a hole no video is left for (no discarded tail).
* `init_validation_dataloader(opt)` -- validate.py:40-52; `main(argv)` -- validate.py:117-153, so that
  `python -m rvdd_release_amd.validate <the flags of scripts/test-*.sh>` reads frames and flows from disk and
  writes `<checkpoints_dir>/<name>/val_visuals/<video>/<frame>_denoised.tif` + `output.log`.

`val_dataset` is any iterable of the dicts the reference's `infer4recDataset` yields through its loader
(data/infer4rec_dataset.py:226-230): 'n' [1,(2+f)*4,h,w], 'gt' [1,6,H,W], 'flow' [1,1+f,2,h,w], 'n_path', 'gt_path'.
"""
from __future__ import annotations

import copy
import os
import time
from typing import Callable, Dict, Iterable, Optional

import torch

from .util._ops import ops_runtime
from .util.Hamilton_Adam_demo import HamiltonAdam


def _pattern_of(model) -> str:
    """The Bayer pattern of the model's raw frames (--bayer_pattern): the re-mosaic of the previous output follows it, so
    that it lines up with the noisy frame it is matched against."""
    return getattr(model, "bayer_pattern", "gbrg")


def compute_flows_from_denoised(data: dict, model, opt) -> None:
    """Replace the flow towards the previous frame in data['flow'] by the TV-L1 flow from the current noisy frame
    to the re-mosaicked previous OUTPUT.

    The released reference cannot actually run this branch (it hands `remosaick` a squeezed 3-D tensor,
    validate.py:29-31 vs util/Hamilton_Adam_demo.py:237-238, and appends the same flow `opt.patch_depth - 1`
    times); this is its evident intent: ONE flow, shaped like the dataset's `data['flow']` ([1,1,2,h,w]).
    With a future frame (`--future_patch_depth 1`) the reference would in addition pair the NEXT noisy frame
    (`data['n'][0, -4:]`) with the previous output and leave the model without its second flow (an IndexError in
    recurrent_model.py:317); here the current frame is the second packed frame whatever follows it, and the flow
    towards the next frame -- which no output exists for yet -- stays the dataset's pre-computed one."""
    dev = model.device
    noisy_cur = data['n'][0, 4:8, :, :].to(dev, torch.float32)                       # packed raw, [-1,1]
    prev_out = HamiltonAdam(_pattern_of(model)).remosaick(model.denoised.to(dev))[0]
    # the reference hands (x+1)/2 images to CPPbridge, which reduces 4 channels to their mean (library.py:67-68, :165-167)
    target = ((noisy_cur + 1.0) / 2.0).mean(dim=0).contiguous()
    moving = ((prev_out + 1.0) / 2.0).mean(dim=0).contiguous()
    flow = ops_runtime(dev.index or 0).tvl1flow(target, moving)                     # moving(x + flow) ~ target(x)
    if getattr(opt, "future_patch_depth", 0):
        keep = data['flow'][:, 1:2].to(dev, torch.float32)                          # cur -> next, from the dataset
        data['flow'] = torch.cat((flow[None, None], keep), dim=1)
    else:
        data['flow'] = flow[None, None]


def init_validation_dataloader(opt):
    """validate.py:40-52: the validation view of the options, then the dataset."""
    from .data import create_dataset
    v = copy.deepcopy(opt)
    v.dataroot, v.dataset_mode, v.videos = opt.val_dataroot, opt.val_dataset_mode, opt.val_videos
    v.max_dataset_size = float("inf")
    v.num_threads, v.batch_size, v.serial_batches = 0, 1, True
    if hasattr(opt, 'model_patch_depth'):
        v.patch_depth = opt.model_patch_depth
    return create_dataset(v)


def compute_validation(model, val_dataset: Iterable[Dict], opt, on_frame: Optional[Callable] = None,
                       val_image_dir: Optional[str] = None, batch_size: int = 1, compact: bool = False) -> dict:
    """validate.py:54-114.  With `val_image_dir` (and a dataset made by `create_dataset`) every frame is written
    to <val_image_dir>/<video>/<frame>_denoised.tif and its losses appended to output.log, as the reference does;
    `on_frame(i, data, visuals, losses)` is an in-memory hook beside that.

    `batch_size` > 1: the videos packed into that many batch slots (`val_dataset` made by `create_dataset`, or a
    `data.packed.PackedLoader`).  Same files, same output.log lines in the same order, same returned losses; `on_frame`
    sees each frame once (data / visuals of its own slot, batch dimension 1), in the order the frames are computed.

    `compact` (with `batch_size` > 1): no slot steps on a repeated frame; see `data.packed.plan_packs`.  Same results again."""
    if batch_size > 1 or hasattr(val_dataset, "packs"):
        return _compute_validation_packed(model, val_dataset, opt, on_frame, val_image_dir, batch_size, compact)
    online_flow = (not model.isTrain) and bool(getattr(opt, "val_flow_from_denoised", False)) and not opt.no_warp
    was_training = model.isTrain
    model.isTrain = False
    model.eval()
    totals = {name: 0.0 for name in model.get_current_losses()}
    frames = 0
    previous_video = ''
    with torch.no_grad():
        for i, data in enumerate(val_dataset):
            video = os.path.dirname(data['gt_path'][0])
            data['FirstOfVideo'] = video != previous_video
            previous_video = video
            if online_flow and not data['FirstOfVideo']:
                compute_flows_from_denoised(data, model, opt)
            model.set_input(data)
            model.test()
            model.compute_losses()
            losses = model.get_current_losses()
            if on_frame is not None:
                on_frame(i, data, model.get_current_visuals(), losses)
            if val_image_dir is not None:
                _write_frame(model, val_dataset, val_image_dir, i, losses)
            for name, value in losses.items():
                totals[name] += value
            frames += 1
    result = {name + "_valLoss": total / max(frames, 1) for name, total in totals.items()}
    result['lr'] = model.optimizers[0].param_groups[0]['lr']
    model.isTrain = was_training
    return result


def _slot(data: dict, b: int) -> dict:
    """Slot b of a packed step as the serial loader would have yielded it (batch dimension 1)."""
    out = {}
    for k, v in data.items():
        if k in ('slots', 'moves', 'prev_index'):        # bookkeeping of a compact step: the serial loader has none
            continue
        if torch.is_tensor(v) and v.dim() >= 1 and k not in ('FirstOfVideo', 'live'):
            out[k] = v[b:b + 1]
        elif isinstance(v, list) and len(v) == len(data['index']):
            out[k] = [v[b]]
        else:
            out[k] = v
    out['FirstOfVideo'] = bool(data['FirstOfVideo'][b])
    return out


def _flows_from_denoised_packed(data: dict, model, opt, rt) -> None:
    """compute_flows_from_denoised for the live slots that continue a video, with ONE rvdd_tvl1flow_batch (bit for bit
    the single calls).  The images are formed per slot exactly as the serial path forms them; the other slots keep the
    dataset's flow, as a first frame does in serial mode.  A compact step names, per sequence, its index in the previous
    step's batch ('prev_index'): a sequence that was moved to another slot finds its previous output there."""
    live, first = data['live'].tolist(), data['FirstOfVideo'].tolist()
    prev_index = data.get('prev_index')
    sel = [b for b in range(len(live)) if live[b] and not first[b]]
    if not sel:
        return
    dev = model.device
    ha = HamiltonAdam(_pattern_of(model))
    targets, movings = [], []
    for b in sel:
        noisy_cur = data['n'][b, 4:8, :, :].to(dev, torch.float32)
        p = b if prev_index is None else int(prev_index[b])
        prev_out = ha.remosaick(model.denoised[p:p + 1].to(dev))[0]
        targets.append(((noisy_cur + 1.0) / 2.0).mean(dim=0))
        movings.append(((prev_out + 1.0) / 2.0).mean(dim=0))
    flows = rt.tvl1flow_batch(torch.stack(targets).contiguous(), torch.stack(movings).contiguous())
    flow = data['flow'].to(dev, torch.float32).clone()
    flow[sel, 0] = flows
    data['flow'] = flow


def _compute_validation_packed(model, val_dataset, opt, on_frame, val_image_dir, batch_size, compact=False) -> dict:
    from .data.packed import PackedLoader
    loader = val_dataset if hasattr(val_dataset, "packs") else PackedLoader(val_dataset, batch_size, compact=compact)
    online_flow = (not model.isTrain) and bool(getattr(opt, "val_flow_from_denoised", False)) and not opt.no_warp
    was_training = model.isTrain
    model.isTrain = False
    model.eval()
    names = list(model.get_current_losses())
    per_frame: Dict[int, dict] = {}
    log_next = 0                 # output.log gets the lines of frames 0 .. log_next - 1, in serial order
    async_rts = []
    with torch.no_grad():
        for data in loader:
            if online_flow and model._rt is not None and not bool(data['FirstOfVideo'].all()):
                if model._rt not in async_rts:
                    model._rt.set_option("tvl1_async", 1)      # the flow batch stays on the stream until the losses' sync
                    async_rts.append(model._rt)
                _flows_from_denoised_packed(data, model, opt, model._rt)
            model.set_input(data)
            model.test()
            model.compute_losses()
            samples = model.get_sample_losses()
            for b, i in enumerate(data['index']):
                if not bool(data['live'][b]):
                    continue
                losses = {name: samples[b][name] for name in names}
                per_frame[i] = losses
                if on_frame is not None or val_image_dir is not None:
                    visuals = {name: v[b:b + 1] for name, v in model.get_current_visuals().items()}
                if on_frame is not None:
                    on_frame(i, _slot(data, b), visuals, losses)
                if val_image_dir is not None:
                    _save_frame(loader.dataset, val_image_dir, i, visuals, data['n_path'][b])
            if val_image_dir is not None:
                log_next = _flush_log(val_image_dir, per_frame, log_next)
    for rt in async_rts:
        rt.set_option("tvl1_async", 0)           # reports a failed pending batch
    totals = {name: 0.0 for name in names}
    for i in sorted(per_frame):                  # serial frame order: the same sums as compute_validation at B = 1
        for name in names:
            totals[name] += per_frame[i][name]
    result = {name + "_valLoss": total / max(len(per_frame), 1) for name, total in totals.items()}
    result['lr'] = model.optimizers[0].param_groups[0]['lr']
    model.isTrain = was_training
    return result


def _save_frame(dataset, val_image_dir, i, visuals, n_path):
    """_write_frame's TIFF for one slot of a packed step."""
    from .library import pathdiff
    from .util.visualizer import save_images
    if i % 40 == 0:
        print('processing (%04d)-th image... %s' % (i, [n_path]))
    save_images(val_image_dir, visuals, [os.path.basename(n_path)], subfolder=pathdiff(n_path, dataset.n_paths))


def _flush_log(val_image_dir, per_frame, log_next):
    """_write_frame's output.log lines of the frames that now follow the last line written without a gap."""
    from .library import print_dict
    while log_next in per_frame:
        print_dict(per_frame[log_next], suffix="", savefile=os.path.join(val_image_dir, "output.log"))
        log_next += 1
    return log_next


def _write_frame(model, val_dataset, val_image_dir, i, losses):
    """validate.py:88-103: the visuals as TIFF under the video's folder, the losses as one line of output.log."""
    from .library import pathdiff, print_dict
    from .util.visualizer import save_images
    img_path = model.get_image_paths()
    if i % 40 == 0:
        print('processing (%04d)-th image... %s' % (i, img_path))
    save_images(val_image_dir, model.get_current_visuals(), [os.path.basename(img_path[0])],
                subfolder=pathdiff(img_path[0], val_dataset.dataset.n_paths))
    print_dict(losses, suffix="", savefile=os.path.join(val_image_dir, "output.log"))


def main(argv=None) -> dict:
    """validate.py:117-153: options -> dataset -> model -> validation -> averaged losses."""
    from .models import create_model
    from .options import parse
    opt = parse(argv)
    val_dataset = init_validation_dataloader(opt)
    print('Number of validation images = %d' % len(val_dataset))
    model = create_model(opt)
    model.setup(opt)
    opt.isTrain = model.isTrain = False
    t0 = time.time()
    val_losses = compute_validation(model, val_dataset, opt,
                                    val_image_dir=os.path.join(opt.checkpoints_dir, opt.name, "val_visuals"),
                                    batch_size=int(getattr(opt, "val_batch_size", 1)),
                                    compact=bool(getattr(opt, "val_compact_slots", False)))
    dt = time.time() - t0
    print('(validation, %d images, %.3f s, %.2f frames/s) ' % (len(val_dataset), dt, len(val_dataset) / max(dt, 1e-9))
          + ', '.join('%s: %.3f' % kv for kv in val_losses.items()))
    return val_losses


if __name__ == '__main__':
    main()
