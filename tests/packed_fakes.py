"""The fake dataset, loader and model of the packed-validation host tests: the model's output is a deterministic function of
(video, frame) and of its own per-slot recurrence, so a wrong FirstOfVideo changes the output."""
import os
from collections import OrderedDict

import torch

from rvdd_release_amd.data import _collate

# video name -> (frames, packed raw size h, w)
VIDEOS = OrderedDict([("000", (7, 4, 6)), ("001", (3, 4, 6)), ("002", (5, 3, 5)), ("003", (9, 4, 6)),
                      ("004", (4, 4, 6)), ("005", (2, 3, 5))])


class FakeDataset:
    """infer4recDataset's path index (where, videos_gt_path, patch_depth = 2: one sample per frame after the first)."""

    def __init__(self, root, videos=VIDEOS):
        self.patch_depth = 2
        self.n_paths = os.path.join(root, "noisy")
        self.where, self.videos_gt_path, self.videos_noisy_path, self.size = [], [], [], []
        self.loads = 0
        for v, (frames, h, w) in videos.items():
            first = len(self.videos_gt_path)
            self.where.extend(first + k for k in range(frames - 1))
            for f in range(frames):
                self.videos_gt_path.append(os.path.join(root, "gt", v, "%08d.tiff" % f))
                self.videos_noisy_path.append(os.path.join(root, "noisy", v, "%08d.tiff" % f))
                self.size.append((h, w))

    def __len__(self):
        return len(self.where)

    def __getitem__(self, i):
        self.loads += 1
        last = self.where[i] + 1
        h, w = self.size[last]
        v = int(os.path.basename(os.path.dirname(self.videos_gt_path[last])))
        f = int(os.path.splitext(os.path.basename(self.videos_gt_path[last]))[0])
        n = torch.full((8, h, w), 0.01 * f - 0.1 * v)
        n[:, 0, 0] = v
        n[:, 0, 1] = f
        gt = torch.full((6, 2 * h, 2 * w), 0.02 * f)
        return {'n': n, 'gt': gt, 'flow': torch.zeros(1, 2, h, w), 'gt_path': self.videos_gt_path[last],
                'n_path': self.videos_noisy_path[last]}


class FakeLoader:
    """CustomDatasetDataLoader at the validation settings."""

    def __init__(self, dataset, max_dataset_size=float("inf")):
        self.dataset = dataset
        self.max_dataset_size = max_dataset_size

    def __len__(self):
        return int(min(len(self.dataset), self.max_dataset_size))

    def __iter__(self):
        for i in range(len(self)):
            yield _collate(self.dataset[i])


class FakeModel:
    """recurrentModel's surface: per slot a recurrent counter (reset by FirstOfVideo) and the video it started on."""

    def __init__(self):
        self.isTrain, self.device, self._rt = False, torch.device("cpu"), None
        self.loss_names = ['L1', 'PSNR', 'Denoiser']
        self.optimizers = [type("Opt", (), {"param_groups": [{"lr": 0.5}]})()]
        self.state = {}

    def eval(self):
        pass

    def get_current_losses(self):
        return OrderedDict((k, float(getattr(self, 'loss_' + k, 0))) for k in self.loss_names)

    def set_input(self, data):
        self.data = data
        first = data['FirstOfVideo']
        self.per_slot = not isinstance(first, bool)
        self.first = [bool(x) for x in first.tolist()] if self.per_slot else [first]
        self.image_paths = data['n_path']

    def test(self):
        n = self.data['n']
        outs = []
        for b in range(n.shape[0]):
            v, f = float(n[b, 0, 0, 0]), float(n[b, 0, 0, 1])
            if self.first[b]:
                self.state[b] = (v, 0)
            start, count = self.state[b]
            self.state[b] = (start, count + 1)
            H, W = 2 * n.shape[2], 2 * n.shape[3]
            outs.append(torch.full((3, H, W), 0.001 * (100 * v + 10 * f + count) + 0.37 * start) - 0.5)
        self.denoised = torch.stack(outs)

    def compute_losses(self):
        gt = self.data['gt'][:, 3:6]
        per = []
        for b in range(gt.shape[0]):
            d = (self.denoised[b] - gt[b]).float()
            l1 = float(d.abs().mean()) * 100.0
            per.append({'L1': l1, 'PSNR': 10.0 / (1e-3 + float((d * d).mean())), 'Denoiser': l1})
        self.sample_losses = per
        for k in self.loss_names:
            setattr(self, 'loss_' + k, sum(p[k] for p in per) / len(per))

    def get_sample_losses(self):
        return list(self.sample_losses)

    def get_current_visuals(self):
        return OrderedDict(denoised=self.denoised)

    def get_image_paths(self):
        return self.image_paths


def _opt():
    from rvdd_release_amd.options import make_opt
    return make_opt()
