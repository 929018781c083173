"""`--dataset_mode rawvideo`: footage as a camera leaves it,

    <dataroot>/<nFolder>/<video>/<frame>.tif[f] ,

and nothing else: no ground truth, no flow or warp folder (the flows of such footage are computed on the device,
`RvddRuntime.video_push`).  A frame is one plane of sensor values (a 1-channel TIFF: the Bayer mosaic, [2h,2w]) or the
reference dataset's packed form (4 channels, [h,w,4], channel k = CFA position (k >> 1, k & 1) of each 2x2 cell), as
`uint16` or `float32` digital numbers.  The first frame of the first video decides which; a later frame of another
kind is an error that names the file.

One sample, in video order:
  'frame'         the array as read: [2h,2w] (mosaic) or [h,w,4] (packed)
  'n_path'        its path
  'video'         the video's key: its folder under <dataroot>/<nFolder>
  'FirstOfVideo'  True for the first frame of a video
Public attributes: `n_paths`, `videos` ([(key, [frame paths])], the order samples come in), `layout` ("mosaic" or
"packed_hwc": what `RvddRuntime.video_push` is told) and `dtype`.
"""
import os

import numpy as np

from ..library import iio_read, list_video_files_at_dir


def _video_dirs(root, wanted):
    """Sub-folders of `root` (one per video), hidden ones skipped, optionally restricted to `wanted` names."""
    return sorted(e.path for e in os.scandir(root)
                  if e.is_dir() and not e.name.startswith('.') and (wanted is None or e.name in wanted))


class rawvideoDataset:
    @staticmethod
    def modify_commandline_options(parser, is_train=True):
        return parser

    def __init__(self, opt):
        self.opt = opt
        self.rootdir = opt.dataroot
        self.n_paths = os.path.join(self.rootdir, opt.nFolder)
        if isinstance(opt.videos, str):
            opt.videos = opt.videos.split(',')
        dirs = _video_dirs(self.n_paths, opt.videos)
        print('%d videos' % len(dirs))
        self.videos = [(os.path.relpath(d, self.n_paths), list_video_files_at_dir(d)) for d in dirs]
        self._index = [(v, k) for v, (_, frames) in enumerate(self.videos) for k in range(len(frames))]
        self.layout = self.dtype = None
        if self._index:
            self._classify(self._read(self.videos[0][1][0]), self.videos[0][1][0])

    @staticmethod
    def _read(path):
        a = iio_read(path)
        return a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a

    def _classify(self, a, path):
        """Layout and sample type of a frame; the first call fixes them, a later frame must agree."""
        if a.ndim == 2 and a.shape[0] % 2 == 0 and a.shape[1] % 2 == 0:
            layout = "mosaic"
        elif a.ndim == 3 and a.shape[2] == 4:
            layout = "packed_hwc"
        else:
            raise ValueError("%s: a raw frame is a 1-channel mosaic of even size or a 4-channel packed frame, got shape %s"
                             % (path, a.shape))
        if a.dtype not in (np.uint16, np.float32):
            raise ValueError("%s: raw frames are uint16 or float32, got %s" % (path, a.dtype))
        if self.layout is None:
            self.layout, self.dtype = layout, a.dtype
        elif (layout, a.dtype) != (self.layout, self.dtype):
            raise ValueError("%s is a %s %s frame, but this dataset's first frame (%s) is %s %s"
                             % (path, layout, a.dtype, self.videos[0][1][0], self.layout, self.dtype))

    def __len__(self):
        return len(self._index)

    def prepare_epoch(self):
        print("nothing to do in prepare_epoch")

    def data_num_channels(self):
        return 4

    def read_frame(self, path):
        """One frame as `__getitem__` yields it, checked against the dataset's layout and sample type."""
        a = self._read(path)
        self._classify(a, path)
        return a

    def __getitem__(self, index):
        v, k = self._index[index]
        key, frames = self.videos[v]
        return {'frame': self.read_frame(frames[k]), 'n_path': frames[k], 'video': key, 'FirstOfVideo': k == 0}
