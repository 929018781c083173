"""`--dataset_mode rawvideo`: footage as a camera leaves it,

    <dataroot>/<nFolder>/<video>/<frame>.tif[f] ,

and nothing else: no ground truth, no flow or warp folder (the flows of such footage are computed on the device,
`RvddRuntime.video_push`).  A frame is one plane of sensor values (a 1-channel TIFF: the Bayer mosaic, [2h,2w]) or the
reference dataset's packed form (4 channels, [h,w,4], channel k = CFA position (k >> 1, k & 1) of each 2x2 cell), as
`uint16` or `float32` digital numbers.  The first frame of the first video decides which; a later frame of another
kind is an error that names the file.

Frames of packed 10 / 12 / 14-bit samples stay packed -- the device unpacks them (`RvddRuntime.video_push(container=...)`):
  * a tree of 1-sample uncompressed TIFFs with BitsPerSample 10 / 12 / 14 (`tiffio.read_packed`) is container "msb"; --bit_depth
    must equal the files' BitsPerSample;
  * with `--raw_container mipi --raw_size WxH` the frames are headerless `<frame>.raw` files of H rows of MIPI CSI-2
    RAW<bit_depth> bytes (W * bit_depth / 8 each), container "mipi".
A frame is then the uint8 [2h, row_bytes] array of its rows, `layout` is "mosaic" and `dtype` uint8; containers do not mix.

One sample, in video order:
  'frame'         the array as read: [2h,2w] (mosaic) or [h,w,4] (packed)
  'n_path'        its path
  'video'         the video's key: its folder under <dataroot>/<nFolder>
  'FirstOfVideo'  True for the first frame of a video
Public attributes: `n_paths`, `videos` ([(key, [frame paths])], the order samples come in), `layout` ("mosaic" or
"packed_hwc": what `RvddRuntime.video_push` is told), `dtype` and `container` (None, "msb" or "mipi").
`frame_size(path)` is a frame's (H, W) in pixels whatever its form.
"""
import os

import numpy as np

from .. import tiffio
from ..library import get_files_pattern, iio_read, list_video_files_at_dir

PACKED_BITS = tiffio.PACKED_BITS


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
        self.bit_depth = int(opt.bit_depth)
        self.raw_size = None
        raw_container = getattr(opt, 'raw_container', None)
        if raw_container is not None:
            self._raw_container_options(raw_container, getattr(opt, 'raw_size', None))
            self.videos = [(os.path.relpath(d, self.n_paths), self._raw_files(d)) for d in dirs]
        else:
            self.videos = [(os.path.relpath(d, self.n_paths), list_video_files_at_dir(d)) for d in dirs]
        self._index = [(v, k) for v, (_, frames) in enumerate(self.videos) for k in range(len(frames))]
        self.layout = self.dtype = self.container = None
        self._width = {}                    # path -> W of a packed frame read so far
        if self._index:
            self.read_frame(self.videos[0][1][0])

    def _raw_container_options(self, container, size):
        if container != 'mipi':
            raise ValueError("--raw_container %r: headerless frames are 'mipi' (packed TIFFs are recognised by themselves)" % (container,))
        if self.bit_depth not in PACKED_BITS:
            raise ValueError("--raw_container mipi needs --bit_depth 10, 12 or 14, got %d" % self.bit_depth)
        try:
            W, H = (int(v) for v in str(size).lower().split('x'))
        except ValueError:
            raise ValueError("--raw_container mipi needs --raw_size WxH in pixels, got %r" % (size,))
        group = 2 if self.bit_depth == 12 else 4
        if W < 2 or H < 2 or W % 2 or H % 2 or W % group:
            raise ValueError("--raw_size %dx%d: a MIPI RAW%d mosaic has an even height and a width that is a multiple of %d"
                             % (W, H, self.bit_depth, max(group, 2)))
        self.raw_size = (H, W)

    @staticmethod
    def _raw_files(d):
        paths = get_files_pattern(d, '*.raw')
        if not paths:
            raise AssertionError("%s holds no .raw frame" % d)
        return [os.path.join(d, p) for p in paths]

    def _read(self, path):
        """-> (array, container): the frame as `__getitem__` yields it"""
        if self.raw_size is not None:
            H, W = self.raw_size
            rb = W * self.bit_depth // 8
            a = np.fromfile(path, dtype=np.uint8)
            if a.size != H * rb:
                raise ValueError("%s: a %dx%d MIPI RAW%d frame is %d bytes, the file has %d" % (path, W, H, self.bit_depth, H * rb, a.size))
            self._width[path] = W
            return a.reshape(H, rb), "mipi"
        plain = lambda a: (a[:, :, 0] if a.ndim == 3 and a.shape[2] == 1 else a)
        if path.lower().endswith(('.tif', '.tiff')):
            first = None
            if self.container != "msb":               # a tree known to be packed goes straight to the packed reader
                try:
                    return plain(iio_read(path)), None
                except tiffio.TiffError as err:
                    first = err
            try:
                rows, W, bits = tiffio.read_packed(path)
            except tiffio.TiffError:
                if first is not None:                 # neither reader takes the file: the general reader's message
                    raise first
                return plain(iio_read(path)), None    # a plain frame in a packed tree: _classify names it
            if bits != self.bit_depth:
                raise ValueError("%s: the file's BitsPerSample is %d but --bit_depth is %d" % (path, bits, self.bit_depth))
            self._width[path] = W
            return rows, "msb"
        return plain(iio_read(path)), None

    def _classify(self, a, path, container=None):
        """Layout, sample type and container of a frame; the first call fixes them, a later frame must agree."""
        if container is not None:
            W = self._width[path]
            if a.shape[0] % 2 or W % 2:
                raise ValueError("%s: a raw frame is a mosaic of even size, got %d x %d" % (path, W, a.shape[0]))
            layout = "mosaic"
        elif a.ndim == 2 and a.shape[0] % 2 == 0 and a.shape[1] % 2 == 0:
            layout = "mosaic"
        elif a.ndim == 3 and a.shape[2] == 4:
            layout = "packed_hwc"
        else:
            raise ValueError("%s: a raw frame is a 1-channel mosaic of even size or a 4-channel packed frame, got shape %s"
                             % (path, a.shape))
        if container is None and a.dtype not in (np.uint16, np.float32):
            raise ValueError("%s: raw frames are uint16 or float32, got %s" % (path, a.dtype))
        if self.layout is None:
            self.layout, self.dtype, self.container = layout, a.dtype, container
        elif (layout, a.dtype, container) != (self.layout, self.dtype, self.container):
            kind = lambda lay, dt, c: "%s %s" % (lay, dt) if c is None else "%s packed-bits (%s)" % (lay, c)
            raise ValueError("%s is a %s frame, but this dataset's first frame (%s) is %s"
                             % (path, kind(layout, a.dtype, container), self.videos[0][1][0], kind(self.layout, self.dtype, self.container)))

    def __len__(self):
        return len(self._index)

    def prepare_epoch(self):
        print("nothing to do in prepare_epoch")

    def data_num_channels(self):
        return 4

    def read_frame(self, path):
        """One frame as `__getitem__` yields it, checked against the dataset's layout and sample type."""
        a, container = self._read(path)
        self._classify(a, path, container)
        return a

    def frame_size(self, path):
        """(H, W) in pixels of the frame at `path`"""
        a = self.read_frame(path)
        if self.container is not None:
            return a.shape[0], self._width[path]
        return (a.shape[0], a.shape[1]) if self.layout == "mosaic" else (2 * a.shape[0], 2 * a.shape[1])

    def __getitem__(self, index):
        v, k = self._index[index]
        key, frames = self.videos[v]
        return {'frame': self.read_frame(frames[k]), 'n_path': frames[k], 'video': key, 'FirstOfVideo': k == 0}
