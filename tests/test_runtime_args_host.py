"""The argument checks of rvdd_release_amd.runtime, without a GPU: one table of (checker call, bad argument, exception type, fragment of
the message).  The fragments are the ones the hand-written checks raised for the same misuse before there was one checker, so the
callers' `pytest.raises(..., match=...)` across the suite keep matching.

The checkers never touch a tensor's data, so a host tensor that SAYS it lives on cuda:k serves for every check behind the first."""
import types

import numpy as np
import pytest
import torch

from rvdd_release_amd import runtime as R

U16 = getattr(torch, "uint16", torch.int16)


class OnCuda(torch.Tensor):
    """a host tensor whose `is_cuda` and `device` claim cuda:`index`"""
    index = 0
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", self.index))


class OnCuda1(OnCuda):
    index = 1


def cuda(*shape, dtype=torch.float32, cls=OnCuda):
    return torch.zeros(*shape, dtype=dtype).as_subclass(cls)


TDEV = torch.device("cuda", 0)
NO_GPU = r"must be a GPU tensor \(rvdd has no CPU path\)"
# an RvddRuntime as far as the argument checks of its methods go
ME = types.SimpleNamespace(device=0)
ME._in_place = types.MethodType(R.RvddRuntime._in_place, ME)
CASES = [
    # not a tensor, and a tensor on the host
    ("chk-none", lambda: R._dev_tensor(None, "rgb", 0), RuntimeError, "rgb " + NO_GPU),
    ("chk-array", lambda: R._dev_tensor([1.0, 2.0], "out", 0), RuntimeError, "out " + NO_GPU),
    ("chk-cpu", lambda: R._dev_tensor(torch.zeros(2, 3), "raw_prev", 0), RuntimeError, "raw_prev " + NO_GPU),
    ("raw-cpu", lambda: R._raw_frames(torch.zeros(1, 4, 4, dtype=torch.int16), "mosaic", "ingest_raw", 0), RuntimeError,
     "ingest_raw: frames " + NO_GPU),
    ("strided-cpu", lambda: R._batch_strided(torch.zeros(1, 4, 2, 2), (1, 4, 2, 2), "raw_cur", 0), RuntimeError, "raw_cur " + NO_GPU),
    ("out-cpu", lambda: R._out_or_new(torch.zeros(2, 6, 10), "egress: out", (2, 6, 10), TDEV, form="egress: out must be a contiguous"),
     RuntimeError, "egress: out " + NO_GPU),
    ("frames-list", lambda: R._frames([[1.0]], 4, "noise_hist: packed is [n,4,hh,ww]", "packed", 0), RuntimeError,
     r"noise_hist: packed is \[n,4,hh,ww\], got \(\)"),
    # another device than the runtime's
    ("chk-dev", lambda: R._dev_tensor(cuda(2, 3, cls=OnCuda1), "raw_cur", 0), RuntimeError, "raw_cur lives on cuda:1 but this runtime drives cuda:0"),
    ("strided-dev", lambda: R._batch_strided(cuda(1, 4, 2, 2, cls=OnCuda1), (1, 4, 2, 2), "raw_cur", 0), RuntimeError, "lives on"),
    # wrong dtype
    ("chk-dtype", lambda: R._dev_tensor(cuda(2, 3, dtype=torch.float64), "flow", 0), RuntimeError, "flow must be float32"),
    ("strided-dtype", lambda: R._batch_strided(cuda(1, 4, 2, 2, dtype=torch.float16), (1, 4, 2, 2), "raw_prev", 0), RuntimeError,
     "raw_prev must be float32"),
    ("raw-dtype", lambda: R._raw_frames(cuda(1, 4, 4, dtype=torch.int32), "mosaic", "ingest_raw", 0), RuntimeError,
     r"ingest_raw: frames must be uint16 \(or its int16 view\) or float32, got torch.int32"),
    ("bits-dtype", lambda: R._dev_tensor(cuda(96, dtype=torch.int16), "ingest_bits: frames", 0, dtype=torch.uint8, contiguous="require",
                                         form="ingest_bits: packed frames are a contiguous uint8 tensor"), RuntimeError,
     "ingest_bits: packed frames are a contiguous uint8 tensor, got torch.int16"),
    ("out-dtype", lambda: R._out_or_new(cuda(2, 6, 10, dtype=torch.int16), "egress: out", (2, 6, 10), TDEV, torch.float32,
                                        form="egress: out must be a contiguous torch.float32 tensor of shape (2, 6, 10)"), RuntimeError,
     r"egress: out must be a contiguous torch.float32 tensor of shape \(2, 6, 10\), got torch.int16 \(2, 6, 10\)"),
    ("words-dtype", lambda: R._out_or_new(cuda(4, 2, 2), "dpc_detect: hits", (4, 2, 2), TDEV, R._WORD32, zero=True,
                                          form="dpc_detect: hits is a contiguous int32 / uint32 tensor [4,2,2] on cuda:0"), RuntimeError,
     r"dpc_detect: hits is a contiguous int32 / uint32 tensor \[4,2,2\] on cuda:0"),
    # wrong shape
    ("chk-shape", lambda: R._dev_tensor(cuda(1, 4, 4, 4), "dither", 0, shape=(1, 4, 4, 3)), RuntimeError,
     r"dither has shape \(1, 4, 4, 4\), expected \(1, 4, 4, 3\)"),
    ("chk-rank", lambda: R._dev_tensor(cuda(4, 4), "gray", 0, shape=(1, 4, 4)), RuntimeError, r"gray has shape \(4, 4\), expected \(1, 4, 4\)"),
    ("strided-shape", lambda: R._batch_strided(cuda(1, 4, 2, 3), (1, 4, 2, 2), "raw_next", 0), RuntimeError, "raw_next has shape"),
    ("open-shape", lambda: R._dev_tensor(cuda(1, 4, 4, 4, dtype=torch.uint8), "unprocess: srgb", 0, dtype=torch.uint8,
                                         shape=(None, None, None, 3), form="unprocess: srgb is uint8 [n,H,W,3]"), RuntimeError,
     r"unprocess: srgb is uint8 \[n,H,W,3\], got torch.uint8 \(1, 4, 4, 4\)"),
    ("out-shape", lambda: R._out_or_new(cuda(2, 6, 10, 1), "egress: out", (2, 6, 10), TDEV, form="egress: out must be a contiguous"),
     RuntimeError, "egress: out must be a contiguous"),
    ("out-bytes", lambda: R._out_or_new(cuda(385, dtype=torch.uint8), "egress_bits: out", (2, 8, 24), TDEV, torch.uint8, nbytes=384,
                                        form="egress_bits: out must be a contiguous uint8 tensor of 384 elements"), RuntimeError,
     r"egress_bits: out must be a contiguous uint8 tensor of 384 elements, got torch.uint8 \(385,\)"),
    ("acc-bytes", lambda: R._dev_tensor(cuda(7, dtype=torch.int32), "noise_hist: acc", 0, dtype=None, nbytes=R.NOISE_ACC_BYTES,
                                        contiguous="require", form="noise_hist: acc is a contiguous tensor of 131616 bytes on cuda:0"),
     RuntimeError, "131616 bytes"),
    ("frames-rank", lambda: R._frames(cuda(4, 2, 2), 4, "dpc: packed is [n,4,hh,ww]", "packed", 0), RuntimeError,
     r"dpc: packed is \[n,4,hh,ww\], got \(4, 2, 2\)"),
    ("frames-channels", lambda: R._frames(cuda(2, 2, 6, 10), 3, "egress: rgb is [n,3,H,W]", "rgb", 0), RuntimeError, r"\[n,3,H,W\]"),
    ("raw-mosaic", lambda: R._raw_frames(cuda(1, 5, 4, dtype=torch.int16), "mosaic", "video_push", 0), RuntimeError,
     r"video_push: mosaic frames are \[n,2hh,2ww\], got \(1, 5, 4\)"),
    ("raw-hwc", lambda: R._raw_frames(cuda(1, 4, 4, 3), "packed_hwc", "ingest_raw", 0), RuntimeError,
     r"ingest_raw: packed_hwc frames are \[n,hh,ww,4\]"),
    # not contiguous where the tensor is written, or corrected, where it lies
    ("out-strided", lambda: R._out_or_new(cuda(4, 6144, dtype=torch.uint8)[::2], "frame_sigs: out", (2, 6144), TDEV, torch.uint8,
                                          form="frame_sigs: out is a contiguous uint8 tensor [2,6144] on cuda:0"), RuntimeError,
     r"frame_sigs: out is a contiguous uint8 tensor \[2,6144\] on cuda:0"),
    ("step-out-strided", lambda: R._out_or_new(cuda(1, 3, 4, 8)[..., ::2], "out", (1, 3, 4, 4), TDEV), RuntimeError, "out must be contiguous"),
    ("in-place-strided", lambda: R._frames(cuda(1, 4, 4, 8)[..., ::2], 4, "dpc_map_apply: packed is [n,4,hh,ww]", "packed", 0,
                                           contiguous="require"), RuntimeError, "packed must be contiguous"),
    # names the library has an enum for
    ("bayer", lambda: R._pattern_index("xtrans", "egress"), ValueError, "egress: pattern 'xtrans' is not one of gbrg, grbg, rggb, bggr"),
    ("bayer-handle", lambda: R.RvddRuntime._pattern(types.SimpleNamespace(bayer_pattern=2), "xtrans", "gray_of_rgb"), ValueError,
     "gray_of_rgb: pattern 'xtrans' is not one of"),
    ("bayer-none", lambda: R._pattern_index(None, "demosaic"), ValueError, "demosaic: pattern None is not one of"),
    ("raw-layout", lambda: R._raw_frames(cuda(1, 4, 4), "chw", "ingest_raw", 0), ValueError, "ingest_raw: layout 'chw' is not one of mosaic, packed_hwc"),
    ("egress-dtype", lambda: R.RvddRuntime.egress(types.SimpleNamespace(_pattern=lambda pattern, who: 0), cuda(2, 3, 6, 10), "mosaic", torch.float16),
     RuntimeError, r"egress: dtype must be torch.uint16 \(or torch.int16, its view\) or torch.float32, got torch.float16"),
    # host maps for the setters and the host-only calls: dtype, rank, a fixed first dimension; arrays and CPU tensors alike
    ("map-dtype", lambda: R._host_map(np.zeros((4, 6), np.int32), "uint8", "set_dpc_map: cellmask is uint8 [hh,ww]", (None, None)), RuntimeError,
     r"set_dpc_map: cellmask is uint8 \[hh,ww\], got int32 \(4, 6\)"),
    ("map-rank", lambda: R._host_map(torch.zeros(2, 4, 6, dtype=torch.uint8), "uint8", "dpc_map_stats: cellmask is uint8 [hh,ww]", (None, None)),
     RuntimeError, r"dpc_map_stats: cellmask is uint8 \[hh,ww\], got uint8 \(2, 4, 6\)"),
    ("map-rows", lambda: R._host_map(np.zeros((3, 8), np.float32), "float32", "set_cols: cmap is float32 [2,ww]", (2, None)), RuntimeError,
     r"set_cols: cmap is float32 \[2,ww\], got float32 \(3, 8\)"),
    ("map-f64", lambda: R._host_map(torch.zeros(2, 3, dtype=torch.float64), "float32", "set_green: gmap is float32 [gh,gw]", (None, None)), RuntimeError,
     r"set_green: gmap is float32 \[gh,gw\], got float64 \(2, 3\)"),
    ("map-stats", lambda: R.dpc_map_stats(np.zeros(16, np.uint8)), RuntimeError, r"dpc_map_stats: cellmask is uint8 \[hh,ww\], got uint8 \(16,\)"),
    # wrong twice: the tensor between packed and gray is named first, as before the preamble was shared
    ("in-place-order-rows", lambda: R.RvddRuntime.rows_apply(ME, cuda(1, 4, 6, 8), cuda(1, 2, 5), gray=cuda(1, 6, 9)), RuntimeError,
     r"rows_apply: offsets is a float32 tensor \[1,2,6\]"),
    ("in-place-order-cols", lambda: R.RvddRuntime.cols_apply(ME, cuda(1, 4, 6, 8), cuda(2, 7), gray=cuda(1, 6, 9)), RuntimeError,
     r"cols_apply: cmap is a float32 tensor \[2,8\]"),
    ("in-place-order-green", lambda: R.RvddRuntime.green_apply(ME, cuda(1, 4, 6, 8), cuda(3), 64.0, gray=cuda(1, 6, 9)), RuntimeError,
     r"green_apply: gmap is a float32 tensor \[gh,gw\]"),
    ("in-place-gray", lambda: R.RvddRuntime.rows_apply(ME, cuda(1, 4, 6, 8), cuda(1, 2, 6), gray=cuda(1, 6, 9)), RuntimeError, "gray"),
    ("map-fit", lambda: R.cols_fit(np.zeros((3, 2, 8), np.float32), np.zeros((3, 2, 8), np.float32), 1), RuntimeError,
     r"cols_fit: offsets is float32 \[F,2,ww\] and state uint8 \[F,2,ww\], got float32 \(3, 2, 8\) and float32 \(3, 2, 8\)"),
]


@pytest.mark.parametrize("call,exc,fragment", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_a_bad_argument_is_refused_with_the_message_its_callers_match(call, exc, fragment):
    with pytest.raises(exc, match=fragment):
        call()


def test_good_arguments_pass_and_come_back_dense():
    m = np.arange(24, dtype=np.float32).reshape(2, 12)
    assert R._host_map(m, "float32", "m", (2, None)) is m and R._host_map(m[:, ::2]).flags["C_CONTIGUOUS"]
    assert np.array_equal(R._host_map(torch.from_numpy(m), "float32", "m", (None, 12)), m)
    assert np.array_equal(R._host_map(torch.from_numpy(m).requires_grad_(), "float32", "m", (2, 12)), m)      # detached: accepted, never refused
    t = cuda(2, 4, 3, 5)
    assert R._dev_tensor(t, "t", 0, shape=(2, 4, 3, 5)) is t and R._dev_tensor(t, "t", None) is t
    assert R._dev_tensor(t, "t", 0, shape=(None, 4, None, 5)) is t
    strided = cuda(2, 4, 3, 10)[..., ::2]
    dense = R._dev_tensor(strided, "t", 0, shape=(2, 4, 3, 5))
    assert dense is not strided and dense.is_contiguous() and R._dev_tensor(strided, "t", 0, contiguous=None) is strided
    assert R._out_or_new(t, "out", (2, 4, 3, 5), TDEV) is t
    words = cuda(4, 3, 5, dtype=torch.int32)
    assert R._out_or_new(words, "hits", (4, 3, 5), TDEV, R._WORD32, zero=True) is words
    got, n, h, w = R._frames(t, 4, "op: packed is [n,4,hh,ww]", "packed", 0)
    assert got is t and (n, h, w) == (2, 3, 5)
    # a step's inputs keep their batch stride: a channel slice is not copied, anything else is
    whole = cuda(2, 6, 3, 5)
    sl, stride = R._batch_strided(whole[:, :4], (2, 4, 3, 5), "raw_cur", 0)
    assert sl.data_ptr() == whole.data_ptr() and stride == 6 * 15
    cp, stride = R._batch_strided(cuda(2, 4, 3, 10)[..., ::2], (2, 4, 3, 5), "raw_cur", 0)
    assert cp.is_contiguous() and stride == 4 * 15
    assert R._batch_strided(None, (2, 4, 3, 5), "raw_next", 0) == (None, 0)


def test_names_and_dtypes_map_to_the_librarys_enums():
    from rvdd_release_amd import _lib
    assert [R._pattern_index(p, "t") for p in R.BAYER_PATTERNS] == [0, 1, 2, 3]
    handle = types.SimpleNamespace(bayer_pattern=2)
    assert R.RvddRuntime._pattern(handle, None, "t") == 2 and R.RvddRuntime._pattern(handle, "grbg", "t") == 1
    assert R.RvddRuntime._pattern(types.SimpleNamespace(), None, "t") == 0            # no set_option("bayer_pattern") yet: gbrg
    assert R._raw_dtype(torch.float32) == _lib.RAW_F32 and R._raw_dtype(torch.int16) == _lib.RAW_U16 and R._raw_dtype(U16) == _lib.RAW_U16
    assert all(R._raw_dtype(d) is None for d in (torch.float16, torch.float64, torch.int32, torch.uint8))
    t, dtype, lay, n, hh, ww = R._raw_frames(cuda(2, 6, 10, dtype=torch.int16), "mosaic", "ingest_raw", 0)
    assert (dtype, lay, n, hh, ww) == (_lib.RAW_U16, _lib.RAW_MOSAIC, 2, 3, 5)
    t, dtype, lay, n, hh, ww = R._raw_frames(cuda(2, 3, 5, 4), "packed_hwc", "ingest_raw", 0)
    assert (dtype, lay, n, hh, ww) == (_lib.RAW_F32, _lib.RAW_PACKED_HWC, 2, 3, 5)


def test_no_module_imports_the_denoise_command():
    """`denoise` drives the feature modules (`footage`, `noise`, `cuts`, `dpc_map`, ...), never the reverse: a text scan of the package's
    own sources for an import of `.denoise` outside denoise.py."""
    import os
    import re
    root = os.path.dirname(os.path.abspath(R.__file__))
    imports = re.compile(r"^\s*(from\s+(\.+|rvdd_release_amd)(\S*\.)?denoise\s+import\b|import\s+rvdd_release_amd\.denoise\b"
                         r"|from\s+(\.+\S*|rvdd_release_amd\S*)\s+import\s+(\(|.*,\s*)?denoise\b)", re.M)
    seen = 0
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py") and os.path.join(dp, f) != os.path.join(root, "denoise.py"):
                seen += 1
                found = imports.search(open(os.path.join(dp, f)).read())
                assert found is None, (os.path.join(dp, f), found.group(0))
    assert seen > 10
    for line in ("from .denoise import dpc_arguments", "    from . import denoise", "from . import cuts, denoise", "import rvdd_release_amd.denoise",
                 "from rvdd_release_amd.denoise import _parse", "from rvdd_release_amd import noise, denoise", "from .. import denoise"):
        assert imports.search(line), line
    for line in ("python -m rvdd_release_amd.denoise --dataroot D", "from .footage import estimate_noise", "from . import denoise_ref"):
        assert not imports.search(line), line
