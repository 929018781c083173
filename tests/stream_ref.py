"""numpy restatement of rvdd_ingest_raw (include/rvdd.h) and small helpers shared by the stream tests."""
import numpy as np
import torch


def cells_of(frames, layout):
    """Sensor frames -> [n,hh,ww,4] float32 DN, channel k = CFA position (k >> 1, k & 1) of each 2x2 cell."""
    a = np.asarray(frames)
    if layout == "mosaic":
        a = np.stack([a[:, (k >> 1)::2, (k & 1)::2] for k in range(4)], axis=-1)
    return a.astype(np.float32)


def ingest_ref(frames, layout, bit_depth):
    """-> (packed [n,4,hh,ww], gray [n,hh,ww]) float32, one f32 operation at a time."""
    c = cells_of(frames, layout)
    maxv = np.float32(2 ** bit_depth - 1)
    t = c / maxv                                              # correctly rounded f32 division
    packed = (np.float32(2.0) * t - np.float32(1.0)).transpose(0, 3, 1, 2)
    gray = (((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]) * np.float32(0.25)
    assert packed.dtype == np.float32 and gray.dtype == np.float32
    return np.ascontiguousarray(packed), np.ascontiguousarray(gray)


def quantised_dn(seq_raw, bit_depth=12):
    """synth.make_sequence(...).raw ([T,4,h,w] in [-1,1]) -> whole digital numbers [T,h,w,4] float32 in 0 .. 2^bd - 1."""
    maxv = float(2 ** bit_depth - 1)
    dn = torch.round((seq_raw.double() + 1.0) / 2.0 * maxv).clamp(0, maxv)
    return dn.permute(0, 2, 3, 1).contiguous().numpy().astype(np.float32)


def mosaic_of(cells):
    """[n,hh,ww,4] -> [n,2hh,2ww]: the plane a sensor writes."""
    n, hh, ww, _ = cells.shape
    m = np.zeros((n, 2 * hh, 2 * ww), dtype=cells.dtype)
    for k in range(4):
        m[:, (k >> 1)::2, (k & 1)::2] = cells[..., k]
    return m


def to_gpu(a, dev="cuda"):
    """numpy sensor frames -> the GPU tensor RvddRuntime.ingest_raw / video_push take (uint16 as its int16 view)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(dev)
