"""numpy reference of the two bit packings of 10 / 12 / 14-bit raw frames (include/rvdd.h, enum rvdd_bits_order): what
rvdd_ingest_bits reads and rvdd_egress_bits writes.  Plain and slow on purpose; the last axis of an array is a sensor row.

  "mipi"  MIPI CSI-2 RAW10 / RAW12 / RAW14: groups of G = 4 (2 at 12 bits) pixels, G bytes of the samples' upper eight bits, then
          G (b - 8) / 8 bytes of their lower bits -- pixel 0's lowest -- least significant byte first
  "msb"   TIFF 6.0 FillOrder 1: every sample b bits wide, most significant bit first, one bit string per row, zero-padded to a byte
"""
import numpy as np

ORDERS = ("mipi", "msb")          # the index is the enum's value
DEPTHS = (10, 12, 14)


def group(bits):
    return 2 if bits == 12 else 4


def row_bytes(width, bits, order):
    """bytes of a row of `width` samples; ValueError where the MIPI packing has no such row"""
    if bits not in DEPTHS:
        raise ValueError(f"bits must be 10, 12 or 14, got {bits}")
    if order == "mipi":
        if width % group(bits):
            raise ValueError(f"a MIPI RAW{bits} row is groups of {group(bits)} pixels, got width {width}")
        return width * bits // 8
    if order != "msb":
        raise ValueError(f"order {order!r} is not one of {ORDERS}")
    return (width * bits + 7) // 8


def pack(x, bits, order):
    """uint16 [..., W] with values below 2^bits -> uint8 [..., row_bytes]"""
    x = np.asarray(x)
    assert x.dtype == np.uint16 and (x.size == 0 or int(x.max()) < (1 << bits))
    W = x.shape[-1]
    rb = row_bytes(W, bits, order)
    if order == "mipi":
        G, low = group(bits), bits - 8
        g = x.reshape(x.shape[:-1] + (W // G, G)).astype(np.uint32)
        L = np.zeros(g.shape[:-1], np.uint32)
        for k in range(G):
            L |= (g[..., k] & ((1 << low) - 1)) << (k * low)
        tail = [((L >> (8 * i)) & 0xFF) for i in range(G * low // 8)]
        out = np.concatenate([g >> low, np.stack(tail, -1)], -1).astype(np.uint8)
        return out.reshape(x.shape[:-1] + (rb,))
    b = ((x[..., None] >> np.arange(bits - 1, -1, -1, dtype=np.uint16)) & 1).astype(np.uint8)
    b = b.reshape(x.shape[:-1] + (W * bits,))
    pad = np.zeros(x.shape[:-1] + (8 * rb - W * bits,), np.uint8)
    return np.packbits(np.concatenate([b, pad], -1), axis=-1)


def unpack(rows, width, bits, order):
    """uint8 [..., row_bytes] -> uint16 [..., width]; pad bits are ignored"""
    rows = np.asarray(rows)
    rb = row_bytes(width, bits, order)
    assert rows.dtype == np.uint8 and rows.shape[-1] == rb, (rows.dtype, rows.shape, rb)
    if order == "mipi":
        G, low = group(bits), bits - 8
        g = rows.reshape(rows.shape[:-1] + (width // G, G * bits // 8)).astype(np.uint32)
        L = np.zeros(g.shape[:-1], np.uint32)
        for i in range(G * low // 8):
            L |= g[..., G + i] << (8 * i)
        px = [(g[..., k] << low) | ((L >> (k * low)) & ((1 << low) - 1)) for k in range(G)]
        return np.stack(px, -1).astype(np.uint16).reshape(rows.shape[:-1] + (width,))
    b = np.unpackbits(rows, axis=-1)[..., :width * bits].reshape(rows.shape[:-1] + (width, bits)).astype(np.uint32)
    return (b << np.arange(bits - 1, -1, -1, dtype=np.uint32)).sum(-1).astype(np.uint16)
