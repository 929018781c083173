"""Packed 10 / 12 / 14-bit raw frames, host side: the numpy reference of the two packings (bits_ref.py) against the known answers of
include/rvdd.h, the packed TIFF reader / writer, the rawvideo dataset's containers, the argument errors of the denoise command
line, and the enum Python shares with the header.  No GPU."""
import os
import re
import struct

import numpy as np
import pytest

import bits_ref
from conftest import REPO

HEX = bytes.fromhex
# bits -> (pixels, MIPI bytes, MSB bytes)
KNOWN = {10: ([0x3FF, 0x000, 0x155, 0x2AA], HEX("FF0055AA93"), HEX("FFC00556AA")),
         12: ([0xABC, 0x123], HEX("AB123C"), HEX("ABC123")),
         14: ([0x3FFF, 0x0000, 0x2AAA, 0x1555], HEX("FF00AA553FA056"), HEX("FFFC000AAA9555"))}


@pytest.mark.parametrize("bits", bits_ref.DEPTHS)
def test_known_answers(bits):
    px, mipi, msb = KNOWN[bits]
    x = np.array(px, np.uint16)
    for order, want in (("mipi", mipi), ("msb", msb)):
        assert bits_ref.pack(x, bits, order).tobytes() == want
        assert bits_ref.unpack(np.frombuffer(want, np.uint8), len(px), bits, order).tolist() == px


def test_msb_row_of_three_pixels_has_two_pad_bits():
    row = bits_ref.pack(np.array([0x3FF, 0x001, 0x200], np.uint16), 10, "msb")
    assert row.tobytes() == HEX("FFC01800")
    dirty = row.copy()
    dirty[-1] |= 0x03                                     # the pad bits are not data
    assert bits_ref.unpack(dirty, 3, 10, "msb").tolist() == [0x3FF, 0x001, 0x200]


@pytest.mark.parametrize("order", bits_ref.ORDERS)
@pytest.mark.parametrize("bits", bits_ref.DEPTHS)
def test_round_trip_of_every_value(bits, order):
    """every value of the depth at every position of a group / of the bit string's byte phases"""
    v = np.arange(1 << bits, dtype=np.uint16)
    for shift in range(4):
        x = np.roll(v, shift).reshape(-1, 64)
        p = bits_ref.pack(x, bits, order)
        assert p.dtype == np.uint8 and p.shape == (x.shape[0], 64 * bits // 8)
        assert np.array_equal(bits_ref.unpack(p, 64, bits, order), x)


def test_row_lengths_and_the_group_rule():
    assert [bits_ref.row_bytes(16, b, "mipi") for b in (10, 12, 14)] == [20, 24, 28]
    assert [bits_ref.row_bytes(16, b, "msb") for b in (10, 12, 14)] == [20, 24, 28]
    assert bits_ref.row_bytes(36, 10, "mipi") == 45 and bits_ref.row_bytes(36, 10, "msb") == 45          # odd row lengths exist
    assert [bits_ref.row_bytes(14, b, "msb") for b in (10, 12, 14)] == [18, 21, 25]                        # 140 / 168 / 196 bits
    assert bits_ref.row_bytes(14, 12, "mipi") == 21                                                        # pairs: any even width
    for b in (10, 14):
        with pytest.raises(ValueError, match="groups of 4"):
            bits_ref.row_bytes(14, b, "mipi")
    with pytest.raises(ValueError):
        bits_ref.row_bytes(16, 11, "msb")
    # an odd ww: the pad bits come out zero, and garbage in them is not read
    rng = np.random.default_rng(1)
    for b in bits_ref.DEPTHS:
        x = rng.integers(0, 1 << b, (10, 14)).astype(np.uint16)
        p = bits_ref.pack(x, b, "msb")
        pad = 8 * p.shape[1] - 14 * b
        assert pad == (0 if b == 12 else 4) and not (p[:, -1] & ((1 << pad) - 1)).any()       # 140 / 168 / 196 bits
        q = p.copy()
        q[:, -1] |= (1 << pad) - 1
        assert np.array_equal(bits_ref.unpack(q, 14, b, "msb"), x)


def test_runtime_row_bytes_is_the_reference():
    from rvdd_release_amd.runtime import BITS_DEPTHS, BITS_ORDERS, bits_row_bytes
    assert tuple(BITS_DEPTHS) == bits_ref.DEPTHS and BITS_ORDERS == {"mipi": 0, "msb": 1}
    for b in bits_ref.DEPTHS:
        for w in (2, 4, 14, 16, 36, 52, 1280):
            assert bits_row_bytes(w, b, "msb") == bits_ref.row_bytes(w, b, "msb")
            if w % bits_ref.group(b) == 0:
                assert bits_row_bytes(w, b, "mipi") == bits_ref.row_bytes(w, b, "mipi")


# ---- tiffio ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", bits_ref.DEPTHS)
def test_tiff_packed_round_trip(tmp_path, bits):
    from rvdd_release_amd import tiffio
    x = np.random.default_rng(bits).integers(0, 1 << bits, (10, 14)).astype(np.uint16)
    rows = bits_ref.pack(x, bits, "msb")
    path = str(tmp_path / "p.tif")
    tiffio.write_packed(path, rows, 14, bits)
    got, W, b = tiffio.read_packed(path)
    assert (W, b) == (14, bits) and got.dtype == np.uint8 and np.array_equal(got, rows)
    assert np.array_equal(bits_ref.unpack(got, W, b, "msb"), x)
    with pytest.raises(tiffio.TiffError, match="unsupported sample type"):
        tiffio.read(path)                                  # `read` keeps its behaviour
    with pytest.raises(tiffio.TiffError):
        tiffio.write_packed(path, rows, 15, bits)          # not that many bytes per row
    with pytest.raises(tiffio.TiffError):
        tiffio.write_packed(path, rows, 14, 11)
    plain = str(tmp_path / "u16.tif")
    tiffio.write(plain, x)
    with pytest.raises(tiffio.TiffError, match="BitsPerSample"):
        tiffio.read_packed(plain)


def test_tiff_packed_two_strips_by_hand(tmp_path):
    """a big-endian file of two strips (3 + 2 rows) that lie in the file in the other order"""
    from rvdd_release_amd import tiffio
    x = np.random.default_rng(5).integers(0, 1 << 12, (5, 6)).astype(np.uint16)
    rows = bits_ref.pack(x, 12, "msb")                     # 9 bytes per row
    s0, s1 = rows[:3].tobytes(), rows[3:].tobytes()
    off1, off0 = 8, 8 + len(s1) + 1                        # strip 1 first, a filler byte, then strip 0
    body = s1 + b"\xEE" + s0
    ifd_off = 8 + len(body) + (len(body) & 1)
    ent = [(256, 3, 1, struct.pack(">HH", 6, 0)), (257, 3, 1, struct.pack(">HH", 5, 0)), (258, 3, 1, struct.pack(">HH", 12, 0)),
           (259, 3, 1, struct.pack(">HH", 1, 0)), (262, 3, 1, struct.pack(">HH", 1, 0)),
           (273, 4, 2, None), (277, 3, 1, struct.pack(">HH", 1, 0)), (278, 3, 1, struct.pack(">HH", 3, 0)), (279, 4, 2, None)]
    extra_off = ifd_off + 2 + 12 * len(ent) + 4
    extra = struct.pack(">II", off0, off1) + struct.pack(">II", len(s0), len(s1))
    ifd = struct.pack(">H", len(ent))
    for tag, typ, cnt, val in ent:
        if val is None:
            val = struct.pack(">I", extra_off + (0 if tag == 273 else 8))
        ifd += struct.pack(">HHI", tag, typ, cnt) + val
    ifd += struct.pack(">I", 0)
    path = str(tmp_path / "two.tif")
    with open(path, "wb") as f:
        f.write(b"MM" + struct.pack(">HI", 42, ifd_off) + body + (b"\0" if len(body) & 1 else b"") + ifd + extra)
    got, W, b = tiffio.read_packed(path)
    assert (W, b) == (6, 12) and np.array_equal(got, rows)
    with pytest.raises(tiffio.TiffError):
        tiffio.read(path)


# ---- the dataset ---------------------------------------------------------------------------------------------------------------
def _tree(root, lengths, bits, form, H=8, W=12, folder="noisy"):
    """<root>/<folder>/<video>/<frame>: form "msb" (TIFF), "mipi" (.raw) or "u16" (TIFF).  -> {video: uint16 [n,H,W]}"""
    from rvdd_release_amd import tiffio
    want = {}
    for v, n in enumerate(lengths):
        key = f"{v:03d}"
        os.makedirs(os.path.join(root, folder, key), exist_ok=True)
        x = np.random.default_rng(50 + v).integers(0, 1 << bits, (n, H, W)).astype(np.uint16)
        for k in range(n):
            stem = os.path.join(root, folder, key, f"{k:08d}")
            if form == "msb":
                tiffio.write_packed(stem + ".tif", bits_ref.pack(x[k], bits, "msb"), W, bits)
            elif form == "mipi":
                bits_ref.pack(x[k], bits, "mipi").tofile(stem + ".raw")
            else:
                tiffio.write(stem + ".tif", x[k])
        want[key] = x
    return want


@pytest.mark.parametrize("form,bits", [("msb", 10), ("msb", 12), ("msb", 14), ("mipi", 10), ("mipi", 12)])
def test_dataset_reads_the_containers_as_they_lie(tmp_path, form, bits):
    from rvdd_release_amd.data import create_dataset
    from rvdd_release_amd.options import make_opt
    W = 14 if form == "msb" else 12                       # 14: odd ww, pad bits
    want = _tree(str(tmp_path), [2, 1], bits, form, W=W)
    extra = dict(raw_container="mipi", raw_size=f"{W}x8") if form == "mipi" else {}
    ds = create_dataset(make_opt(dataroot=str(tmp_path), dataset_mode="rawvideo", serial_batches=True, bit_depth=bits, **extra)).dataset
    assert (ds.container, ds.layout, ds.dtype) == (form, "mosaic", np.dtype(np.uint8)) and len(ds) == 3
    for i, (v, k) in enumerate([("000", 0), ("000", 1), ("001", 0)]):
        d = ds[i]
        assert d["video"] == v and d["FirstOfVideo"] == (k == 0)
        assert d["frame"].dtype == np.uint8 and d["frame"].shape == (8, bits_ref.row_bytes(W, bits, form))
        assert np.array_equal(bits_ref.unpack(d["frame"], W, bits, form), want[v][k])
        assert ds.frame_size(d["n_path"]) == (8, W)


def test_dataset_bit_depth_must_be_the_files(tmp_path):
    from rvdd_release_amd.data import create_dataset
    from rvdd_release_amd.options import make_opt
    _tree(str(tmp_path), [1], 10, "msb")
    with pytest.raises(ValueError, match=r"BitsPerSample is 10 but --bit_depth is 12"):
        create_dataset(make_opt(dataroot=str(tmp_path), dataset_mode="rawvideo", serial_batches=True, bit_depth=12))


def test_dataset_containers_do_not_mix(tmp_path):
    from rvdd_release_amd import tiffio
    from rvdd_release_amd.data import create_dataset
    from rvdd_release_amd.options import make_opt
    want = _tree(str(tmp_path), [2, 2], 12, "msb")
    bad = os.path.join(str(tmp_path), "noisy", "001", "00000001.tif")
    tiffio.write(bad, want["001"][1])                      # a uint16 mosaic among packed frames
    ds = create_dataset(make_opt(dataroot=str(tmp_path), dataset_mode="rawvideo", serial_batches=True, bit_depth=12)).dataset
    assert ds[2]["frame"].dtype == np.uint8
    with pytest.raises(ValueError, match=re.escape(bad)):
        ds[3]
    # and the other way round: a packed frame among uint16 mosaics
    root = str(tmp_path / "b")
    want = _tree(root, [2], 12, "u16")
    bad = os.path.join(root, "noisy", "000", "00000001.tif")
    tiffio.write_packed(bad, bits_ref.pack(want["000"][1], 12, "msb"), 12, 12)
    ds = create_dataset(make_opt(dataroot=root, dataset_mode="rawvideo", serial_batches=True, bit_depth=12)).dataset
    assert ds.container is None and ds[0]["frame"].dtype == np.uint16
    with pytest.raises(ValueError, match=re.escape(bad)):
        ds[1]


def test_dataset_mipi_options(tmp_path):
    from rvdd_release_amd.data import create_dataset
    from rvdd_release_amd.options import make_opt
    _tree(str(tmp_path), [1], 10, "mipi")
    mk = lambda **kw: create_dataset(make_opt(dataroot=str(tmp_path), dataset_mode="rawvideo", serial_batches=True, **kw))
    with pytest.raises(ValueError, match="raw_size"):
        mk(bit_depth=10, raw_container="mipi")
    with pytest.raises(ValueError, match="multiple of 4"):
        mk(bit_depth=10, raw_container="mipi", raw_size="14x8")
    with pytest.raises(ValueError, match="bit_depth"):
        mk(bit_depth=16, raw_container="mipi", raw_size="12x8")
    with pytest.raises(ValueError, match="raw_container"):
        mk(bit_depth=10, raw_container="lsb", raw_size="12x8")
    with pytest.raises(ValueError, match=r"is 160 bytes, the file has 120"):
        mk(bit_depth=10, raw_container="mipi", raw_size="16x8")


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_denoise_argument_errors():
    from rvdd_release_amd.denoise import OUT_FORMATS, _parse
    assert OUT_FORMATS["mosaic_msb"][2] == ".tif" and OUT_FORMATS["mosaic_mipi"][2] == ".raw"
    opt = _parse(["--out_format", "mosaic_msb", "--bit_depth", "10"])
    assert opt.out_bit_depth == 10 and opt.raw_container is None
    opt = _parse(["--out_format", "mosaic_mipi", "--bit_depth", "12", "--raw_container", "mipi", "--raw_size", "64x32"])
    assert (opt.raw_container, opt.raw_size) == ("mipi", "64x32")
    for argv, msg in ((["--out_format", "mosaic_msb", "--bit_depth", "16"], "out_bit_depth"),
                      (["--out_format", "mosaic_mipi", "--out_bit_depth", "11"], "out_bit_depth"),
                      (["--out_format", "mosaic_lsb"], "out_format"),
                      (["--raw_container", "mipi", "--bit_depth", "12"], "raw_size"),
                      (["--raw_container", "mipi", "--raw_size", "64x32", "--bit_depth", "16"], "bit_depth"),
                      (["--raw_container", "tiff", "--raw_size", "64x32"], "raw_container")):
        with pytest.raises(SystemExit, match=msg):
            _parse(argv)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_bits_order_of_header_and_binding_agree():
    from rvdd_release_amd import _lib
    from rvdd_release_amd.runtime import BITS_ORDERS
    txt = open(os.path.join(REPO, "include", "rvdd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"enum\s+rvdd_bits_order\s*\{([^}]*)\}", code)
    assert m
    vals = {k: int(v) for k, v in re.findall(r"\b(RVDD_BITS_[A-Z]+)\s*=\s*(\d+)", m.group(1))}
    assert vals == {"RVDD_BITS_MIPI": _lib.BITS_MIPI, "RVDD_BITS_MSB": _lib.BITS_MSB} == {"RVDD_BITS_MIPI": 0, "RVDD_BITS_MSB": 1}
    assert BITS_ORDERS == {"mipi": 0, "msb": 1} and tuple(BITS_ORDERS) == bits_ref.ORDERS
    assert {"rvdd_ingest_bits", "rvdd_egress_bits"} <= set(_lib.exported_symbols())
    assert re.search(r"\bint\s+rvdd_ingest_bits\s*\(", code) and re.search(r"\bint\s+rvdd_egress_bits\s*\(", code)
    assert len(_lib._PROTOS["rvdd_ingest_bits"][1]) == 10 and len(_lib._PROTOS["rvdd_egress_bits"][1]) == 10
    assert '"stream_container"' in txt


def test_library_exports_the_bits_functions_and_knows_the_option():
    from rvdd_release_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "rvdd_ingest_bits") and hasattr(lib, "rvdd_egress_bits")
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"stream_container" in blob and b"ingest_bits_kernel" in blob and b"egress_bits_kernel" in blob


def test_bits_kernels_use_no_lds_and_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_resources
    from rvdd_release_amd import _lib
    rows = [r for r in kernel_resources.kernel_table(_lib.LIB_PATH) if "_bits_kernel<" in r["name"]]
    assert len(rows) == 24, sorted(r["name"] for r in rows)          # 2 directions x 3 depths x 2 orders x 2 forms
    bad = [(r["name"], {k: v for k, v in r.items() if k != "name"}) for r in rows
           if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)
           or r.get("group_segment_fixed_size", 0)]
    assert not bad, bad
