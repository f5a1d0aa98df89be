"""CPU side of the KITTI Scene Flow preparation: the PNG reader and writer (ogc_amd/data_prepare/png16.py, csrc/png_unfilter.h
through ogc_png_unfilter), the fixture tests/golden/kittisf_prepare.npz and its mirror, the ABI wiring of ogc_kittisf_unproject,
and the refusals of scan_ops.kittisf_unproject that need no device."""
import ctypes
import io
import json
import os
import struct
import sys
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = {"grey8": (np.uint8, ()), "grey16": (np.uint16, ()), "rgb16": (np.uint16, (3,))}


@pytest.fixture(scope="module")
def golden():
    data = np.load(os.path.join(HERE, "golden", "kittisf_prepare.npz"))
    return data, json.loads(str(data["meta"]))


@pytest.fixture(scope="module")
def mirror():
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_kittisf_prepare_golden
    return make_kittisf_prepare_golden


@pytest.fixture(scope="module")
def lib():
    from ogc_amd.csrc import build as b
    L = ctypes.CDLL(b.build())
    L.ogc_png_unfilter.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.ogc_png_unfilter.restype = ctypes.c_int
    L.ogc_last_error.restype = ctypes.c_char_p
    return L


def write(tmp_path, name, data):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(bytes(data))
    return path


def test_read_png_equals_the_fixture_and_pil(golden, tmp_path):
    from PIL import Image

    from ogc_amd.data_prepare.png16 import read_png
    data, meta = golden
    assert len(meta["png_files"]) == 19 and sum("two_idat" in f for f in meta["png_files"]) == 1
    for name in meta["png_files"]:
        kind = name.split("_")[1]
        want = data["png_%s_array" % kind]
        got = read_png(write(tmp_path, name + ".png", data[name]))
        assert got.dtype == want.dtype == KINDS[kind][0] and got.shape == want.shape == (5, 7) + KINDS[kind][1], name
        assert got.dtype.isnative and np.array_equal(got, want), name
        if kind != "rgb16":
            assert np.array_equal(np.array(Image.open(io.BytesIO(bytes(data[name])))), got), name
    assert bytes(data["png_rgb16_two_idat"]).count(b"IDAT") == 2


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("shape", ((1, 1), (1, 300), (37, 53)))
def test_write_then_read_round_trips(kind, shape, tmp_path):
    from ogc_amd.data_prepare.png16 import read_png, write_png
    dtype, tail = KINDS[kind]
    rs = np.random.RandomState(shape[0] * 1000 + shape[1])
    array = rs.randint(0, np.iinfo(dtype).max + 1, size=shape + tail).astype(dtype)
    array[0, 0] = np.iinfo(dtype).max                                   # the wrap-around of every filter's arithmetic
    path = str(tmp_path / "a.png")
    for filters in [[k] * shape[0] for k in range(5)] + [None, rs.randint(0, 5, size=shape[0])]:
        write_png(path, array, filters)
        got = read_png(path)
        assert got.dtype == dtype and np.array_equal(got, array), (kind, shape, filters)
    # a smooth image, where the predictors are close: differences of both signs
    ramp = (np.add.outer(np.arange(shape[0]) * 7, np.arange(shape[1]) * 3)[..., None] + np.arange(3) * 50)
    ramp = (ramp if tail else ramp[..., 0]).astype(dtype)
    write_png(path, ramp)
    assert np.array_equal(read_png(path), ramp)


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def png_bytes(width, height, depth, colour, interlace, stream):
    from ogc_amd.data_prepare.png16 import SIGNATURE
    return (SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, colour, 0, 0, interlace))
            + chunk(b"IDAT", zlib.compress(stream)) + chunk(b"IEND", b""))


def test_malformed_files_raise_value_error(golden, tmp_path):
    from ogc_amd.data_prepare.png16 import SIGNATURE, read_png
    data, _ = golden
    good = bytes(data["png_grey16_mixed"])
    rows = b"".join(b"\x00" + bytes(14) for _ in range(5))             # 5 rows of 7 grey 16-bit pixels, filter None
    cases = {
        "truncated_in_idat": good[:len(good) - 20],
        "truncated_before_iend": good[:len(good) - 12],
        "truncated_header": good[:20],
        "bad_signature": b"\x89PNX" + good[4:],
        "interlaced": png_bytes(7, 5, 16, 0, 1, rows),
        "palette": png_bytes(7, 5, 8, 3, 0, b"".join(b"\x00" + bytes(7) for _ in range(5))),
        "grey_alpha": png_bytes(7, 5, 8, 4, 0, rows),
        "depth_4": png_bytes(7, 5, 4, 0, 0, b"".join(b"\x00" + bytes(4) for _ in range(5))),
        "filter_5": png_bytes(7, 5, 16, 0, 0, rows[:30] + b"\x05" + rows[31:]),
        "short_stream": png_bytes(7, 5, 16, 0, 0, rows[:-1]),
        "long_stream": png_bytes(7, 5, 16, 0, 0, rows + b"\x00"),
        "not_zlib": SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", 7, 5, 16, 0, 0, 0, 0)) + chunk(b"IDAT", b"no deflate stream")
        + chunk(b"IEND", b""),
    }
    assert np.array_equal(read_png(write(tmp_path, "ok.png", png_bytes(7, 5, 16, 0, 0, rows))), np.zeros((5, 7), np.uint16))
    for name, content in cases.items():
        path = write(tmp_path, name + ".png", content)
        with pytest.raises(ValueError) as e:
            read_png(path)
        assert path in str(e.value), name
    assert "filter byte" in str(pytest.raises(ValueError, read_png, write(tmp_path, "f5.png", cases["filter_5"])).value)


def test_png_unfilter_refusals(lib):
    src = np.zeros(5 * 15, dtype=np.uint8)
    dst = np.full(5 * 14 + 8, 0xAB, dtype=np.uint8)

    def call(a, b, height, row_bytes, bpp):
        rc = lib.ogc_png_unfilter(a, b, height, row_bytes, bpp)
        return rc, lib.ogc_last_error().decode()
    assert call(src.ctypes.data, dst.ctypes.data, 5, 14, 2)[0] == 0
    assert not dst[:70].any() and (dst[70:] == 0xAB).all()              # nothing behind height * row_bytes is touched
    for args, word in (((None, dst.ctypes.data, 5, 14, 2), "null"), ((src.ctypes.data, None, 5, 14, 2), "null"),
                       ((src.ctypes.data, dst.ctypes.data, 5, 14, 4), "bpp"), ((src.ctypes.data, dst.ctypes.data, 5, 14, 0), "bpp"),
                       ((src.ctypes.data, dst.ctypes.data, 5, 14, 3), "multiple"), ((src.ctypes.data, dst.ctypes.data, 5, 14, 6), "multiple"),
                       ((src.ctypes.data, dst.ctypes.data, -1, 14, 2), "negative")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (args[2:], rc, msg)
    src[2 * 15] = 5
    rc, msg = call(src.ctypes.data, dst.ctypes.data, 5, 14, 2)
    assert rc == -1 and "filter byte" in msg and "row 2" in msg


def test_png_unfilter_every_filter_against_the_definition(lib):
    """Each filter type, each bpp, against a byte-by-byte statement of the PNG specification's reconstruction functions."""
    rs = np.random.RandomState(3)
    for bpp in (1, 2, 3, 6):
        height, row_bytes = 6, bpp * 5
        stream = rs.randint(0, 256, size=(height, 1 + row_bytes)).astype(np.uint8)
        stream[:, 0] = [4, 3, 2, 1, 0, 4]
        want = np.zeros((height, row_bytes), dtype=np.int64)
        for y in range(height):
            for x in range(row_bytes):
                a = want[y, x - bpp] if x >= bpp else 0
                b = want[y - 1, x] if y > 0 else 0
                c = want[y - 1, x - bpp] if y > 0 and x >= bpp else 0
                p = a + b - c
                paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else (b if abs(p - b) <= abs(p - c) else c)
                pred = (0, a, b, (a + b) // 2, paeth)[stream[y, 0]]
                want[y, x] = (int(stream[y, 1 + x]) + pred) % 256
        got = np.zeros((height, row_bytes), dtype=np.uint8)
        assert lib.ogc_png_unfilter(stream.ctypes.data, got.ctypes.data, height, row_bytes, bpp) == 0
        assert np.array_equal(got, want), bpp


def test_fixture_is_complete_and_the_mirror_reproduces_it(golden, mirror):
    data, meta = golden
    assert os.path.getsize(os.path.join(HERE, "golden", "kittisf_prepare.npz")) < 256 * 1024
    assert meta["tile"] == 1024 and meta["select_semantics"] == [26, 28] and meta["depth_thresh"] == 35.0
    assert [(c["height"], c["width"]) for c in (meta["cases"]["a"], meta["cases"]["b"])] == [(25, 41), (32, 96)]
    P = data["P_rect"]
    assert P.dtype == np.float32 and P.shape == (3, 4) and np.array_equal(P, mirror.p_rect())
    for name, case in meta["cases"].items():
        h, w = case["height"], case["width"]
        maps = [data["%s_%s" % (name, k)] for k in ("disp1", "disp2", "flow", "inst")]
        assert all(m.dtype == np.uint16 for m in maps) and [m.shape for m in maps] == [(h, w), (h, w), (h, w, 3), (h, w)]
        pc1, pc2, segm, keep_idx = (data["%s_%s" % (name, k)] for k in ("pc1", "pc2", "segm", "keep_idx"))
        m = case["kept"]
        assert 0 < m < case["valid"] < case["pixels"] == h * w
        assert pc1.shape == pc2.shape == (m, 3) and pc1.dtype == pc2.dtype == np.float32
        assert segm.shape == keep_idx.shape == (m,) and segm.dtype == np.int64 and keep_idx.dtype == np.int32
        assert (pc1[:, 2] < 35.0).all() and (pc2[:, 2] < 35.0).all() and pc1[:, 2].max() > 30.0
        got = mirror.unproject_mirror(*maps, P)
        for g, want in zip(got, (pc1, pc2, segm, keep_idx)):
            assert g.dtype == want.dtype and np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g,
                                                            want.view(np.int32) if want.dtype == np.float32 else want)
        # labels: selected ids among the kept pixels, in ascending order; unselected ids are present too
        ids = maps[3].reshape(-1)[keep_idx].astype(np.int64)
        chosen = sorted(i for i in set(ids.tolist()) if (i >> 8) in (26, 28))
        assert len(chosen) >= 2 and any((i >> 8) not in (26, 28) and i > 0 for i in set(ids.tolist()))
        assert np.array_equal(segm, np.array([chosen.index(i) + 1 if i in chosen else 0 for i in ids.tolist()]))


def test_library_exports_the_entry_points(lib):
    from ogc_amd import _lib
    from ogc_amd import pointnet2_cuda as nat
    for name in ("ogc_kittisf_unproject", "ogc_png_unfilter"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["ogc_kittisf_unproject"][-1] is ctypes.c_void_p and len(_lib.SIGNATURES["ogc_kittisf_unproject"]) == 22
    assert _lib.SIGNATURES["ogc_png_unfilter"][-1] is ctypes.c_int      # no stream: not a launching entry point
    lib.ogc_scan_crop_tile.restype = ctypes.c_int
    assert lib.ogc_scan_crop_tile() == nat.SCAN_CROP_TILE               # the tile of the unprojection kernels too
    assert callable(nat.kittisf_unproject_wrapper) and callable(nat.png_unfilter)
    header = open(os.path.join(os.path.dirname(HERE), "include", "ogc_ops.h")).read()
    assert "int ogc_kittisf_unproject(int height, int width," in header and "int ogc_png_unfilter(" in header


def test_read_kittisf_calib(tmp_path):
    from ogc_amd.data_prepare.kitti_io import read_kittisf_calib
    line = "P_rect_02: 7.215377e+02 0.000000e+00 6.095593e+02 4.485728e+01 0.000000e+00 7.215377e+02 1.728540e+02 2.163791e-01 0.000000e+00 0.000000e+00 1.000000e+00 2.745884e-03\n"
    path = write(tmp_path, "c.txt", ("calib_time: 09-Jan-2012 13:57:47\n" + line + "P_rect_03: 1 0 0 0 0 1 0 0 0 0 1 0\n").encode())
    P = read_kittisf_calib(path)
    assert P.dtype == np.float32 and P.shape == (3, 4) and P[0, 0] == np.float32(721.5377) and P[2, 3] == np.float32(0.002745884)
    with pytest.raises(ValueError):
        read_kittisf_calib(write(tmp_path, "d.txt", (line + line).encode()))
    with pytest.raises(ValueError):
        read_kittisf_calib(write(tmp_path, "e.txt", line.replace("7.215377e+02 1.728540e+02", "7.2e+02 1.728540e+02").encode()))


def test_kittisf_unproject_has_no_cpu_path(golden):
    from ogc_amd.data_prepare import scan_ops
    from ogc_amd.pointnet2_cuda import U16
    data, _ = golden
    P = data["P_rect"]
    maps = [torch.from_numpy(data["a_" + k].view(np.int16)).view(U16) for k in ("disp1", "disp2", "flow", "inst")]
    with pytest.raises(RuntimeError):
        scan_ops.kittisf_unproject(*maps, P)                            # CPU tensors
    with pytest.raises(TypeError):
        scan_ops.kittisf_unproject(maps[0].to(torch.int32), *maps[1:], P)
    with pytest.raises(TypeError):
        scan_ops.kittisf_unproject(maps[0], maps[1], maps[2].to(torch.float32), maps[3], P)
    with pytest.raises(TypeError):
        scan_ops.kittisf_unproject(data["a_disp1"], *maps[1:], P)       # numpy
    with pytest.raises(ValueError):
        scan_ops.kittisf_unproject(maps[0].reshape(-1), *maps[1:], P)
