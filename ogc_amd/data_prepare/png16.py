"""A PNG reader and writer for the 16-bit maps of KITTI Scene Flow (disparity, optical flow, instance ids), on zlib and numpy
alone — PIL opens a 16-bit RGB file as 8-bit, and no other decoder is a dependency of this package.

    read_png(path) -> (H, W) or (H, W, 3) array, uint8 or native uint16
    write_png(path, array, filters=None)

Bit depth 8 or 16, colour type 0 (grey) or 2 (RGB), not interlaced; everything else is a ValueError that names the file.  The
reader walks the chunks, inflates the concatenated IDAT data, undoes the row filters with the library's host function
ogc_png_unfilter (csrc/png_unfilter.h: sequential per byte) and swaps the big-endian samples.  The writer exists for synthetic
roots and test fixtures: filtering needs only the original neighbours, so it is plain numpy."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunks(data, path):
    pos = len(SIGNATURE)
    while True:
        if pos + 8 > len(data):
            raise ValueError("%s: truncated PNG, no IEND chunk" % path)
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + length > len(data):
            raise ValueError("%s: truncated PNG, chunk %r runs past the end of the file" % (path, kind))
        yield kind, data[pos + 8:pos + 8 + length]
        if kind == b"IEND":
            return
        pos += 12 + length


def read_png(path):
    with open(path, "rb") as f:
        data = f.read()
    if data[:len(SIGNATURE)] != SIGNATURE:
        raise ValueError("%s: not a PNG file (bad signature)" % path)
    header, idat = None, []
    for kind, body in _chunks(data, path):
        if kind == b"IHDR":
            if len(body) != 13:
                raise ValueError("%s: IHDR chunk of %d bytes" % (path, len(body)))
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
    if header is None:
        raise ValueError("%s: no IHDR chunk" % path)
    width, height, depth, colour, compression, filter_method, interlace = header
    if width == 0 or height == 0:
        raise ValueError("%s: empty image (%d x %d)" % (path, width, height))
    if depth not in (8, 16):
        raise ValueError("%s: bit depth %d, only 8 and 16 are read" % (path, depth))
    if colour not in (0, 2):
        raise ValueError("%s: colour type %d, only grey (0) and RGB (2) are read" % (path, colour))
    if compression != 0 or filter_method != 0:
        raise ValueError("%s: compression method %d, filter method %d" % (path, compression, filter_method))
    if interlace != 0:
        raise ValueError("%s: interlaced PNGs are not read" % path)
    channels = 3 if colour == 2 else 1
    bpp = channels * depth // 8
    row_bytes = width * bpp
    try:
        stream = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise ValueError("%s: the image data do not inflate (%s)" % (path, e))
    if len(stream) != height * (1 + row_bytes):
        raise ValueError("%s: the image data inflate to %d bytes, %d rows of 1 + %d bytes need %d"
                         % (path, len(stream), height, row_bytes, height * (1 + row_bytes)))
    from .. import _lib, pointnet2_cuda
    try:
        rows = pointnet2_cuda.png_unfilter(stream, height, row_bytes, bpp)
    except _lib.OgcOpsError as e:
        raise ValueError("%s: %s" % (path, e))
    if depth == 16:
        rows = rows.view(">u2").astype(np.uint16)
    return rows.reshape((height, width, 3) if channels == 3 else (height, width))


def _filter_row(kind, cur, up, bpp):
    """One row of bytes (int16 arithmetic, reduced modulo 256 at the end) under PNG filter type `kind`."""
    left = np.zeros_like(cur)
    left[bpp:] = cur[:-bpp]
    if kind == 0:
        out = cur
    elif kind == 1:
        out = cur - left
    elif kind == 2:
        out = cur - up
    elif kind == 3:
        out = cur - ((left + up) >> 1)
    else:
        corner = np.zeros_like(up)
        corner[bpp:] = up[:-bpp]
        p = left + up - corner
        pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - corner)
        out = cur - np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, corner))
    return (out & 0xFF).astype(np.uint8)


def encode_png(array, filters=None, idat_chunks=1):
    """The bytes of a PNG file of `array` ((H, W) or (H, W, 3), uint8 or uint16); `filters` one filter type (0-4) per row, by
    default cycling through all five; the compressed data split over `idat_chunks` IDAT chunks."""
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16):
        raise ValueError("array must be uint8 or uint16, got %s" % array.dtype)
    if array.ndim not in (2, 3) or (array.ndim == 3 and array.shape[2] != 3) or array.shape[0] == 0 or array.shape[1] == 0:
        raise ValueError("array must be a non-empty (H, W) or (H, W, 3), got %s" % (array.shape,))
    height, width = array.shape[:2]
    depth = 8 * array.dtype.itemsize
    bpp = (3 if array.ndim == 3 else 1) * array.dtype.itemsize
    rows = np.ascontiguousarray(array.astype(">u2") if depth == 16 else array).view(np.uint8).reshape(height, width * bpp).astype(np.int16)
    filters = [y % 5 for y in range(height)] if filters is None else [int(k) for k in filters]
    if len(filters) != height or any(k < 0 or k > 4 for k in filters):
        raise ValueError("filters must hold one filter type 0..4 per row")
    zero = np.zeros(width * bpp, dtype=np.int16)
    stream = b"".join(bytes([k]) + _filter_row(k, rows[y], rows[y - 1] if y > 0 else zero, bpp).tobytes() for y, k in enumerate(filters))
    packed = zlib.compress(stream, 6)

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    step = max(1, -(-len(packed) // max(1, int(idat_chunks))))
    parts = [packed[i:i + step] for i in range(0, len(packed), step)]
    return (SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, 2 if array.ndim == 3 else 0, 0, 0, 0))
            + b"".join(chunk(b"IDAT", p) for p in parts) + chunk(b"IEND", b""))


def write_png(path, array, filters=None):
    with open(path, "wb") as f:
        f.write(encode_png(array, filters))
