"""A minimal PNG writer and reader for the display transform's 8-bit output (take_amd.capi.tonemap): 8-bit truecolour
with or without alpha, no interlace, every scanline with filter type 0, one IDAT chunk.  Standard library only (zlib,
struct).  read_png reads what write_png writes — and any non-interlaced 8-bit RGB / RGBA file whose scanlines use
filter type 0 — and refuses the rest."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_COLOUR_TYPE = {3: 2, 4: 6}  # channels -> PNG colour type (truecolour, truecolour with alpha)


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png(path, img, level=6):
    """img: uint8 (H, W, 3) or (H, W, 4), row 0 = top -> the file at `path`"""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in _COLOUR_TYPE or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes a non-empty (H, W, 3) or (H, W, 4) uint8 array")
    h, w, c = a.shape
    rows = np.zeros((h, 1 + w * c), np.uint8)  # the filter byte (0: none), then the scanline
    rows[:, 1:] = a.reshape(h, w * c)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, _COLOUR_TYPE[c], 0, 0, 0)
    with open(path, "wb") as f:
        f.write(SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)) + _chunk(b"IEND", b""))


def read_png(path):
    """-> uint8 (H, W, 3) or (H, W, 4); ValueError for a file that is not a PNG of the kind write_png writes"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != SIGNATURE:
        raise ValueError(f"{path}: not a PNG file")
    pos, ihdr, idat, ended = 8, None, [], False
    while pos + 12 <= len(data) and not ended:
        (n,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise ValueError(f"{path}: truncated chunk")
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise ValueError(f"{path}: bad CRC in chunk {kind!r}")
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
        pos += 12 + n
    if ihdr is None or not ended:
        raise ValueError(f"{path}: missing IHDR or IEND")
    w, h, depth, colour, compression, filtering, interlace = ihdr
    channels = {v: k for k, v in _COLOUR_TYPE.items()}.get(colour)
    if depth != 8 or channels is None or compression or filtering or interlace or w < 1 or h < 1:
        raise ValueError(f"{path}: only non-interlaced 8-bit RGB / RGBA is read")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    if raw.size != h * (1 + w * channels):
        raise ValueError(f"{path}: wrong amount of image data")
    rows = raw.reshape(h, 1 + w * channels)
    if rows[:, 0].any():
        raise ValueError(f"{path}: only filter type 0 is read")
    return rows[:, 1:].reshape(h, w, channels).copy()
