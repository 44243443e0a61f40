"""A minimal PNG writer and reader for the sheets volume.render_planes draws, written against the published PNG specification (ISO/IEC 15948, RFC 2083) with the
standard library (zlib, struct) and numpy only -- PIL is not a dependency of the product.  Like nifti_min.py and hdf5_min.py this restates documented semantics;
tests/test_png_min.py reads this writer's files with PIL and PIL's files with this reader where PIL is at hand.

Write: 8 bits per sample, greyscale (colour type 0) from uint8 [H, W] or RGB (colour type 2) from uint8 [H, W, 3]; non-interlaced, every row with filter type 0, one
       IDAT chunk, correct CRCs.
Read:  8-bit greyscale / RGB, non-interlaced, all five filter types (None, Sub, Up, Average, Paeth), any number of IDAT chunks, ancillary chunks skipped, every CRC
       checked -- so that files written by other tools can be read in tests.  Everything else (16-bit, palette, alpha, interlaced) is refused with a PngFormatError
       that names the case.
"""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3}                                            # colour type -> samples per pixel, of the types that are read
_COLOUR_NAMES = {0: "greyscale", 2: "RGB", 3: "palette", 4: "greyscale + alpha", 6: "RGB + alpha"}


class PngFormatError(ValueError):
    pass


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(image, level=6):
    """uint8 [H, W] or [H, W, 3] -> the bytes of the file"""
    a = np.asarray(image)
    if a.dtype != np.uint8:
        raise ValueError(f"an image is uint8, not {a.dtype}")
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError(f"an image is [H, W] or [H, W, 3], not {a.shape}")
    H, W = int(a.shape[0]), int(a.shape[1])
    if H < 1 or W < 1:
        raise ValueError(f"an image of {H} x {W} pixels cannot be written: PNG has no empty image")
    rows = np.ascontiguousarray(a).reshape(H, -1)
    raw = np.zeros((H, rows.shape[1] + 1), np.uint8)                # filter type 0 in front of every row
    raw[:, 1:] = rows
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(raw.tobytes(), level)) + _chunk(b"IEND", b"")


def write(path_or_file, image, level=6):
    """image: uint8 [H, W] (greyscale) or [H, W, 3] (RGB); path_or_file: a path, or an object with write()."""
    data = encode(image, level)
    if isinstance(path_or_file, (str, os.PathLike)):
        with open(path_or_file, "wb") as f:
            f.write(data)
    else:
        path_or_file.write(data)


def _unfilter(raw, H, stride, bpp, what):
    out = np.zeros((H, stride), np.uint8)
    prev = np.zeros(stride, np.int64)
    for y in range(H):
        ft = raw[y * (stride + 1)]
        line = np.frombuffer(raw, np.uint8, stride, y * (stride + 1) + 1).astype(np.int64)
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 0xFF
        elif ft == 1:                                               # Sub: a running sum over the samples of one channel
            cur = line.copy()
            for c in range(bpp):
                cur[c::bpp] = np.cumsum(line[c::bpp]) & 0xFF
        elif ft in (3, 4):                                          # Average, Paeth: each byte needs its reconstructed left neighbour
            cur = np.zeros(stride, np.int64)
            for x in range(stride):
                a = cur[x - bpp] if x >= bpp else 0
                b = prev[x]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = prev[x - bpp] if x >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (line[x] + pred) & 0xFF
        else:
            raise PngFormatError(f"{what}: row {y} has filter type {ft}, which PNG does not define")
        out[y] = cur
        prev = cur
    return out


def decode(data, what="<bytes>"):
    """the bytes of a file -> uint8 [H, W] or [H, W, 3]"""
    if data[:8] != SIGNATURE:
        raise PngFormatError(f"{what}: not a PNG file (signature {bytes(data[:8])!r})")
    pos, ihdr, idat, ended = 8, None, [], False
    while pos + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if len(body) != n or pos + 12 + n > len(data):
            raise PngFormatError(f"{what}: chunk {kind!r} is cut short")
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        if crc != (zlib.crc32(kind + body) & 0xFFFFFFFF):
            raise PngFormatError(f"{what}: chunk {kind!r} fails its CRC")
        pos += 12 + n
        if ihdr is None and kind != b"IHDR":
            raise PngFormatError(f"{what}: the first chunk is {kind!r}, not IHDR")
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            ended = True
            break
        elif not (kind[0] & 0x20):                                  # an upper-case first letter: a critical chunk this reader does not know
            raise PngFormatError(f"{what}: critical chunk {kind!r} is not supported")
    if ihdr is None or not ended:
        raise PngFormatError(f"{what}: no IHDR or no IEND chunk")
    W, H, depth, colour, comp, filt, interlace = ihdr
    if depth != 8:
        raise PngFormatError(f"{what}: {depth} bits per sample are not supported (8 only)")
    if colour not in _CHANNELS:
        raise PngFormatError(f"{what}: colour type {colour} ({_COLOUR_NAMES.get(colour, 'unknown')}) is not supported (greyscale and RGB only)")
    if interlace != 0:
        raise PngFormatError(f"{what}: interlaced (Adam7) files are not supported")
    if comp != 0 or filt != 0 or W < 1 or H < 1:
        raise PngFormatError(f"{what}: compression method {comp}, filter method {filt}, {W} x {H} pixels")
    ch = _CHANNELS[colour]
    stride = W * ch
    try:
        raw = zlib.decompress(b"".join(idat))
    except zlib.error as e:
        raise PngFormatError(f"{what}: the image data do not inflate ({e})") from None
    if len(raw) != H * (stride + 1):
        raise PngFormatError(f"{what}: {len(raw)} bytes of image data, {H * (stride + 1)} expected")
    out = _unfilter(raw, H, stride, ch, what)
    return out.reshape(H, W) if ch == 1 else out.reshape(H, W, 3)


def read(path):
    """-> uint8 [H, W] (greyscale) or [H, W, 3] (RGB)"""
    with open(path, "rb") as f:
        return decode(f.read(), str(path))
