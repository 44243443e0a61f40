"""CPU: png_min writes files other tools read and reads files other tools write.  PIL is used where it is installed (it is not a dependency of the product); the chunk
structure and the CRCs are also checked against the specification directly, so the file is not its own witness where PIL is missing."""
import io
import struct
import zlib

import numpy as np
import pytest

from covidseg_amd import png_min

RNG = np.random.default_rng(5)
IMAGES = {"grey": RNG.integers(0, 256, (9, 13), dtype=np.uint8), "rgb": RNG.integers(0, 256, (6, 7, 3), dtype=np.uint8),          # 7 x 3 bytes per row: no multiple of 4
          "one_grey": np.array([[200]], np.uint8), "one_rgb": np.array([[[1, 2, 3]]], np.uint8), "wide": RNG.integers(0, 256, (2, 301, 3), dtype=np.uint8)}


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_write_then_read(tmp_path, name):
    a = IMAGES[name]
    p = tmp_path / "a.png"
    png_min.write(p, a)
    b = png_min.read(p)
    assert b.dtype == np.uint8 and b.shape == a.shape and np.array_equal(a, b)
    f = io.BytesIO()
    png_min.write(f, a)                                             # a file object
    assert f.getvalue() == p.read_bytes()


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_the_file_is_what_the_specification_says(name):
    a = IMAGES[name]
    data = png_min.encode(a)
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, kinds, idat = 8, [], b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        kinds.append(kind)
        if kind == b"IHDR":
            assert struct.unpack(">IIBBBBB", body) == (a.shape[1], a.shape[0], 8, 0 if a.ndim == 2 else 2, 0, 0, 0)
        if kind == b"IDAT":
            idat += body
        pos += 12 + n
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and pos == len(data)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(a.shape[0], -1)
    assert (raw[:, 0] == 0).all() and np.array_equal(raw[:, 1:], a.reshape(a.shape[0], -1))          # filter type 0 on every row


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_pil_opens_what_is_written(tmp_path, name):
    Image = pytest.importorskip("PIL.Image")
    a = IMAGES[name]
    p = tmp_path / "a.png"
    png_min.write(p, a)
    with Image.open(p) as im:
        assert im.mode == ("L" if a.ndim == 2 else "RGB")
        assert np.array_equal(np.asarray(im), a)


def _filtered(a, ft):
    """the rows of `a` filtered with type ft as the specification defines it, written here independently of the reader"""
    H = a.shape[0]
    bpp = 1 if a.ndim == 2 else 3
    rows = a.reshape(H, -1).astype(np.int64)
    out = bytearray()
    for y in range(H):
        cur, up = rows[y], rows[y - 1] if y else np.zeros_like(rows[0])
        left = np.concatenate([np.zeros(bpp, np.int64), cur[:-bpp]])
        ul = np.concatenate([np.zeros(bpp, np.int64), up[:-bpp]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) // 2
        else:
            p = left + up - ul
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
        out += bytes([ft]) + ((cur - pred) & 0xFF).astype(np.uint8).tobytes()
    return bytes(out)


def _file(a, raw, depth=8, colour=None, interlace=0, split=1):
    colour = (0 if a.ndim == 2 else 2) if colour is None else colour
    ch = lambda k, d: struct.pack(">I", len(d)) + k + d + struct.pack(">I", zlib.crc32(k + d) & 0xFFFFFFFF)
    z = zlib.compress(raw)
    cut = [len(z) * i // split for i in range(split + 1)]
    return (b"\x89PNG\r\n\x1a\n" + ch(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], depth, colour, 0, 0, interlace)) + ch(b"tEXt", b"Comment\0made by hand") +
            b"".join(ch(b"IDAT", z[cut[i]:cut[i + 1]]) for i in range(split)) + ch(b"IEND", b""))


@pytest.mark.parametrize("ft", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", ["grey", "rgb", "one_rgb"])
def test_every_filter_type_reads_back(ft, name):
    a = IMAGES[name]
    assert np.array_equal(png_min.decode(_file(a, _filtered(a, ft), split=3)), a)          # three IDAT chunks and an ancillary chunk in front of them


def test_a_pil_file_with_adaptive_filters_reads_back(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    yy, xx = np.mgrid[0:40, 0:53]
    smooth = np.stack([(3 * xx + yy) % 256, (xx * yy // 7) % 256, (5 * yy) % 256], -1).astype(np.uint8)          # gradients: the encoder picks non-zero filters
    for a in (smooth, smooth[:, :, 1], IMAGES["rgb"]):
        p = tmp_path / "p.png"
        Image.fromarray(a).save(p, optimize=True)
        assert np.array_equal(png_min.read(p), a)
    Image.fromarray(smooth).save(p)
    raw =zlib.decompress(b"".join(c for k, c in _chunks(p.read_bytes()) if k == b"IDAT"))
    assert set(raw[::smooth.shape[1] * 3 + 1]) - {0}, "PIL used filter 0 only: the test would not see the other filters"


def _chunks(data):
    pos = 8
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        yield kind, data[pos + 8:pos + 8 + n]
        pos += 12 + n


def test_what_is_not_supported_is_refused(tmp_path):
    a = IMAGES["grey"]
    raw = _filtered(a, 0)
    with pytest.raises(png_min.PngFormatError, match="16 bits"):
        png_min.decode(_file(a, raw, depth=16))
    with pytest.raises(png_min.PngFormatError, match="interlaced"):
        png_min.decode(_file(a, raw, interlace=1))
    with pytest.raises(png_min.PngFormatError, match="colour type 6"):
        png_min.decode(_file(a, raw, colour=6))
    with pytest.raises(png_min.PngFormatError, match="colour type 3"):
        png_min.decode(_file(a, raw, colour=3))
    with pytest.raises(png_min.PngFormatError, match="signature"):
        png_min.decode(b"GIF89a" + bytes(40))
    good = bytearray(_file(a, raw))
    good[40] ^= 1                                                   # inside the tEXt chunk
    with pytest.raises(png_min.PngFormatError, match="CRC"):
        png_min.decode(bytes(good))
    with pytest.raises(png_min.PngFormatError, match="filter type 7"):
        png_min.decode(_file(a, bytes([7]) + raw[1:]))
    with pytest.raises(png_min.PngFormatError, match="expected"):
        png_min.decode(_file(a, raw[:-3]))
    Image = pytest.importorskip("PIL.Image")
    p = tmp_path / "deep.png"
    Image.fromarray((np.arange(12, dtype=np.uint16) * 5000).reshape(3, 4)).save(p)          # a real 16-bit file
    with pytest.raises(png_min.PngFormatError, match="16 bits"):
        png_min.read(p)


def test_bad_images_are_refused():
    for bad in (np.zeros((3, 3), np.float32), np.zeros((3, 3, 4), np.uint8), np.zeros((3,), np.uint8), np.zeros((0, 3), np.uint8)):
        with pytest.raises(ValueError):
            png_min.encode(bad)
