"""CPU: nifti_min against files built here with struct.pack at the byte offsets of the NIfTI-1 specification (nifti1.h), independently of its writer."""
import gzip
import struct

import numpy as np
import pytest

from covidseg_amd import nifti_min as N

TYPES = {2: "u1", 256: "i1", 4: "i2", 512: "u2", 8: "i4", 768: "u4", 16: "f4", 64: "f8"}
SHAPE = (5, 4, 3)                                                    # non-cubic: a transposed or C-ordered read cannot pass


def make_nifti(data_bytes, code, bitpix, bo="<", dim=(3, 5, 4, 3, 1, 1, 1, 1), pixdim=(1.0, 0.75, 0.5, 2.5, 0.0, 0.0, 0.0, 0.0), vox_offset=400.0, slope=0.0, inter=0.0,
               magic=b"n+1\x00", sizeof_hdr=348, pad=None):
    h = bytearray(348)
    struct.pack_into(bo + "i", h, 0, sizeof_hdr)
    struct.pack_into(bo + "8h", h, 40, *dim)
    struct.pack_into(bo + "h", h, 70, code)
    struct.pack_into(bo + "h", h, 72, bitpix)
    struct.pack_into(bo + "8f", h, 76, *pixdim)
    struct.pack_into(bo + "f", h, 108, vox_offset)
    struct.pack_into(bo + "f", h, 112, slope)
    struct.pack_into(bo + "f", h, 116, inter)
    h[123] = 10                                                      # xyzt_units: mm + s
    struct.pack_into(bo + "2h", h, 252, 1, 2)                        # qform_code, sform_code
    struct.pack_into(bo + "6f", h, 256, 0.1, 0.2, 0.3, -10.0, -20.0, 30.0)
    struct.pack_into(bo + "12f", h, 280, *[float(i) - 3.5 for i in range(12)])
    h[344:348] = magic
    gap = int(vox_offset) - 348 if pad is None else pad
    return bytes(h) + b"\xAB" * gap + data_bytes


def ramp(kind):
    n = int(np.prod(SHAPE))
    a = np.arange(n, dtype=np.float64)
    if kind in ("i1", "i2", "i4", "f4", "f8"):
        a = a - 17
    if kind in ("f4", "f8"):
        a = a * 0.37
    return a.astype(kind)                                            # element i = voxel (x, y, z) with i = x + 5 (y + 4 z)


@pytest.mark.parametrize("gz", [False, True])
@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("code", sorted(TYPES))
def test_reads_every_type_both_byte_orders_plain_and_gzip(tmp_path, code, bo, gz):
    kind = TYPES[code]
    flat = ramp(kind)
    blob = make_nifti(flat.astype(np.dtype(kind).newbyteorder(bo)).tobytes(), code, np.dtype(kind).itemsize * 8, bo)
    path = tmp_path / ("a.nii.gz" if gz else "a.nii")
    path.write_bytes(gzip.compress(blob) if gz else blob)
    vol = N.read(path)
    raw, (slope, inter), pixdim, header = vol
    assert raw.shape == SHAPE and raw.dtype == np.dtype(kind) and raw.dtype.isnative
    for x, y, z in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (4, 3, 2), (2, 1, 1)):
        assert raw[x, y, z] == flat[x + 5 * (y + 4 * z)]            # Fortran order: dim[1] fastest
    assert np.array_equal(raw.reshape(-1, order="F"), flat)
    assert pixdim == (0.75, 0.5, 2.5) and header == blob[:348] and vol.byteorder == bo
    assert vol.get_fdata().dtype == np.float64 and np.array_equal(vol.get_fdata(), raw.astype(np.float64))          # slope 0: not scaled


def test_scaling_rules_case_by_case(tmp_path):
    flat = ramp("i2")

    def fdata(slope, inter):
        p = tmp_path / "s.nii"
        p.write_bytes(make_nifti(flat.tobytes(), 4, 16, slope=slope, inter=inter))
        return N.read(p).get_fdata().reshape(-1, order="F")
    f64 = flat.astype(np.float64)
    assert np.array_equal(fdata(0.0, 5.0), f64)                     # slope 0: no scaling at all (inter ignored too)
    assert np.array_equal(fdata(float("nan"), 5.0), f64)
    assert np.array_equal(fdata(float("inf"), 5.0), f64)
    s = float(np.float32(0.1)); i = float(np.float32(-1024.3))
    assert np.array_equal(fdata(0.1, -1024.3), f64 * s + i)          # two rounded float64 operations on the float32 header values
    assert np.array_equal(fdata(0.1, float("nan")), f64 * s)         # a non-finite inter counts as 0
    assert np.array_equal(fdata(2.0, float("inf")), f64 * 2.0)
    assert N.scaling(0.0, 1.0) is None and N.scaling(float("nan"), 1.0) is None and N.scaling(2.0, float("nan")) == (2.0, 0.0)
    # not an fma: a product that rounds before the sum
    v = np.array([3], np.int32); sl = float(np.float32(1 / 3)); it = -1.0
    assert N.apply_scaling(v, sl, it)[0] == np.float64(3.0 * sl) + it


def test_trailing_unit_dimensions_are_accepted(tmp_path):
    flat = ramp("u1")
    p = tmp_path / "t.nii"
    p.write_bytes(make_nifti(flat.tobytes(), 2, 8, dim=(5, 5, 4, 3, 1, 1, 1, 1)))
    assert N.read(p).raw.shape == SHAPE


@pytest.mark.parametrize("kw,match", [
    (dict(sizeof_hdr=540), "NIfTI-2"),
    (dict(magic=b"ni1\x00"), "pair"),
    (dict(code=32), "complex64"),
    (dict(code=1792), "complex128"),
    (dict(code=128), "RGB24"),
    (dict(code=2304), "RGBA32"),
    (dict(code=1536), "float128"),
    (dict(dim=(4, 5, 4, 3, 2, 1, 1, 1)), "truly 4-D"),
    (dict(short=True), "too short"),
    (dict(sizeof_hdr=123), "sizeof_hdr"),
])
def test_refusals_name_their_case(tmp_path, kw, match):
    kw = dict(kw)
    code = kw.pop("code", 4)
    short = kw.pop("short", False)
    data = ramp("i2").tobytes()
    blob = make_nifti(data[:-2] if short else data, code, 16, **kw)
    p = tmp_path / "r.nii"
    p.write_bytes(blob)
    with pytest.raises(N.NiftiFormatError, match=match):
        N.read(p)


@pytest.mark.parametrize("bo", ["<", ">"])
@pytest.mark.parametrize("suffix", [".nii", ".nii.gz"])
@pytest.mark.parametrize("kind", ["u1", "f4"])
def test_writer_round_trip_keeps_the_source_geometry_byte_for_byte(tmp_path, kind, suffix, bo):
    src = make_nifti(ramp("i2").astype(np.dtype("i2").newbyteorder(bo)).tobytes(), 4, 16, bo, slope=0.5, inter=-100.0)
    vol = (np.arange(60).reshape(SHAPE, order="F") % 7).astype(kind)
    out = tmp_path / ("m" + suffix)
    N.write(out, vol, src[:348])
    back = N.read(out)
    assert np.array_equal(back.raw, vol) and back.raw.dtype == np.dtype(kind)
    assert (back.slope, back.inter) == (1.0, 0.0) and back.pixdim == (0.75, 0.5, 2.5)
    h = back.header
    for lo, hi in ((40, 56), (76, 108), (123, 124), (252, 328)):     # dim, pixdim, xyzt_units, qform_code .. srow_z
        assert h[lo:hi] == src[lo:hi]
    blob = gzip.decompress(out.read_bytes()) if suffix.endswith(".gz") else out.read_bytes()
    assert struct.unpack(bo + "f", blob[108:112])[0] == 352.0 and len(blob) == 352 + vol.nbytes
    with pytest.raises(N.NiftiFormatError, match="source header"):
        N.write(tmp_path / "x.nii", vol[:4], src[:348])
    with pytest.raises(N.NiftiFormatError, match="uint8 or float32"):
        N.write(tmp_path / "x.nii", vol.astype(np.int16), src[:348])


def test_writer_without_a_source_header(tmp_path):
    vol = (np.arange(24).reshape((2, 3, 4), order="F")).astype(np.uint8)
    N.write(tmp_path / "d.nii.gz", vol, pixdim=(0.5, 0.5, 2.0))
    back = N.read(tmp_path / "d.nii.gz")
    assert np.array_equal(back.raw, vol) and back.pixdim == (0.5, 0.5, 2.0)
