"""CPU: the orientation fields of nifti_min (qform / sform -> affine, axcodes).  Headers are built here with struct.pack at nifti1.h's byte offsets, independently of
the reader; nibabel is not installed, so the axis-code rule is the one nifti_min.axcodes_from_affine states ("parity unpinned")."""
import gzip
import itertools
import struct

import numpy as np
import pytest

PIXDIM = (0.5, 0.75, 2.5)
LETTERS = (("L", "R"), ("P", "A"), ("I", "S"))


def _header(bo="<", shape=(4, 3, 2), pixdim=PIXDIM, qfac=1.0, qform_code=0, sform_code=0, quatern=(0.0, 0.0, 0.0), qoffset=(0.0, 0.0, 0.0), srow=None):
    h = bytearray(348)
    struct.pack_into(bo + "i", h, 0, 348)
    struct.pack_into(bo + "8h", h, 40, 3, shape[0], shape[1], shape[2], 1, 1, 1, 1)
    struct.pack_into(bo + "2h", h, 70, 2, 8)                         # uint8
    struct.pack_into(bo + "8f", h, 76, qfac, pixdim[0], pixdim[1], pixdim[2], 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(bo + "3f", h, 108, 352.0, 0.0, 0.0)
    h[123] = 2
    struct.pack_into(bo + "2h", h, 252, qform_code, sform_code)
    struct.pack_into(bo + "3f", h, 256, *quatern)
    struct.pack_into(bo + "3f", h, 268, *qoffset)
    if srow is not None:
        struct.pack_into(bo + "12f", h, 280, *np.asarray(srow, np.float64).reshape(-1))
    h[344:348] = b"n+1\x00"
    return bytes(h)


def _file(tmp_path, header, name="v.nii", shape=(4, 3, 2)):
    data = np.arange(int(np.prod(shape)), dtype=np.uint8)
    p = tmp_path / name
    blob = header + b"\0\0\0\0" + data.tobytes()
    p.write_bytes(gzip.compress(blob, 1) if name.endswith(".gz") else blob)
    return p, data.reshape(shape, order="F")


def _quat_rotation(b, c, d):
    a = np.sqrt(max(0.0, 1.0 - b * b - c * c - d * d))
    return np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                     [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                     [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])


SROW = [[-0.5, 0.0, 0.0, 120.0], [0.0, -0.75, 0.0, 90.5], [0.0, 0.0, 2.5, -300.0]]          # an axial CT as most scanners write it: LPS


@pytest.mark.parametrize("bo", ["<", ">"])
def test_parse_header_returns_the_orientation_fields(bo):
    from covidseg_amd import nifti_min
    h = _header(bo, qfac=-1.0, qform_code=1, sform_code=2, quatern=(0.0, 1.0, 0.0), qoffset=(1.5, -2.5, 3.25), srow=SROW)
    got_bo, f = nifti_min.parse_header(h)
    assert got_bo == bo and f["qform_code"] == 1 and f["sform_code"] == 2
    assert (f["quatern_b"], f["quatern_c"], f["quatern_d"]) == (0.0, 1.0, 0.0)
    assert (f["qoffset_x"], f["qoffset_y"], f["qoffset_z"]) == (1.5, -2.5, 3.25)
    assert tuple(f["srow_x"]) == tuple(SROW[0]) and tuple(f["srow_y"]) == tuple(SROW[1]) and tuple(f["srow_z"]) == tuple(SROW[2])
    assert f["pixdim"][0] == -1.0 and tuple(f["dim"][1:4]) == (4, 3, 2)


@pytest.mark.parametrize("bo", ["<", ">"])
def test_sform_wins_over_qform(tmp_path, bo):
    from covidseg_amd import nifti_min
    p, data = _file(tmp_path, _header(bo, qform_code=1, sform_code=1, quatern=(0.0, 0.0, 0.0), srow=SROW))
    v = nifti_min.read(p)
    assert v.affine_source == "sform" and v.affine.dtype == np.float64 and v.affine.shape == (4, 4)
    assert np.array_equal(v.affine, np.array(SROW + [[0.0, 0.0, 0.0, 1.0]]))
    assert v.axcodes == ("L", "P", "S") and np.array_equal(v.raw, data) and v.byteorder == bo


@pytest.mark.parametrize("bo", ["<", ">"])
def test_qform_only_with_qfac_minus_one(tmp_path, bo):
    from covidseg_amd import nifti_min
    b, c, d = 0.0, 0.0, 1.0                                          # a half turn about z: x -> -x, y -> -y
    p, _ = _file(tmp_path, _header(bo, qfac=-1.0, qform_code=1, quatern=(b, c, d), qoffset=(10.0, 20.0, 30.0), srow=SROW))          # (the srow is ignored: sform_code = 0)
    v = nifti_min.read(p)
    want = np.eye(4)
    want[:3, :3] = _quat_rotation(b, c, d) * np.array([np.float32(PIXDIM[0]), np.float32(PIXDIM[1]), -np.float32(PIXDIM[2])], np.float64)[None, :]
    want[:3, 3] = (10.0, 20.0, 30.0)
    assert v.affine_source == "qform" and np.array_equal(v.affine, want)
    assert v.axcodes == ("L", "P", "I")                              # qfac = -1 turns the third axis over
    q = nifti_min.read(_file(tmp_path, _header(bo, qfac=0.0, qform_code=1, quatern=(b, c, d)), "q0.nii")[0])          # qfac is -1 only when pixdim[0] == -1
    assert q.axcodes == ("L", "P", "S")
    # a general unit quaternion: the nine-term matrix, a from the three stored float32 values
    bcd = tuple(float(np.float32(t)) for t in (0.1, -0.2, 0.3))
    g = nifti_min.read(_file(tmp_path, _header(bo, qform_code=2, quatern=bcd), "g.nii")[0])
    R = _quat_rotation(*bcd)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12)
    assert np.array_equal(g.affine[:3, :3], R * np.array([np.float32(t) for t in PIXDIM], np.float64)[None, :])


def test_identity_quaternion_is_ras(tmp_path):
    from covidseg_amd import nifti_min
    v = nifti_min.read(_file(tmp_path, _header(qform_code=1))[0])
    assert v.axcodes == ("R", "A", "S")
    assert np.array_equal(v.affine, np.diag([np.float32(PIXDIM[0]), np.float32(PIXDIM[1]), np.float32(PIXDIM[2]), 1.0]).astype(np.float64))


def test_no_codes_no_orientation(tmp_path):
    from covidseg_amd import nifti_min
    v = nifti_min.read(_file(tmp_path, _header(srow=SROW, quatern=(0.0, 0.0, 1.0)))[0])          # fields filled in, both codes 0
    assert v.affine is None and v.axcodes is None and v.affine_source is None
    d = nifti_min.NiftiVolume(np.zeros((2, 2, 2), np.uint8), 0.0, 0.0, (1.0, 1.0, 1.0), nifti_min.default_header((2, 2, 2)), "<")
    assert d.affine is None and d.axcodes is None and d.affine_source is None


def test_all_48_axis_codes_round_trip():
    from covidseg_amd import nifti_min
    seen = set()
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((0, 1), repeat=3):
            c = tuple(LETTERS[w][s] for w, s in zip(perm, signs))
            a = nifti_min.affine_from_axcodes(c, PIXDIM)
            assert a.dtype == np.float64 and a.shape == (4, 4) and np.array_equal(a[3], [0, 0, 0, 1])
            assert np.array_equal(np.abs(a[:3, :3]).sum(axis=0), PIXDIM) and np.count_nonzero(a[:3, :3]) == 3
            assert nifti_min.axcodes_from_affine(a) == c
            assert np.array_equal(nifti_min.affine_from_axcodes("".join(c), PIXDIM), a)          # a string is taken as well
            seen.add(c)
    assert len(seen) == 48
    for bad in ("RAR", "RA", "RASS", "XAS", "ras", ("R", "A"), ("R", "L", "S"), 5, ("RA", "S", "I"), ""):
        with pytest.raises(ValueError):
            nifti_min.affine_from_axcodes(bad, PIXDIM)
    for bad in ((1, 1), (1, 1, 0), (1, -1, 1), (1, 1, np.nan)):
        with pytest.raises(ValueError):
            nifti_min.affine_from_axcodes("RAS", bad)


def test_a_ten_degree_oblique_sform_keeps_the_aligned_code(tmp_path):
    from covidseg_amd import nifti_min
    t = np.deg2rad(10.0)
    rz = np.array([[np.cos(t), -np.sin(t), 0.0], [np.sin(t), np.cos(t), 0.0], [0.0, 0.0, 1.0]])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(t), -np.sin(t)], [0.0, np.sin(t), np.cos(t)]])
    for codes in (("L", "P", "S"), ("R", "A", "S"), ("P", "S", "R"), ("I", "L", "A")):
        base = nifti_min.affine_from_axcodes(codes, PIXDIM)
        for rot in (rz, rx, rz @ rx):
            a = base.copy()
            a[:3, :3] = rot @ base[:3, :3]
            assert nifti_min.axcodes_from_affine(a) == codes
            v = nifti_min.read(_file(tmp_path, _header(sform_code=1, srow=a[:3]))[0])
            assert v.axcodes == codes
    # the rule's order: voxel axis 0 chooses first, a tie goes to the lowest world axis
    tie = np.eye(4); tie[:3, :3] = [[1.0, 1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 0.0, 1.0]]
    assert nifti_min.axcodes_from_affine(tie) == ("R", "P", "S")


def test_a_zero_or_non_finite_column_is_refused(tmp_path):
    from covidseg_amd import nifti_min
    zero = [[1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]
    v = nifti_min.read(_file(tmp_path, _header(sform_code=1, srow=zero))[0])          # the voxels still read; the codes are refused
    assert v.affine_source == "sform"
    with pytest.raises(nifti_min.NiftiFormatError):
        v.axcodes
    for bad in (np.zeros((4, 4)), np.diag([1.0, np.inf, 1.0, 1.0]), np.diag([1.0, np.nan, 1.0, 1.0])):
        with pytest.raises(nifti_min.NiftiFormatError):
            nifti_min.axcodes_from_affine(bad)


def test_a_file_without_orientation_reads_as_before(tmp_path):
    from covidseg_amd import nifti_min
    raw = (np.arange(24, dtype=np.uint8) % 5).reshape((4, 3, 2), order="F")
    p = tmp_path / "plain.nii.gz"
    nifti_min.write(p, raw, pixdim=PIXDIM)
    v = nifti_min.read(p)
    r, (slope, inter), pixdim, header = v
    assert np.array_equal(r, raw) and r.flags.f_contiguous and (slope, inter) == (1.0, 0.0) and v.scaling == (1.0, 0.0)
    assert pixdim == tuple(float(np.float32(t)) for t in PIXDIM) and v.byteorder == "<" and len(header) == 348
    assert header[252:328] == bytes(76) and v.affine is None and v.axcodes is None and v.affine_source is None
    assert nifti_min.default_header((4, 3, 2), PIXDIM)[252:328] == bytes(76)
    # a written copy of an oriented file keeps its orientation fields byte for byte
    src, _ = _file(tmp_path, _header(">", qform_code=1, sform_code=1, quatern=(0.0, 0.0, 1.0), srow=SROW), "o.nii")
    o = nifti_min.read(src)
    nifti_min.write(tmp_path / "copy.nii", np.asarray(o.raw), o.header)
    c = nifti_min.read(tmp_path / "copy.nii")
    assert c.header[252:328] == o.header[252:328] and np.array_equal(c.affine, o.affine) and c.axcodes == o.axcodes == ("L", "P", "S")
