"""A minimal NIfTI-1 reader and writer: what `nib.load(path)` + `get_fdata()` need for the CT scans and masks of the reference (T1:285-286,
317-318), written against the published NIfTI-1 specification (nifti1.h) with the standard library and numpy only -- nibabel is not installed
here, so like hdf5_min.py this restates documented semantics ("parity unpinned": tests/test_nifti_min.py builds its files with struct.pack at
the specification's byte offsets, independently of this writer; the day nibabel is at hand the same files pin it).

Read:  single-file NIfTI-1 (`.nii`, magic `n+1\\0`), or `.nii.gz` through gzip; both byte orders (found from sizeof_hdr == 348); vox_offset honoured;
       uint8, int8, int16, uint16, int32, uint32, float32, float64; 3-D data, or more dimensions when every trailing one is 1; Fortran order
       (dim[1] fastest).
Write: a uint8 or float32 volume with the geometry of a source header (dim, pixdim, qform / sform, xyzt_units), scl_slope = 1, scl_inter = 0.
Everything else is refused with a NiftiFormatError that names the case.

Orientation: `affine` is the sform when sform_code > 0, else the qform (quaternion, pixdim, qfac, qoffset exactly as nifti1.h states them) when qform_code > 0, else
None; `axcodes` names the direction in which every voxel axis grows, in NIfTI's RAS+ world (+x = the patient's right, +y = anterior, +z = superior).  The rule of
axcodes_from_affine is stated there; for axis-aligned and mildly oblique affines it gives what nibabel's aff2axcodes gives ("parity unpinned", like the rest).
"""
from __future__ import annotations

import gzip
import struct

import numpy as np

HEADER_BYTES = 348
# NIfTI-1 datatype code -> numpy type (without byte order)
DTYPES = {2: "u1", 256: "i1", 4: "i2", 512: "u2", 8: "i4", 768: "u4", 16: "f4", 64: "f8"}
_REFUSED_TYPES = {1: "binary (1 bit)", 32: "complex64", 1792: "complex128", 2048: "complex256", 128: "RGB24", 2304: "RGBA32", 1536: "float128", 1024: "int64",
                  1280: "uint64", 0: "unknown (0)"}
_CODE_OF = {np.dtype(v).newbyteorder("=").str[1:]: k for k, v in DTYPES.items()}


class NiftiFormatError(ValueError):
    pass


class NiftiVolume:
    """What a read returns: `raw` (the voxels as stored, numpy [X, Y, Z] in Fortran order, native byte order), `slope` / `inter` (scl_slope, scl_inter as
    stored), `pixdim` (pixdim[1:4]), `header` (the 348 header bytes, for a mask written with the same geometry), `byteorder` ('<' or '>'); from the header's
    orientation fields `affine` (float64 4 x 4, None when qform_code and sform_code are both 0), `affine_source` ("sform", "qform" or None) and `axcodes` (three letters,
    None without an affine; an affine with a zero or non-finite column raises NiftiFormatError when the codes are asked for)."""

    def __init__(self, raw, slope, inter, pixdim, header, byteorder):
        self.raw, self.slope, self.inter, self.pixdim, self.header, self.byteorder = raw, slope, inter, pixdim, header, byteorder
        self.affine, self.affine_source = affine_of_header(header)

    @property
    def axcodes(self):
        return None if self.affine is None else axcodes_from_affine(self.affine)

    @property
    def shape(self):
        return self.raw.shape

    @property
    def scaling(self):
        return scaling(self.slope, self.inter)

    def get_fdata(self):
        return apply_scaling(self.raw, self.slope, self.inter)

    def __iter__(self):                                        # raw, (slope, inter), pixdim, header = read(path)
        return iter((self.raw, (self.slope, self.inter), self.pixdim, self.header))


def scaling(slope, inter):
    """nibabel's reading of (scl_slope, scl_inter): None when the data are not scaled (slope 0 or not finite), else (slope, inter) as float64 with a
    non-finite inter counted as 0."""
    slope, inter = float(slope), float(inter)
    if slope == 0.0 or not np.isfinite(slope):
        return None
    return slope, (inter if np.isfinite(inter) else 0.0)


def apply_scaling(raw, slope, inter):
    """get_fdata(): float64; (float64(v) * slope) + inter -- two rounded operations -- when the header scales, else the cast alone."""
    a = np.asarray(raw).astype(np.float64)
    sc = scaling(slope, inter)
    if sc is None:
        return a
    a *= sc[0]
    a += sc[1]
    return a


def _read_all(path):
    path = str(path)
    if path.endswith(".hdr") or path.endswith(".img"):
        raise NiftiFormatError(f"{path}: a .hdr / .img pair is not supported (single-file .nii / .nii.gz only)")
    with open(path, "rb") as f:
        head = f.read(2)
        f.seek(0)
        if head == b"\x1f\x8b":
            with gzip.GzipFile(fileobj=f) as g:
                return g.read()
        return f.read()


def parse_header(buf):
    """(byteorder, fields) of the 348 header bytes; raises NiftiFormatError for what this reader refuses."""
    if len(buf) < 4:
        raise NiftiFormatError("file too short for a NIfTI header")
    (le,), (be,) = struct.unpack("<i", buf[:4]), struct.unpack(">i", buf[:4])
    if le == 540 or be == 540:
        raise NiftiFormatError("NIfTI-2 file (sizeof_hdr == 540) is not supported")
    if le == HEADER_BYTES:
        bo = "<"
    elif be == HEADER_BYTES:
        bo = ">"
    else:
        raise NiftiFormatError(f"not a NIfTI-1 file: sizeof_hdr is {le}, not 348, in either byte order")
    if len(buf) < HEADER_BYTES:
        raise NiftiFormatError("file too short for a NIfTI header: fewer than 348 bytes")
    magic = bytes(buf[344:348])
    if magic == b"ni1\x00":
        raise NiftiFormatError("NIfTI-1 .hdr / .img pair (magic 'ni1') is not supported (single-file 'n+1' only)")
    if magic != b"n+1\x00":
        raise NiftiFormatError(f"not a single-file NIfTI-1 file: magic {magic!r}")
    dim = struct.unpack(bo + "8h", buf[40:56])
    datatype, bitpix = struct.unpack(bo + "2h", buf[70:74])
    pixdim = struct.unpack(bo + "8f", buf[76:108])
    vox_offset, slope, inter = struct.unpack(bo + "3f", buf[108:120])
    qform_code, sform_code = struct.unpack(bo + "2h", buf[252:256])
    quatern = struct.unpack(bo + "3f", buf[256:268])
    qoffset = struct.unpack(bo + "3f", buf[268:280])
    srow = struct.unpack(bo + "12f", buf[280:328])
    return bo, {"dim": dim, "datatype": datatype, "bitpix": bitpix, "pixdim": pixdim, "vox_offset": vox_offset, "scl_slope": slope, "scl_inter": inter,
                "xyzt_units": buf[123], "qform_code": qform_code, "sform_code": sform_code, "quatern_b": quatern[0], "quatern_c": quatern[1], "quatern_d": quatern[2],
                "qoffset_x": qoffset[0], "qoffset_y": qoffset[1], "qoffset_z": qoffset[2], "srow_x": srow[0:4], "srow_y": srow[4:8], "srow_z": srow[8:12]}


# the two letters of every world axis of RAS+: (negative direction, positive direction)
AXIS_LETTERS = (("L", "R"), ("P", "A"), ("I", "S"))


def affine_from_fields(h):
    """The voxel -> world matrix of parsed header fields -> (float64 4 x 4, "sform" | "qform"), or (None, None) when both codes are 0.  sform_code > 0: the three srow
    rows.  Otherwise qform_code > 0, nifti1.h's method 2: a = sqrt(max(0, 1 - b^2 - c^2 - d^2)), R the nine-term rotation matrix of (a, b, c, d), column j scaled by
    pixdim[j + 1], the third column also by qfac (-1 only when pixdim[0] == -1, else +1), translation qoffset.  All in float64 from the stored float32 values."""
    if h["sform_code"] > 0:
        m = np.eye(4)
        m[0], m[1], m[2] = (np.asarray(h[k], np.float64) for k in ("srow_x", "srow_y", "srow_z"))
        return m, "sform"
    if h["qform_code"] > 0:
        b, c, d = float(h["quatern_b"]), float(h["quatern_c"]), float(h["quatern_d"])
        a = float(np.sqrt(max(0.0, 1.0 - b * b - c * c - d * d)))
        R = np.array([[a * a + b * b - c * c - d * d, 2.0 * b * c - 2.0 * a * d, 2.0 * b * d + 2.0 * a * c],
                      [2.0 * b * c + 2.0 * a * d, a * a + c * c - b * b - d * d, 2.0 * c * d - 2.0 * a * b],
                      [2.0 * b * d - 2.0 * a * c, 2.0 * c * d + 2.0 * a * b, a * a + d * d - c * c - b * b]], np.float64)
        qfac = -1.0 if float(h["pixdim"][0]) == -1.0 else 1.0
        m = np.eye(4)
        m[:3, :3] = R * np.array([float(h["pixdim"][1]), float(h["pixdim"][2]), float(h["pixdim"][3]) * qfac], np.float64)[None, :]
        m[:3, 3] = [float(h["qoffset_x"]), float(h["qoffset_y"]), float(h["qoffset_z"])]
        return m, "qform"
    return None, None


def affine_of_header(header):
    """(affine, source) of 348 header bytes (see affine_from_fields)"""
    return affine_from_fields(parse_header(header)[1])


def axcodes_from_affine(affine):
    """Three letters: the world direction in which voxel axes 0, 1, 2 grow.  (1) the three columns of affine[:3, :3] are normalised to unit length -- a zero or
    non-finite column raises NiftiFormatError; (2) for voxel axes 0, 1, 2 in that order: the world axis with the largest absolute component among those not yet taken,
    ties to the lowest world axis; (3) R / A / S when that component is positive, L / P / I when it is negative."""
    m = np.asarray(affine, np.float64)
    if m.shape not in ((4, 4), (3, 3), (3, 4)) or not np.isfinite(m[:3, :3]).all():
        raise NiftiFormatError(f"an affine is a finite 4 x 4 matrix, not {m.shape}" if m.shape not in ((4, 4), (3, 3), (3, 4)) else "the affine has a non-finite column")
    rz = m[:3, :3]
    norms = np.sqrt((rz * rz).sum(axis=0))
    if not np.isfinite(norms).all() or (norms == 0).any():
        raise NiftiFormatError(f"the affine has a zero or non-finite column (column lengths {norms.tolist()}): no orientation can be read from it")
    unit = rz / norms[None, :]
    taken, codes = [], []
    for j in range(3):
        best = None
        for w in range(3):
            if w not in taken and (best is None or abs(unit[w, j]) > abs(unit[best, j])):
                best = w
        taken.append(best)
        codes.append(AXIS_LETTERS[best][1 if unit[best, j] > 0 else 0])
    return tuple(codes)


def check_axcodes(codes):
    """A 3-letter string or tuple with one letter from each of L/R, P/A, I/S -> [(world axis, sign)] per voxel axis; anything else raises ValueError."""
    try:
        letters = tuple(str(c) for c in codes)
    except TypeError:
        raise ValueError(f"axis codes are three letters, one from each of L/R, P/A, I/S, not {codes!r}") from None
    if len(letters) != 3:
        raise ValueError(f"axis codes are three letters, one from each of L/R, P/A, I/S, not {codes!r}")
    out = []
    for c in letters:
        hit = [(w, 1.0 if pair[1] == c else -1.0) for w, pair in enumerate(AXIS_LETTERS) if c in pair]
        if len(c) != 1 or not hit:
            raise ValueError(f"axis codes are three letters, one from each of L/R, P/A, I/S, not {codes!r}")
        out.append(hit[0])
    if sorted(w for w, _ in out) != [0, 1, 2]:
        raise ValueError(f"axis codes take one letter from each of L/R, P/A, I/S, not {codes!r}")
    return out


def affine_from_axcodes(codes, pixdim=(1.0, 1.0, 1.0)):
    """The axis-aligned affine (float64 4 x 4, no translation) whose axcodes_from_affine is `codes`: voxel axis j grows by pixdim[j] mm along its letter."""
    axes = check_axcodes(codes)
    p = np.asarray(pixdim, np.float64).reshape(-1)
    if p.shape != (3,) or not np.isfinite(p).all() or not (p > 0).all():
        raise ValueError(f"pixdim is three positive finite numbers, not {pixdim!r}")
    m = np.zeros((4, 4))
    m[3, 3] = 1.0
    for j, (w, sign) in enumerate(axes):
        m[w, j] = sign * p[j]
    return m


def read(path):
    """-> NiftiVolume (unpacks as raw, (slope, inter), pixdim[1:4], header bytes)."""
    buf = _read_all(path)
    bo, h = parse_header(buf)
    code = h["datatype"]
    if code not in DTYPES:
        raise NiftiFormatError(f"datatype {code} ({_REFUSED_TYPES.get(code, 'not a NIfTI-1 code')}) is not supported: only uint8, int8, int16, uint16, int32, uint32, "
                               "float32, float64")
    dim = h["dim"]
    nd = dim[0]
    if not 3 <= nd <= 7:
        raise NiftiFormatError(f"dim[0] = {nd}: only 3-D data (or more dimensions with every trailing one equal to 1)")
    if any(d != 1 for d in dim[4:nd + 1]):
        raise NiftiFormatError(f"truly {nd}-D data (dim = {list(dim[1:nd + 1])}): only volumes whose dimensions past the third are 1")
    shape = tuple(int(d) for d in dim[1:4])
    if any(d < 1 for d in shape):
        raise NiftiFormatError(f"dim = {list(dim[1:4])}: every dimension must be positive")
    dt = np.dtype(DTYPES[code]).newbyteorder(bo)
    nvox = shape[0] * shape[1] * shape[2]
    off = int(h["vox_offset"])
    if off < HEADER_BYTES + 4:
        off = HEADER_BYTES + 4                                  # (a single file's data cannot start before byte 352)
    if len(buf) < off + nvox * dt.itemsize:
        raise NiftiFormatError(f"file too short: {len(buf)} bytes, but vox_offset {off} + {nvox} voxels x {dt.itemsize} bytes = {off + nvox * dt.itemsize}")
    raw = np.frombuffer(buf, dt, nvox, off).reshape(shape, order="F")
    raw = raw.astype(dt.newbyteorder("="), order="F")           # native byte order, own memory (Fortran order kept)
    return NiftiVolume(raw, float(np.float32(h["scl_slope"])), float(np.float32(h["scl_inter"])), tuple(float(p) for p in h["pixdim"][1:4]), bytes(buf[:HEADER_BYTES]), bo)


def default_header(shape, pixdim=(1.0, 1.0, 1.0)):
    """The 348 bytes of a little-endian NIfTI-1 header for a bare [X, Y, Z] volume (no qform / sform), for volumes that did not come from a file."""
    h = bytearray(HEADER_BYTES)
    struct.pack_into("<i", h, 0, HEADER_BYTES)
    struct.pack_into("<8h", h, 40, 3, int(shape[0]), int(shape[1]), int(shape[2]), 1, 1, 1, 1)
    struct.pack_into("<8f", h, 76, 1.0, float(pixdim[0]), float(pixdim[1]), float(pixdim[2]), 0.0, 0.0, 0.0, 0.0)
    h[123] = 2                                                   # NIFTI_UNITS_MM
    h[344:348] = b"n+1\x00"
    return bytes(h)


def header_with_affine(shape, affine):
    """The 348 bytes of a little-endian NIfTI-1 header for an [X, Y, Z] volume that lies at `affine` (voxel -> RAS+ world, 4 x 4 or its top 3 x 4): sform_code = 1 with
    the three srow rows (stored as float32, so a read gives the affine back rounded to float32), pixdim = the lengths of the three columns, qform_code = 0, millimetres.
    A non-finite affine or a zero column raises NiftiFormatError."""
    m = np.asarray(affine, np.float64)
    if m.shape not in ((4, 4), (3, 4)) or not np.isfinite(m).all():
        raise NiftiFormatError(f"an affine is a finite 4 x 4 (or 3 x 4) matrix, not {m.shape}" if m.shape not in ((4, 4), (3, 4)) else "the affine has a non-finite entry")
    norms = np.sqrt((m[:3, :3] * m[:3, :3]).sum(axis=0))
    if not np.isfinite(norms).all() or (norms == 0).any():
        raise NiftiFormatError(f"the affine has a zero or non-finite column (column lengths {norms.tolist()})")
    h = bytearray(default_header(shape, norms))
    struct.pack_into("<2h", h, 252, 0, 1)                        # qform_code, sform_code (NIFTI_XFORM_SCANNER_ANAT)
    struct.pack_into("<12f", h, 280, *(float(v) for v in m[:3, :4].reshape(-1)))
    return bytes(h)


def write(path, volume, header=None, pixdim=(1.0, 1.0, 1.0)):
    """Write a uint8 or float32 [X, Y, Z] volume as `.nii`, or gzip-compressed when the path ends in `.gz`.  `header`: the 348 bytes of the source
    (NiftiVolume.header) -- its dim, pixdim, qform / sform fields, xyzt_units and byte order are kept byte for byte; datatype, bitpix, vox_offset = 352,
    scl_slope = 1, scl_inter = 0 and the calibration range are set for the new data."""
    vol = np.asarray(volume)
    if vol.ndim != 3 or vol.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise NiftiFormatError(f"write: a 3-D uint8 or float32 volume is expected, not {vol.dtype} with {vol.ndim} dimensions")
    if header is None:
        header = default_header(vol.shape, pixdim)
    bo, h = parse_header(header)
    if tuple(h["dim"][1:4]) != tuple(vol.shape):
        raise NiftiFormatError(f"write: the volume is {tuple(vol.shape)} but the source header says {tuple(h['dim'][1:4])}")
    out = bytearray(header[:HEADER_BYTES])
    code = _CODE_OF[vol.dtype.str[1:]]
    struct.pack_into(bo + "2h", out, 70, code, vol.dtype.itemsize * 8)
    struct.pack_into(bo + "3f", out, 108, 352.0, 1.0, 0.0)
    struct.pack_into(bo + "2f", out, 124, 0.0, 0.0)              # cal_max, cal_min: no display range
    out[344:348] = b"n+1\x00"
    data = np.asarray(vol, vol.dtype.newbyteorder(bo)).tobytes(order="F")
    blob = bytes(out) + b"\x00\x00\x00\x00" + data                # (four extension bytes: no extensions)
    if str(path).endswith(".gz"):
        with open(path, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", compresslevel=1, mtime=0, filename="") as g:
            g.write(blob)
    else:
        with open(path, "wb") as f:
            f.write(blob)
