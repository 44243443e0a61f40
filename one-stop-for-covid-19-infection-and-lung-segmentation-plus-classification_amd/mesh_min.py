"""Triangle meshes on disk with the standard library and numpy only, beside png_min and nifti_min: what volume.extract_surface hands to a viewer, a printer or a planning tool.

    write_stl(path, vertices, triangles)              binary STL: 80-byte header, uint32 count, 50 bytes per facet (normal, three corners, attribute 0), little endian
    write_ply(path, vertices, triangles, groups)      PLY binary_little_endian 1.0: float x y z, faces as `list uchar int vertex_indices`, `int group` per face with groups
    write_obj(path, vertices, triangles, groups)      Wavefront OBJ text: v lines with 9 significant digits (a float32 round-trips), f lines 1-based, a `g group_<n>` line
                                                      in front of every run of one group
    read_stl(path) -> (facets float32 [nt, 3, 3], normals float32 [nt, 3])      an STL holds no indices: the corners come back per facet
    read_ply(path) -> (vertices float32 [nv, 3], triangles int32 [nt, 3], groups int32 [nt] or None)      the files write_ply writes
    write(path, vertices, triangles, groups)          by suffix: .stl, .ply, .obj

A facet normal is the normalised cross product (b - a) x (c - a) in float32 arithmetic, and (0, 0, 0) for a degenerate facet (a zero or non-finite length).  Units and
frame are the caller's: the writers store the numbers they are given."""
from __future__ import annotations

import os
import struct

import numpy as np

STL_HEADER_BYTES, STL_FACET_BYTES = 80, 50
_FACET = np.dtype([("normal", "<f4", (3,)), ("corners", "<f4", (3, 3)), ("attribute", "<u2")])
assert _FACET.itemsize == STL_FACET_BYTES


def _check(vertices, triangles, groups=None):
    v = np.asarray(vertices)
    t = np.asarray(triangles)
    if v.ndim != 2 or v.shape[1] != 3 or v.dtype.kind not in "fiu":
        raise ValueError(f"vertices are [nv, 3] numbers, not {v.dtype} {v.shape}")
    if t.ndim != 2 or t.shape[1] != 3 or t.dtype.kind not in "iu":
        raise ValueError(f"triangles are [nt, 3] integers, not {t.dtype} {t.shape}")
    v = np.ascontiguousarray(v, "<f4")
    t64 = t.astype(np.int64)
    if t64.size and (t64.min() < 0 or t64.max() >= v.shape[0]):
        raise ValueError(f"a triangle names a vertex outside 0..{v.shape[0] - 1}")
    g = None
    if groups is not None:
        g = np.asarray(groups)
        if g.shape != (t.shape[0],) or g.dtype.kind not in "iu":
            raise ValueError(f"groups are [nt] = [{t.shape[0]}] integers, not {g.dtype} {g.shape}")
        g = np.ascontiguousarray(g, "<i4")
    return v, np.ascontiguousarray(t64, "<i4"), g


def facet_normals(corners):
    """float32 [nt, 3, 3] -> the unit normals in float32 arithmetic, zero where the cross product has no finite positive length"""
    c = np.asarray(corners, np.float32)
    u, w = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    with np.errstate(all="ignore"):
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1).astype(np.float32)
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]).astype(np.float32)
        ok = np.isfinite(length) & (length > 0)
        out = np.where(ok[:, None], n / np.where(ok, length, np.float32(1))[:, None], np.float32(0)).astype(np.float32)
    return out


def stl_bytes(vertices, triangles, header=b"covidseg_amd mesh_min binary STL"):
    v, t, _ = _check(vertices, triangles)
    if len(header) > STL_HEADER_BYTES or header[:5].lower() == b"solid":
        raise ValueError("an STL header is at most 80 bytes and does not begin with 'solid' (that marks the text format)")
    rec = np.zeros(t.shape[0], _FACET)
    rec["corners"] = v[t]
    rec["normal"] = facet_normals(rec["corners"])
    return header.ljust(STL_HEADER_BYTES, b"\0") + struct.pack("<I", t.shape[0]) + rec.tobytes()


def write_stl(path, vertices, triangles, header=b"covidseg_amd mesh_min binary STL"):
    data = stl_bytes(vertices, triangles, header)
    with open(path, "wb") as f:
        f.write(data)


def read_stl(path):
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < STL_HEADER_BYTES + 4:
        raise ValueError(f"{path}: shorter than a binary STL's header")
    (n,) = struct.unpack_from("<I", data, STL_HEADER_BYTES)
    if len(data) != STL_HEADER_BYTES + 4 + n * STL_FACET_BYTES:
        raise ValueError(f"{path}: {n} facets need {STL_HEADER_BYTES + 4 + n * STL_FACET_BYTES} bytes, the file has {len(data)}")
    rec = np.frombuffer(data, _FACET, n, STL_HEADER_BYTES + 4)
    return rec["corners"].astype(np.float32), rec["normal"].astype(np.float32)


def ply_bytes(vertices, triangles, groups=None):
    v, t, g = _check(vertices, triangles, groups)
    head = ["ply", "format binary_little_endian 1.0", "comment covidseg_amd mesh_min", f"element vertex {v.shape[0]}", "property float x", "property float y",
            "property float z", f"element face {t.shape[0]}", "property list uchar int vertex_indices"]
    fields = [("n", "u1"), ("idx", "<i4", (3,))]
    if g is not None:
        head.append("property int group")
        fields.append(("group", "<i4"))
    head.append("end_header")
    face = np.zeros(t.shape[0], np.dtype(fields))
    face["n"] = 3
    face["idx"] = t
    if g is not None:
        face["group"] = g
    return ("\n".join(head) + "\n").encode("ascii") + v.tobytes() + face.tobytes()


def write_ply(path, vertices, triangles, groups=None):
    data = ply_bytes(vertices, triangles, groups)
    with open(path, "wb") as f:
        f.write(data)


def read_ply(path):
    """the subset write_ply writes: binary_little_endian, float x y z vertices, triangular faces, an optional int group"""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").split("\n")
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian 1.0 is read")
    nv = nt = None
    props = {"vertex": [], "face": []}
    cur = None
    for ln in lines:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            if cur == "vertex":
                nv = int(w[2])
            elif cur == "face":
                nt = int(w[2])
            else:
                raise ValueError(f"{path}: element {cur!r} is not read")
        elif w[:1] == ["property"] and cur in props:
            props[cur].append(" ".join(w[1:]))
    if nv is None or nt is None or props["vertex"] != ["float x", "float y", "float z"] or props["face"][:1] != ["list uchar int vertex_indices"] \
            or props["face"][1:] not in ([], ["int group"]):
        raise ValueError(f"{path}: not the layout write_ply writes")
    has_group = len(props["face"]) == 2
    fields = [("n", "u1"), ("idx", "<i4", (3,))] + ([("group", "<i4")] if has_group else [])
    face_dt = np.dtype(fields)
    at = end + len(b"end_header\n")
    if len(data) != at + 12 * nv + face_dt.itemsize * nt:
        raise ValueError(f"{path}: {nv} vertices and {nt} faces need {at + 12 * nv + face_dt.itemsize * nt} bytes, the file has {len(data)}")
    v = np.frombuffer(data, "<f4", 3 * nv, at).reshape(nv, 3).astype(np.float32)
    face = np.frombuffer(data, face_dt, nt, at + 12 * nv)
    if nt and (face["n"] != 3).any():
        raise ValueError(f"{path}: a face is not a triangle")
    return v, face["idx"].astype(np.int32), (face["group"].astype(np.int32) if has_group else None)


def obj_text(vertices, triangles, groups=None):
    v, t, g = _check(vertices, triangles, groups)
    out = ["# covidseg_amd mesh_min"]
    out += ["v %.9g %.9g %.9g" % (float(p[0]), float(p[1]), float(p[2])) for p in v]
    last = None
    for k in range(t.shape[0]):
        if g is not None and int(g[k]) != last:
            last = int(g[k])
            out.append(f"g group_{last}")
        out.append("f %d %d %d" % (int(t[k, 0]) + 1, int(t[k, 1]) + 1, int(t[k, 2]) + 1))
    return "\n".join(out) + "\n"


def write_obj(path, vertices, triangles, groups=None):
    text = obj_text(vertices, triangles, groups)
    with open(path, "w", encoding="ascii", newline="\n") as f:
        f.write(text)


FORMATS = {".stl": "stl", ".ply": "ply", ".obj": "obj"}


def format_of(path):
    ext = os.path.splitext(os.fspath(path))[1].lower()
    if ext not in FORMATS:
        raise ValueError(f"a mesh file ends in {sorted(FORMATS)}, not {ext!r}")
    return FORMATS[ext]


def write(path, vertices, triangles, groups=None):
    fmt = format_of(path)
    if fmt == "stl":
        write_stl(path, vertices, triangles)
    elif fmt == "ply":
        write_ply(path, vertices, triangles, groups)
    else:
        write_obj(path, vertices, triangles, groups)
