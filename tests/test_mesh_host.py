"""CPU: tests/mesh_oracle.py (the numpy definition of csrc/kernels_mesh.hip) against its own rule, against topology and against closed forms; the
bit-level rules of the interpolation; mesh_min's files; the argument checks of volume.extract_surface / lesion_shapes / segment_volume(mesh=); the four entries in the
header and the bindings, and the kernel's constant table against the derivation."""
import os
import re
import struct

import numpy as np
import pytest

import mesh_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"unet_vol_mesh_count": 18, "unet_vol_mesh_emit": 23, "unet_vol_mesh_measure": 8}


# ---- the table ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_follows_the_rule_over_all_mixed_cases():
    table = MO.derive_table()
    assert len(table) == 6 and all(len(row) == 16 for row in table)
    mixed = 0
    for n in range(6):
        v = MO.tet_corners(n).astype(np.float64)
        assert np.array_equal(v[0], [0, 0, 0]) and np.array_equal(v[3], [1, 1, 1]) and all((v[k + 1] - v[k]).sum() >= 1 for k in range(3))
        assert abs(np.linalg.det(v[1:] - v[0])) == 1.0                                     # six tetrahedra of volume 1 / 6 fill the cube
        assert table[n][0] == [] and table[n][15] == []
        for case in range(1, 15):
            mixed += 1
            ins = [k for k in range(4) if (case >> k) & 1]
            out = [k for k in range(4) if not (case >> k) & 1]
            tris = table[n][case]
            assert len(tris) == (2 if len(ins) == 2 else 1)
            edges = {e for tri in tris for e in tri}
            assert edges == {(i, o) for i in ins for o in out}                          # every crossed edge, each with its inside corner first
            if len(ins) == 1:
                assert tris[0][0] == (ins[0], out[0])                                   # the first edge of a triangle is the rule's first: the winding swaps 2nd and 3rd only
            elif len(ins) == 3:
                assert tris[0][0] == (ins[0], out[0])
            else:
                assert tris[0][0] == tris[1][0] == (ins[0], out[0]) and {tris[0][1], tris[0][2]} == {(ins[0], out[1]), (ins[1], out[1])}
            for tri in tris:                                                            # every triangle's normal points from inside to outside
                m = [(v[i] + v[o]) * 0.5 for i, o in tri]
                nrm = np.cross(m[1] - m[0], m[2] - m[0])
                assert np.dot(nrm, v[out].mean(0) - v[ins].mean(0)) > 0
    assert mixed == 6 * 14


def test_the_kernel_holds_the_derived_table_and_the_design_prints_it():
    from covidseg_amd import _lib
    want = MO.packed_table()
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "kernels_mesh.hip")).read()
    m = re.search(r"MS_TABLE\[6\]\[16\]\s*=\s*\{(.*?)\};", src, flags=re.S)
    got = np.array([int(x) for x in re.findall(r"\d+", m.group(1))], np.uint32).reshape(6, 16)
    assert np.array_equal(got, want)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("4z."):]
    for n in range(6):
        assert " ".join(str(int(x)) for x in want[n]) in sec, f"DESIGN.md section 4z does not print row {n} of the table"
    # the packing itself: count in the low bits, 3-bit edge codes above
    t = MO.derive_table()
    for n in range(6):
        for case in range(16):
            w = int(want[n, case])
            assert (w & 15) == len(t[n][case])
            flat = [e for tri in t[n][case] for e in tri]
            assert [MO.PAIRS[(w >> (4 + 3 * j)) & 7] for j in range(len(flat))] == [(min(e), max(e)) for e in flat]


# ---- topology -------------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 4, 3), (9, 7, 5)])
def test_every_random_mask_gives_a_closed_consistently_wound_surface(shape):
    for seed in range(5):
        m = (np.random.default_rng(seed).random(shape) < 0.5).astype(np.uint8)
        r = MO.extract(mask=m)
        assert MO.is_closed_manifold(r.triangles), (shape, seed)
        assert r.counts.max() <= 12 and int(r.counts.sum()) == len(r.triangles) and int(np.unpackbits(r.flags).sum()) == len(r.vertices)
        assert set(np.unique(r.triangles)) == set(range(len(r.vertices)))               # every vertex is used
        _, vol = MO.measure(r.vertices, r.triangles)
        assert vol.sum() > 0


def test_the_256_corner_patterns():
    r = MO.extract(mask=MO.pattern_volume())
    assert r.vertices.shape == (11904, 3) and r.triangles.shape == (22656, 3)
    assert MO.is_closed_manifold(r.triangles) and r.counts.max() <= 12


def test_ball_and_torus_have_their_euler_characteristic():
    for rad in (3, 5, 8, 12):
        n = 2 * rad + 6
        r = MO.extract(values=MO.ball_field((n, n, n), (n / 2 - 0.3, n / 2 + 0.2, n / 2 - 0.1), rad), iso=0.0)
        assert MO.is_closed_manifold(r.triangles) and MO.euler(len(r.vertices), r.triangles) == 2
    r = MO.extract(values=MO.torus_field((24, 24, 12), (11.7, 12.2, 5.6), 6, 2.5), iso=0.0)
    assert MO.is_closed_manifold(r.triangles) and MO.euler(len(r.vertices), r.triangles) == 0


def test_an_open_mesh_has_boundary_edges_and_padding_closes_them():
    f = MO.ball_field((12, 12, 12), (2.2, 6.1, 5.8), 5.0)                             # the ball leaves the volume through x = 0
    opened = MO.extract(values=f, iso=0.0, closed=False)
    assert len(opened.triangles) and not MO.is_closed_manifold(opened.triangles)
    e = MO.directed_edges(opened.triangles)
    fwd = {(int(a), int(b)) for a, b in e}
    assert len(fwd) == len(e) and any((b, a) not in fwd for a, b in fwd)               # wound consistently, and some edges have no partner
    closed = MO.extract(values=f, iso=0.0, closed=True)
    assert MO.is_closed_manifold(closed.triangles) and MO.euler(len(closed.vertices), closed.triangles) == 2
    assert closed.vertices[:, 0].min() == -1.0                                          # the cap lies on the virtual layer: a padded point is at index -1
    m = (f > 0).astype(np.uint8)
    assert not MO.is_closed_manifold(MO.extract(mask=m, closed=False).triangles) and MO.is_closed_manifold(MO.extract(mask=m, closed=True).triangles)
    assert MO.extract(mask=m, closed=True).vertices[:, 0].min() == -0.5


def test_an_unpadded_volume_with_an_extent_of_one_has_no_cells():
    r = MO.extract(mask=np.ones((5, 1, 3), np.uint8), closed=False)
    assert len(r.vertices) == 0 and len(r.triangles) == 0 and not r.flags.any()
    r = MO.extract(mask=np.ones((1, 1, 1), np.uint8), closed=True)
    assert MO.is_closed_manifold(r.triangles) and MO.euler(len(r.vertices), r.triangles) == 2


# ---- sphere bounds: twice the deviation the oracle measures (area -0.40 % / volume -0.78 % at r = 8, -2.9 % / -5.5 % at r = 3, binary ratio 1.27) ----
def _ball(rad, binary):
    n = 2 * rad + 6
    f = MO.ball_field((n, n, n), (n / 2 - 0.3, n / 2 + 0.2, n / 2 - 0.1), rad)
    r = MO.extract(mask=(f > 0).astype(np.uint8)) if binary else MO.extract(values=f, iso=0.0)
    a, v = MO.measure(r.vertices, r.triangles)
    return a.sum() / (4 * np.pi * rad ** 2), v.sum() / (4 / 3 * np.pi * rad ** 3)


def test_a_smooth_ball_meets_the_analytic_area_and_volume():
    a, v = _ball(8, False)
    print(f"smooth r = 8: area {100 * (a - 1):+.3f} % volume {100 * (v - 1):+.3f} %")
    assert abs(a - 1) <= 0.008 and abs(v - 1) <= 0.016
    a, v = _ball(3, False)
    print(f"smooth r = 3: area {100 * (a - 1):+.3f} % volume {100 * (v - 1):+.3f} %")
    assert abs(a - 1) <= 0.06 and abs(v - 1) <= 0.11


def test_a_binary_ball_is_a_staircase():
    a, v = _ball(8, True)
    print(f"binary r = 8: area ratio {a:.4f} volume {100 * (v - 1):+.3f} %")
    assert 1.20 <= a <= 1.35
    sph, _ = MO.shape_fields(a * 4 * np.pi * 64, v * 4 / 3 * np.pi * 512)
    assert 0.75 < float(sph) < 0.83                                                    # about 0.79, not 1


# ---- geometry -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _oblique():
    c, s = np.cos(0.3), np.sin(0.3)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.2), -np.sin(0.2)], [0, np.sin(0.2), np.cos(0.2)]])
    return np.hstack([R * np.array([0.7, 0.8, 2.5]), [[-31.5], [12.25], [100.0]]])


def test_the_matrix_moves_the_vertices():
    f = MO.ball_field((14, 13, 12), (6.7, 6.2, 5.9), 4.0)
    base = MO.extract(values=f, iso=0.0)
    for M in (MO.default_matrix((0.7, 0.8, 2.5)), _oblique()):
        r = MO.extract(values=f, iso=0.0, matrix=M)
        assert np.array_equal(r.triangles, base.triangles)
        want = base.vertices.astype(np.float64) @ M[:, :3].T + M[:, 3]
        assert np.abs(r.vertices - want).max() <= 2e-5 * np.abs(want).max()          # float32 storage of both
        _, v = MO.measure(r.vertices, r.triangles)
        _, v0 = MO.measure(base.vertices, base.triangles)
        assert v.sum() > 0 and abs(v.sum() / (v0.sum() * 0.7 * 0.8 * 2.5) - 1) < 1e-4


def test_the_signed_volume_is_positive_and_ignores_the_translation():
    f = MO.ball_field((14, 13, 12), (6.7, 6.2, 5.9), 4.0)
    r = MO.extract(values=f, iso=0.0)
    v64 = r.vertices.astype(np.float64)
    tr = r.triangles.astype(np.int64)

    def vol(shift):                                                                   # the same formula on translated float64 vertices (float32 storage would round the shift in)
        a, b, c = (v64[tr[:, k]] + shift for k in range(3))
        return (np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0).sum()
    v0 = vol(np.zeros(3))
    assert v0 > 0 and abs(MO.measure(r.vertices, r.triangles)[1].sum() / v0 - 1) < 1e-12
    for shift in ([100.0, -50.0, 25.0], [-3.5, 0.25, 1e3]):
        assert abs(vol(np.array(shift)) / v0 - 1) <= 1e-9


# ---- bit-level rules ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_sample_equal_to_iso_is_outside_and_gives_t_zero():
    v = np.zeros((3, 3, 3))
    v[1, 1, 1] = 2.0                                                                  # the neighbours equal iso = 0: outside, and every vertex lies ON them
    r = MO.extract(values=v, iso=0.0, closed=False)
    assert len(r.vertices) == 14 and MO.is_closed_manifold(r.triangles)
    assert set(map(tuple, r.vertices.tolist())) == {tuple(float(1 + s * d) for d in dd) for dd in MO.DIRS for s in (-1, 1)}          # t = 0 at a lower end, t = 1 at an upper end
    a, _ = MO.measure(r.vertices, r.triangles)
    assert (a > 0).all()
    v[0, 1, 1] = 0.0; v[1, 1, 1] = 0.0; v[2, 1, 1] = 1.0                           # an inside sample whose lower neighbours equal iso: t = fl(0 / 1) = 0
    r = MO.extract(values=v, iso=0.0, closed=False)
    assert [2.0, 1.0, 1.0] not in r.vertices.tolist() and [1.0, 1.0, 1.0] in r.vertices.tolist()


def test_zero_area_triangles_are_kept():
    v = np.full((4, 4, 4), -1.0)
    v[1, 1, 1] = 0.0; v[2, 1, 1] = 1.0                                               # (1,1,1) equals iso: outside, and the edges from it to (2,1,1) collapse onto it
    v[2, 2, 1] = 1.0                                                                 # a second inside corner of the same tetrahedron: two of its vertices land on (1,1,1)
    r = MO.extract(values=v, iso=0.0)
    a, _ = MO.measure(r.vertices, r.triangles)
    assert MO.is_closed_manifold(r.triangles) and MO.euler(len(r.vertices), r.triangles) == 2
    assert len(np.unique(r.vertices, axis=0)) < len(r.vertices)                     # distinct vertex ids at one place
    assert (a == 0).any() and (a > 0).any()


def test_a_non_finite_endpoint_gives_t_one_half():
    for bad in (np.nan, np.inf, -np.inf):
        v = np.full((3, 3, 3), -1.0)
        v[1, 1, 1] = 3.0
        v[2, 1, 1] = bad
        r = MO.extract(values=v, iso=0.0, closed=False)
        verts = set(map(tuple, r.vertices.tolist()))
        if bad == np.inf:                                                             # +inf is inside: the edge between the two inside samples is not crossed
            assert (1.5, 1.0, 1.0) not in verts and (2.0, 1.5, 1.0) in verts          # (2,1,1) -> (2,2,1): a non-finite end, t = 0.5
        else:                                                                         # NaN and -inf are outside
            assert (1.5, 1.0, 1.0) in verts
        assert (1.0, 1.75, 1.0) in verts                                              # a finite edge: t = (0 - 3) / (-1 - 3)


def test_labels_select_and_groups():
    lab = np.zeros((6, 5, 4), np.int32)
    lab[1:3, 1:3, 1:3] = 1
    lab[3:5, 3, 1:3] = 2                                                              # touches label 1 along the face diagonal (1, 1, 0)
    both = MO.extract(labels=lab, select=0)
    one = MO.extract(labels=lab, select=1)
    two = MO.extract(labels=lab, select=2)
    assert set(np.unique(both.groups)) == {1, 2} and set(np.unique(one.groups)) == {1} and set(np.unique(two.groups)) == {2}
    assert MO.is_closed_manifold(both.triangles) and MO.euler(len(both.vertices), both.triangles) == 2          # one surface: the two share it
    assert MO.euler(len(one.vertices), one.triangles) == 2 and MO.euler(len(two.vertices), two.triangles) == 2
    same = MO.extract(mask=(lab != 0).astype(np.uint8))
    assert np.array_equal(same.triangles, both.triangles) and MO.same_bits(same.vertices, both.vertices)
    a, v = MO.measure(both.vertices, both.triangles)
    gv = MO.group_sums(v, both.groups, [1, 2])
    assert (gv > 0).all() and abs(gv.sum() - v.sum()) < 1e-9


# ---- mesh_min -------------------------------------------------------------------------------------------------------------------------------------------------------------
def _small_mesh():
    lab = np.zeros((5, 4, 4), np.int32)
    lab[1:3, 1:3, 1:3] = 1
    lab[3, 1, 1] = 7
    return MO.extract(labels=lab, matrix=_oblique())


def test_stl_bytes_and_round_trip(tmp_path):
    from covidseg_amd import mesh_min as MM
    r = _small_mesh()
    p = tmp_path / "m.stl"
    MM.write_stl(p, r.vertices, r.triangles)
    data = open(p, "rb").read()
    nt = len(r.triangles)
    assert len(data) == 80 + 4 + 50 * nt and struct.unpack_from("<I", data, 80)[0] == nt and not data.startswith(b"solid")
    first = struct.unpack_from("<12fH", data, 84)
    assert first[12] == 0 and np.array_equal(np.array(first[3:12], np.float32).reshape(3, 3), r.vertices[r.triangles[0]])
    corners, normals = MM.read_stl(p)
    assert MO.same_bits(corners, r.vertices[r.triangles])
    a, b, c = (r.vertices[r.triangles[:, k]].astype(np.float64) for k in range(3))
    n64 = np.cross(b - a, c - a)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    assert np.abs(normals - n64).max() < 1e-5 and np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1).max() < 1e-6
    MM.write_stl(p, np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32))                          # a degenerate facet: normal (0, 0, 0)
    assert not MM.read_stl(p)[1].any()
    with pytest.raises(ValueError):
        MM.write_stl(p, r.vertices, r.triangles, header=b"solid x")


def test_ply_bytes_group_property_and_round_trip(tmp_path):
    from covidseg_amd import mesh_min as MM
    r = _small_mesh()
    p = tmp_path / "m.ply"
    MM.write_ply(p, r.vertices, r.triangles, r.groups)
    data = open(p, "rb").read()
    head, body = data[:data.index(b"end_header\n") + 11], data[data.index(b"end_header\n") + 11:]
    lines = head.decode().split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and f"element vertex {len(r.vertices)}" in lines and f"element face {len(r.triangles)}" in lines
    assert "property list uchar int vertex_indices" in lines and "property int group" in lines
    assert len(body) == 12 * len(r.vertices) + 17 * len(r.triangles)
    assert struct.unpack_from("<B3ii", body, 12 * len(r.vertices)) == (3,) + tuple(int(v) for v in r.triangles[0]) + (int(r.groups[0]),)
    v, t, g = MM.read_ply(p)
    assert MO.same_bits(v, r.vertices) and np.array_equal(t, r.triangles) and np.array_equal(g, r.groups) and set(np.unique(g)) == {1, 7}
    MM.write_ply(p, r.vertices, r.triangles)
    data = open(p, "rb").read()
    assert b"property int group" not in data and len(data) - data.index(b"end_header\n") - 11 == 12 * len(r.vertices) + 13 * len(r.triangles)
    v, t, g = MM.read_ply(p)
    assert g is None and np.array_equal(t, r.triangles)


def test_obj_text_and_the_suffix_dispatch(tmp_path):
    from covidseg_amd import mesh_min as MM
    r = _small_mesh()
    MM.write(tmp_path / "m.obj", r.vertices, r.triangles, r.groups)
    lines = open(tmp_path / "m.obj").read().split("\n")
    vs = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")], np.float32)
    fs = np.array([[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("f ")], np.int32)
    assert MO.same_bits(vs, r.vertices) and np.array_equal(fs - 1, r.triangles)
    assert {ln for ln in lines if ln.startswith("g ")} == {"g group_1", "g group_7"}
    MM.write(tmp_path / "m.STL", r.vertices, r.triangles, r.groups)
    assert len(MM.read_stl(tmp_path / "m.STL")[0]) == len(r.triangles)
    with pytest.raises(ValueError):
        MM.write(tmp_path / "m.vtk", r.vertices, r.triangles)
    with pytest.raises(ValueError):
        MM.write_ply(tmp_path / "bad.ply", r.vertices, r.triangles + len(r.vertices))
    with pytest.raises(ValueError):
        MM.write_ply(tmp_path / "bad.ply", r.vertices, r.triangles, r.groups[:-1])


def test_an_empty_mesh_round_trips(tmp_path):
    from covidseg_amd import mesh_min as MM
    v, t = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    MM.write_stl(tmp_path / "e.stl", v, t)
    assert os.path.getsize(tmp_path / "e.stl") == 84 and MM.read_stl(tmp_path / "e.stl")[0].shape == (0, 3, 3)
    MM.write_ply(tmp_path / "e.ply", v, t, np.zeros(0, np.int32))
    rv, rt, rg = MM.read_ply(tmp_path / "e.ply")
    assert rv.shape == (0, 3) and rt.shape == (0, 3) and rg.shape == (0,)
    MM.write_obj(tmp_path / "e.obj", v, t)
    assert open(tmp_path / "e.obj").read().startswith("#")


# ---- argument checks: all before any device work (this machine has no GPU) ---------------------------------------------------------------------------------------------------
def test_extract_surface_refuses_bad_arguments_before_any_device_work():
    from covidseg_amd import volume as V
    m = np.zeros((4, 4, 4), np.uint8)
    f = np.zeros((4, 4, 4), np.float32)
    lab = np.zeros((4, 4, 4), np.int32)
    bad = [
        (f, {}),                                                                      # a scalar volume needs iso
        (m.astype(bool), dict(iso=0.5)),                                              # a mask has none
        (m.astype(bool), dict(select=1)), (m.astype(bool), dict(groups=True)),
        (f, dict(iso=np.nan)), (f, dict(iso=np.inf)), (f, dict(iso="x")),
        (f, dict(iso=0.0, pad_value=1.0)), (f, dict(iso=0.0, pad_value=np.nan)), (f, dict(iso=0.0, pad_value=-np.inf)),
        (f, dict(iso=0.0, select=2)), (f, dict(iso=0.0, groups=True)),
        (m, dict(pad_value=0.0)),
        (lab, dict(select=-1)), (lab, dict(select=1.5)), (lab, dict(select=True)), (lab, dict(select=2 ** 31)),
        (m, dict(closed=1)), (lab, dict(groups=1)),
        (m, dict(pixdim=(1, 1, 1), affine=np.eye(4))), (m, dict(pixdim=(1, 0, 1))), (m, dict(affine=np.zeros((4, 4)))),
        (m, dict(shape=(4, 4, 4))),                                                   # shape= describes a device tensor
        (np.zeros((4, 4), np.uint8), {}),
    ]
    for x, kw in bad:
        with pytest.raises(ValueError):
            V.extract_surface(x, **kw)
    assert V._mesh_kind(m, None, 0, False) == "mask" and V._mesh_kind(m, None, 3, False) == "labels" and V._mesh_kind(lab, None, 0, False) == "labels"
    assert V._mesh_kind(m, 0.5, 0, False) == "scalar" and V._mesh_kind(np.zeros((2, 2, 2), np.int16), -300.0, 0, False) == "scalar" and V._mesh_kind("ct.nii", None, 0, True) == "labels"
    assert V._check_mesh_args("scalar", 0.25, 0, True, None, False) == (0.25, 0, 0.25) and V._check_mesh_args("mask", None, 0, True, None, False) == (0.5, 0, 0.0)
    with pytest.raises(ValueError):
        V._check_mesh_lattice((2047, 1023, 1023), True)
    V._check_mesh_lattice((1290, 1290, 1290), False)


def test_lesion_shapes_and_mesh_option_refuse_bad_arguments():
    from covidseg_amd import volume as V
    lab = np.zeros((4, 4, 4), np.int32)
    for n in (-1, 1.5, True, None):
        with pytest.raises(ValueError):
            V.lesion_shapes(lab, n)
    with pytest.raises(ValueError):
        V.lesion_shapes(lab.astype(np.float32), 1)
    with pytest.raises(ValueError):
        V.lesion_shapes(np.zeros((4, 4), np.int32), 1)
    for mesh in ("yes", 3, {"what": "heart"}, {"colour": 1}, {"what": "lung"}, {"what": "both"}, {"lesions": 1}, {"out_path": "m.vtk"}):
        with pytest.raises(ValueError):
            V._check_mesh(mesh, None)
    assert V._check_mesh(None, None) is None and V._check_mesh(False, None) is None
    assert V._check_mesh(True, None) == {"what": "infection", "out_path": None, "lesions": False}
    assert V._check_mesh({"what": "both", "out_path": "a/b.ply", "lesions": True}, "lung.nii")["what"] == "both" and V._lung_mesh_path("a/b.ply") == "a/b_lung.ply"
    ct = np.zeros((8, 8, 4), np.int16)
    for fn, args in ((V.segment_volume, (ct, None)), (V.segment_volume_ensemble, (ct, [None]))):
        with pytest.raises(ValueError, match="mesh"):
            fn(*args, mesh={"what": "lung"})                                          # no lung mask: before any device work, before the model is looked at
    import covidseg_amd
    for name in ("extract_surface", "lesion_shapes", "SurfaceMesh"):
        assert getattr(covidseg_amd, name) is getattr(V, name) and name in covidseg_amd.__all__
    assert "mesh_min" in covidseg_amd.__all__
    sph, s2v = V.shape_descriptors([4 * np.pi * 9.0, 0.0, 1.0], [4 / 3 * np.pi * 27.0, 1.0, -1.0])
    assert abs(sph[0] - 1) < 1e-12 and abs(s2v[0] - 1.0) < 1e-12 and np.isnan(sph[1:]).all() and np.isnan(s2v[2])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_entries_are_declared_bound_and_exported():
    import ctypes
    from covidseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name, argc in ENTRIES.items():
        m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code)
        assert m and m.group(1).count(",") + 1 == argc, name
        restype, args = _lib._PROTOS[name]
        assert restype is ctypes.c_int32 and len(args) == argc and args[0] is ctypes.c_void_p and args[-1] is ctypes.c_void_p
    m = re.search(r"\bsize_t\s+unet_vol_mesh_ws_bytes\s*\(([^;{]*?)\)\s*;", code)
    assert m and m.group(1).count(",") + 1 == 4 and _lib._PROTOS["unet_vol_mesh_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int32] * 4)
    lib = _lib.load()
    for name in ENTRIES:
        assert getattr(lib, name).argtypes is not None
    # the workspace: two bytes per lattice point (padded to 16) and two offset arrays of one int32 per 2048-point chunk, plus one; nothing for a volume without cells
    assert lib.unet_vol_mesh_ws_bytes(0, 5, 5, 1) == 0 and lib.unet_vol_mesh_ws_bytes(5, 1, 5, 0) == 0 and lib.unet_vol_mesh_ws_bytes(-1, 5, 5, 1) == 0
    assert lib.unet_vol_mesh_ws_bytes(1, 1, 1, 1) == 2 * 32 + 2 * 16
    npts = 133 * 35 * 19
    assert lib.unet_vol_mesh_ws_bytes(131, 33, 17, 1) == 2 * ((npts + 15) // 16 * 16) + 2 * ((((npts + 2047) // 2048 + 1) * 4 + 15) // 16 * 16)
    assert lib.unet_vol_mesh_ws_bytes(2047, 1023, 1023, 1) == 0 and lib.unet_vol_mesh_ws_bytes(1290, 1290, 1290, 0) > 0
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert src.count("kernels_mesh") >= 6                            # SRCS, the comment, the -ffp-contract=off list in its three places, the header dependency
    for line in src.split("\n"):
        if "EXTRA = -ffp-contract=off" in line:
            assert "kernels_mesh.o" in line
