"""CPU: the host-side helpers that every volume kernel file takes from csrc/vol_common.h -- the two extents predicates, the NIfTI datatype table, the bounded-grid size,
the 16-byte padding, the overlap and alignment tests -- run on the CPU by tools/vol_common_host_check.hip and held to a restatement in Python integers, which cannot
overflow.  The per-family test_gpu_*.py files probe the same refusals through the entry points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "one-stop-for-covid-19-infection-and-lung-segmentation-plus-classification_amd", "csrc")
LIMIT = 1 << 31
M = LIMIT - 1

# (X, Y, Z) -> (strict, lenient): the triples the predicates are pinned on, whatever else the program prints
PINNED = {
    (-1, 3, 2): (0, 0),
    (0, 0, 0): (1, 1),
    (5, 3, 0): (1, 1),
    (2047, 1024, 1024): (1, 1),
    (2048, 2048, 512): (0, 0),                                         # exactly 2^31 voxels
    (46340, 46340, 1): (1, 1),
    (46341, 46341, 1): (0, 0),
    (65536, 65536, 0): (0, 1),                                         # no voxels, but a slice of 2^32: only the lenient form takes it
    (M, M, 0): (0, 1),
    (0, M, M): (1, 1),
    (M, M, M): (0, 0),                                                 # X Y Z = 2^93: past a 64-bit product
}


def dims_strict(X, Y, Z):
    return int(min(X, Y, Z) >= 0 and X * Y < LIMIT and X * Y * Z < LIMIT)


def dims_lenient(X, Y, Z):
    return int(min(X, Y, Z) >= 0 and (X * Y * Z == 0 or dims_strict(X, Y, Z) == 1))


def dims_before(X, Y, Z):
    """the body ten files used to hold, where it was defined: no signed 64-bit product overflows"""
    assert abs(X * Y * Z) < 1 << 63
    return int(min(X, Y, Z) >= 0 and X * Y * Z < LIMIT and (X == 0 or Y == 0 or X * Y < LIMIT))


def itemsize(dt):
    return {2: 1, 256: 1, 4: 2, 512: 2, 8: 4, 768: 4, 16: 4, 64: 8}.get(dt, 0)


def blocks(items, cap, tpb):
    q = items + tpb - 1
    b = abs(q) // tpb * (1 if q >= 0 else -1)                         # C++ division truncates towards zero
    return max(1, min(cap, b))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vol_common")
    exe = str(tmp / "vol_common_host_check")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I", CSRC,
                    os.path.join(ROOT, "tools", "vol_common_host_check.hip"), "-o", exe], check=True, cwd=str(tmp))
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in out.splitlines()]
    assert rows and all(len(r) >= 3 for r in rows)
    return [(r[0], tuple(int(v) for v in r[1:-1]), int(r[-1])) if r[0] != "dims" else (r[0], tuple(int(v) for v in r[1:4]), (int(r[4]), int(r[5]))) for r in rows]


def _of(lines, name):
    got = [(args, res) for n, args, res in lines if n == name]
    assert got, name
    return got


def test_both_extents_predicates_equal_their_restatement_and_the_pinned_triples(lines):
    got = dict(_of(lines, "dims"))
    for t, want in PINNED.items():
        assert got[t] == want, t
    for t, res in got.items():
        assert res == (dims_strict(*t), dims_lenient(*t)), t
    assert {s for s, _ in got.values()} == {0, 1} and any(s != l for s, l in got.values())


def test_the_strict_predicate_answers_as_the_former_body_did_wherever_that_was_defined(lines):
    defined = [t for t, _ in _of(lines, "dims") if abs(t[0] * t[1] * t[2]) < 1 << 63]
    assert len(defined) >= 20 and (65536, 65536, 0) in defined and (0, M, M) in defined
    for t in defined:
        assert dims_strict(*t) == dims_before(*t), t
    assert dims_strict(M, M, M) == 0                                  # where it overflowed, the shared form refuses


def test_the_datatype_table(lines):
    got = dict(_of(lines, "itemsize"))
    assert {dt for (dt,), n in got.items() if n} == {2, 256, 4, 512, 8, 768, 16, 64}
    for (dt,), n in got.items():
        assert n == itemsize(dt), dt


def test_the_bounded_grid_size(lines):
    got = _of(lines, "blocks")
    assert any(res == cap for (items, cap, tpb), res in got) and any(1 < res < cap for (items, cap, tpb), res in got) and any(items <= 0 for (items, cap, tpb), res in got)
    assert len({tpb for (items, cap, tpb), res in got}) >= 3
    for (items, cap, tpb), res in got:
        assert res == blocks(items, cap, tpb), (items, cap, tpb)


def test_padding_overlap_and_alignment(lines):
    for (b,), res in _of(lines, "pad16"):
        assert res == (b + 15) // 16 * 16 and res % 16 == 0 and 0 <= res - b < 16, b
    laps = _of(lines, "overlap")
    assert {res for _, res in laps} == {0, 1}
    for (a, na, b, nb), res in laps:
        assert res == int(a < b + nb and b < a + na), (a, na, b, nb)
    als = _of(lines, "aligned")
    assert {res for _, res in als} == {0, 1}
    for (p, a), res in als:
        assert res == int(p % a == 0), (p, a)
