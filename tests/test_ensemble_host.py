"""CPU: tests/ensemble_oracle.py checked against itself, every argument error of volume.vote_volume / segment_volume_ensemble raised without a GPU, the vote
rules, and the new entry points' presence in include/unet_hip.h and _lib."""
import os
import re

import numpy as np
import pytest

import ensemble_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("unet_vol_dihedral", "unet_vol_canvas_axpy", "unet_vol_canvas_div", "unet_vol_unslice_prob", "unet_vol_vote_pack", "unet_vol_vote_reduce")


def _asym(n=2, d=5):
    return np.arange(n * d * d, dtype=np.float32).reshape(n, d, d) ** 1.5


def test_every_symmetry_composed_with_its_inverse_is_the_identity():
    from covidseg_amd import volume as V
    a = _asym()
    assert V.TTA == EO.TTA
    for code, name in enumerate(EO.TTA):
        assert np.array_equal(EO.dihedral(EO.dihedral(a, name), EO.INVERSE[name]), a), name
        assert V.TTA[V.DIHEDRAL_INVERSE[code]] == EO.INVERSE[name]                          # the product's table is the oracle's
        assert np.array_equal(EO.dihedral(a, code), EO.dihedral(a, name))
        assert np.array_equal(EO.dihedral(a[..., None], name)[..., 0], EO.dihedral(a, name))


def test_the_eight_symmetries_are_distinct_and_mean_what_numpy_means():
    a = _asym()
    got = [EO.dihedral(a, name) for name in EO.TTA]
    for i in range(8):
        for j in range(i + 1, 8):
            assert not np.array_equal(got[i], got[j]), (EO.TTA[i], EO.TTA[j])
    m = a[0]
    assert np.array_equal(got[1][0], np.rot90(m)) and np.array_equal(got[4][0], m[:, ::-1]) and np.array_equal(got[5][0], m[::-1]) and np.array_equal(got[6][0], m.T)
    assert np.array_equal(got[7][0], np.rot90(m.T, 2)) and got[1][0][0, 0] == m[0, -1] and got[3][0][0, 0] == m[-1, 0]


def _members(shape, M, seed):
    rng = np.random.default_rng(seed)
    ms = [(rng.random(shape) < rng.uniform(0.05, 0.7)).astype(np.uint8) for _ in range(M)]
    if M >= 3:
        ms[1] = np.zeros(shape, np.uint8); ms[2] = np.ones(shape, np.uint8)
    if M >= 5:
        ms[4] = ms[3].copy()
    return ms


@pytest.mark.parametrize("M", [1, 2, 3, 7, 32])
def test_reduce_invariants(M):
    shape = (9, 7, 4)
    ms = _members(shape, M, M)
    words = EO.pack(ms)
    r = {rule: EO.reduce(words, M, EO.min_votes(rule, M)) for rule in ("any", "majority", "all")}
    a = r["majority"]
    assert np.array_equal(a["pair"], a["pair"].T) and np.array_equal(np.diag(a["pair"]), a["member_voxels"])
    assert np.array_equal(a["member_voxels"], [int(m.sum()) for m in ms])
    assert a["hist"].sum() == np.prod(shape) and a["hist"].shape == (M + 1,)
    assert np.array_equal(a["votes"], np.sum(ms, axis=0).astype(np.uint8))
    assert (r["any"]["mask"] >= r["majority"]["mask"]).all() and (r["majority"]["mask"] >= r["all"]["mask"]).all()          # any >= majority >= all
    assert np.array_equal(r["any"]["mask"], np.any(ms, axis=0)) and np.array_equal(r["all"]["mask"], np.all(ms, axis=0))
    assert np.array_equal(a["counts"], a["mask"].sum(axis=(0, 1)))
    d = EO.pairwise_dice(a["pair"])
    for i in range(M):
        for j in range(M):
            den = int(ms[i].sum()) + int(ms[j].sum())
            want = 2.0 * int((ms[i] & ms[j]).sum()) / den if den else np.nan
            assert d[i, j] == want or (np.isnan(d[i, j]) and np.isnan(want))


def test_weighted_mean_is_sequential_float32():
    rng = np.random.default_rng(0)
    cs = [rng.random(1000).astype(np.float32) for _ in range(3)]
    mean, wsum = EO.weighted_mean(cs, (0.3, 0.3, 0.4))
    F = np.float32
    want = np.empty(1000, F)
    for i in range(1000):                                           # scalar by scalar
        acc = F(F(0.3) * cs[0][i]); acc = F(acc + F(F(0.3) * cs[1][i])); acc = F(acc + F(F(0.4) * cs[2][i]))
        want[i] = F(acc / F(F(F(0.3) + F(0.3)) + F(0.4)))
    assert np.array_equal(mean, want) and wsum == F(F(F(0.3) + F(0.3)) + F(0.4))
    one, w1 = EO.weighted_mean([cs[0]], (1.0,))
    assert np.array_equal(one, cs[0]) and w1 == 1.0                 # 1 p and p / 1 are exact


@pytest.mark.parametrize("M", [1, 2, 3, 4, 32])
def test_min_votes_of_every_rule(M):
    from covidseg_amd import volume as V
    assert V.min_votes_of("majority", M) == M // 2 + 1 == EO.min_votes("majority", M)
    assert V.min_votes_of("any", M) == 1 and V.min_votes_of("all", M) == M
    for k in range(1, M + 1):
        assert V.min_votes_of(k, M) == k
    assert 2 * V.min_votes_of("majority", M) > M                     # strict: a tie is background
    for bad in (0, M + 1, -1, 1.5, True, "most", None):
        with pytest.raises(ValueError):
            V.min_votes_of(bad, M)


class _Stub:
    def __init__(self, h=8):
        self.h = h

    def predict(self, x, batch_size=32):
        raise AssertionError("an argument error must be raised before anything is predicted")


def test_vote_volume_refusals_need_no_gpu():
    from covidseg_amd import volume as V
    m = np.ones((4, 3, 2), np.uint8)
    bad = [lambda: V.vote_volume([m] * 33), lambda: V.vote_volume([]), lambda: V.vote_volume([m, np.ones((4, 3, 3), np.uint8)]), lambda: V.vote_volume([m, m], rule=3),
           lambda: V.vote_volume([m, m], rule=0), lambda: V.vote_volume([m, m], rule="most"), lambda: V.vote_volume([m, m[0]]), lambda: V.vote_volume([m, m * 0.5]),
           lambda: V.vote_volume(7), lambda: V.vote_volume([m], rule=1.0)]
    for f in bad:
        with pytest.raises(ValueError):
            f()


def test_segment_volume_ensemble_refusals_need_no_gpu():
    from covidseg_amd import volume as V
    ct = np.zeros((8, 8, 5), np.int16)
    s = _Stub()
    bad = [lambda: V.segment_volume_ensemble(ct, [s] * 33),                                                   # 33 members
           lambda: V.segment_volume_ensemble(ct, [s] * 5, tta=V.TTA[:7]),                                     # 35 members
           lambda: V.segment_volume_ensemble(ct, []),
           lambda: V.segment_volume_ensemble(ct, [s], tta=("id", "flip")),                                    # unknown name
           lambda: V.segment_volume_ensemble(ct, [s], tta=("id", "hflip", "id")),                             # repeated name
           lambda: V.segment_volume_ensemble(ct, [s], tta=()),
           lambda: V.segment_volume_ensemble(ct, [s, s], combine=5),                                          # rule out of range
           lambda: V.segment_volume_ensemble(ct, [s, s], combine=0),
           lambda: V.segment_volume_ensemble(ct, [s, s], combine="median"),
           lambda: V.segment_volume_ensemble(ct, [s, s], weights=(1.0,)),                                     # wrong length
           lambda: V.segment_volume_ensemble(ct, [s, s], weights=(1.0, 2.0, 3.0)),
           lambda: V.segment_volume_ensemble(ct, [s, s], weights=(1.0, float("nan"))),
           lambda: V.segment_volume_ensemble(ct, [s, s], weights=(0.0, 0.0)),
           lambda: V.segment_volume_ensemble(ct, [s, s], weights=(1.0, -1.0)),
           lambda: V.segment_volume_ensemble(ct, [s, _Stub(16)]),                                             # different input sizes
           lambda: V.segment_volume_ensemble(ct, [s], connectivity=4),
           lambda: V.dihedral(np.zeros((2, 3, 3), np.float32), "flip"), lambda: V.dihedral(np.zeros((2, 3, 3), np.float32), 8),
           lambda: V.dihedral(np.zeros((2, 3, 4), np.float32), "id"), lambda: V.dihedral(np.zeros((2, 3, 3), np.float64), "id"),
           lambda: V.models_from_weights([], 64), lambda: V.models_from_weights(["fold1.txt"], 64), lambda: V.models_from_weights(["/nonexistent/fold1.hdf5"], 64)]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
    members = V._check_ensemble([s, s], ("id", "hflip", "rot90"), "mean", (0.3, 0.7))
    assert members[1] == [(0, "id"), (0, "hflip"), (0, "rot90"), (1, "id"), (1, "hflip"), (1, "rot90")]          # model-major
    F = np.float32
    assert members[3] == F(F(F(F(F(F(0.3) + F(0.3)) + F(0.3)) + F(0.7)) + F(0.7)) + F(0.7)) and members[4] is None
    assert V._check_ensemble([s] * 4, V.TTA, "majority", None)[4] == 17                                     # 32 members are accepted


def test_the_new_symbols_are_declared_and_bound():
    from covidseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "unet_hip.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for name in SYMBOLS:
        m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code)
        assert m, f"{name} is not declared in include/unet_hip.h"
        assert name in _lib._PROTOS and len(_lib._PROTOS[name][1]) == m.group(1).count(",") + 1
        assert m.group(1).strip().endswith("void* stream")
    assert "section 4s" in hdr
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
