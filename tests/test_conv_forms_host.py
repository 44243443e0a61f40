"""CPU: the cases of tests/conv_forms.py reach the launch forms they are named for -- on 256 compute units and on other CU counts --, are ragged in the way their
comments say, stay small enough for a float64 reference, and the dispatch text their transcriptions mirror is still the sources'."""
import os

import pytest

import bnfold_checks as B
import conv_forms as F

CUS = [256, 128, 192]
ALL_CASES = F.CASES + F.BITS_CASES + F.FOLD_FWD_EXTRA


@pytest.mark.parametrize("cu", CUS)
@pytest.mark.parametrize("case", ALL_CASES, ids=F.case_id)
def test_every_case_reaches_its_arm_at_its_batch_and_not_below(case, cu):
    arm, (M, h, w), _ = case
    n = F.case_batch(cu, case)
    assert B.h2_arm(cu, n, h, w, M) == arm
    assert n == 1 or B.h2_arm(cu, n - 1, h, w, M) != arm
    assert arm != B.ARMS[0] and F.K_SIDE % 16 == 0


def test_batches_at_256_compute_units_are_the_stated_ones():
    got = {c[1]: F.case_batch(256, c) for c in F.CASES}
    assert got == {(16, 125, 250): 2, (48, 125, 125): 2, (96, 61, 170): 2, (64, 125, 250): 1, (512, 29, 100): 1, (512, 125, 250): 1, (512, 120, 248): 1, (512, 61, 250): 2,
                   (512, 21, 250): 3, (512, 130, 120): 1, (64, 250, 250): 2}


@pytest.mark.parametrize("case", ALL_CASES, ids=F.case_id)
def test_every_case_is_ragged_as_its_comment_names(case):
    arm, (M, h, w), rag = case
    assert F.is_ragged_as_named(case)
    assert rag.get("cols") and w % 32 != 0                    # every case has a short last column tile
    if arm == B.ARMS[3]:
        assert "rows16" in rag and h <= 128                   # the 16-row instance: the case says how many rows its last tile holds
    else:
        assert h % 8 != 0
    assert sum(1 for c in F.CASES if c[2].get("half_block")) == 1


def test_the_16_row_cases_hold_a_tile_whose_second_half_is_empty_and_one_that_is_not():
    rows = sorted(h % 16 for arm, (M, h, w), _ in F.CASES if arm == B.ARMS[3])
    assert rows[0] == 8 and any(8 < r < 16 for r in rows)     # 8: rows 8-15 of the last tile lie outside the image; 13: they straddle its edge


def test_every_arm_but_the_small_grid_one_has_cases_in_every_mode_list():
    three = (B.ARMS[1], B.ARMS[3], B.ARMS[4])
    for cases, arms in ((F.CASES, B.ARMS[1:]), (F.BITS_CASES, B.ARMS[1:]), (F.GEN_CASES, three), (F.FOLD_CASES, three), (F.FOLD_FWD_CASES, three)):
        assert {c[0] for c in cases} >= set(arms)
    for arm, (M, h, w), _ in F.BITS_CASES:
        assert w % 8 == 0 and M % 32 == 0
    assert (B.ARMS[1], (96, 61, 170), F.CASES[2][2]) in F.FOLD_CASES
    for arm, (M, h, w), _ in F.FOLD_CASES:
        assert M % 32 == 0                                    # (a limit below cin needs 32-channel blocks; 256 % 16 == 0 for the cout = 16 side)
    for arm, (M, h, w), _ in F.FOLD_FWD_CASES:
        assert 256 % M == 0                                   # (what unet_conv3x3_bnfold_supported asks of cout)


def test_statistics_cases_are_ones_whose_launch_takes_the_request():
    """launch_h2 declines an armed statistics request where 2 c xw > UNET_BN_SLOT_DOUBLES (xw = UNET_XW in deterministic mode; both constants and the condition are
    pinned by DISPATCH_SOURCES): the deterministic cases stop at M = 256, and still reach every arm and both kinds of last 16-row tile"""
    assert (F.BN_SLOT_DOUBLES, F.XW) == (2048, 4)
    for arm, (M, h, w), _ in F.STATS_CASES:
        assert 2 * M * 1 <= F.BN_SLOT_DOUBLES and F.stats_epilogue_accepts(M, False)
    for arm, (M, h, w), _ in F.STATS_DET_CASES:
        assert 2 * M * 4 <= 2048 and F.stats_epilogue_accepts(M, True)
    assert not F.stats_epilogue_accepts(512, True) and F.stats_epilogue_accepts(256, True)
    assert {c[0] for c in F.STATS_DET_CASES} == set(B.ARMS[1:])
    assert {h % 16 for arm, (M, h, w), _ in F.STATS_DET_CASES if arm == B.ARMS[3]} >= {8, 13}
    assert any(c[2].get("half_block") for c in F.STATS_DET_CASES)
    assert all(c in F.STATS_DET_CASES or c[1][0] == 512 for c in F.STATS_CASES)


def test_cases_stay_small_enough_for_a_float64_reference():
    for case in ALL_CASES:
        arm, (M, h, w), _ = case
        n = F.case_batch(256, case)
        floats = n * h * w * M
        flop = 2 * 9 * F.K_SIDE * floats
        assert floats <= 17 * 2 ** 20 and flop <= 5e9, (case, floats, flop)


@pytest.mark.parametrize("shape", F.WGRAD_CASES)
def test_weight_gradient_cases_walk_two_units_per_workgroup(shape):
    p = F.plan_wgrad_h2(*shape)
    assert p["upb"] >= 2
    assert p["WA"] == 2 and p["WB"] == 2 and p["R"] == 2 and p["pairs"] == 64


def test_weight_gradient_plans_are_the_stated_ones():
    p = F.plan_wgrad_h2(*F.WGRAD_CASES[0])
    assert (p["units"], p["upb"], p["ublocks"]) == (17, 2, 9) and p["units"] % p["upb"] != 0 and F.WGRAD_CASES[0][1] % 2 == 1          # the last unit block is short; odd height
    q = F.plan_wgrad_h2(*F.WGRAD_CASES[1])
    assert (q["units"], q["upb"], q["ublocks"]) == (16, 2, 8) and q["units"] % q["upb"] == 0                                          # the even twin
    # why these cases exist: the headline step's c5b (512 -> 512 at 32 x 32, batch 16) and a 512 -> 256 layer at 64 x 64 walk two units, the full-size op-test shapes one
    assert F.plan_wgrad_h2(16, 32, 32, 512, 512)["upb"] == 2 and F.plan_wgrad_h2(16, 64, 64, 512, 256)["upb"] >= 2
    assert max(F.plan_wgrad_h2(*s)["upb"] for s in [(2, 512, 512, 32, 32), (2, 256, 256, 64, 64), (4, 32, 32, 256, 512), (16, 128, 128, 64, 64), (16, 32, 32, 128, 128)]) == 1


def test_pooled_sums_case_takes_the_16_row_branch():
    (n, h, w, cin, cout), rate = F.POOL_CASE
    assert F.pool_sums_form(n, h, w, cin) == F.POOL_FORMS[1]
    assert h % 2 == 0 and w % 2 == 0 and w % 32 != 0 and h % 16 != 0 and 0.0 < rate < 1.0
    assert B.cdiv(w, 32) * B.cdiv(h, 16) * n * B.cdiv(cin, 64) == 512
    # the shapes of the existing op test take the other two
    for s in [(2, 16, 32, 64, 32), (1, 24, 40, 128, 64), (2, 8, 8, 256, 128), (3, 16, 16, 64, 64)]:
        assert F.pool_sums_form(s[0], s[1], s[2], s[4]) in (F.POOL_FORMS[0], F.POOL_FORMS[2])


@pytest.mark.parametrize("cu", CUS)
def test_convT_case_takes_the_four_block_branch(cu):
    n, h, w, cin, cout = F.CONVT_CASE
    assert F.convT_fwd_form(cu, n, h, w, cout) == F.CONVT_FORMS[1] or cu > 256
    assert w % 32 != 0
    if cu == 256:
        assert B.cdiv(w, 32) * B.cdiv(h, 8) * n * B.cdiv(4 * cout, 128) == 256
        for s in [(10, 30, 64, 256, 128), (16, 48, 96, 128, 64)]:          # the shapes that reached the form before: whole column tiles
            assert F.convT_fwd_form(cu, s[0], s[1], s[2], s[4]) == F.CONVT_FORMS[1] and s[2] % 32 == 0


@pytest.mark.parametrize("file,text", F.DISPATCH_SOURCES, ids=[f"{f}:{i}" for i, (f, _) in enumerate(F.DISPATCH_SOURCES)])
def test_a_transcribed_condition_is_the_sources(file, text):
    from covidseg_amd import _lib
    src = F.normalised(F.strip_comments(open(os.path.join(os.path.dirname(_lib.__file__), "csrc", file)).read()))
    assert src.count(F.normalised(text)) == 1, f"{file}: the dispatch no longer reads `{text}`; tests/conv_forms.py (or bnfold_checks.h2_arm) mirrors it"
