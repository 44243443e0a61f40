"""The launch forms of the fp32 h2 conv kernels and the ragged shapes that reach each of them, shared by test_conv_forms_host.py (the arithmetic, on the CPU) and
test_gpu_conv_forms.py (the device at those shapes).  numpy only.

The conv3x3 dispatch itself is bnfold_checks.h2_arm (the end of k_conv3x3_h2_fwd, transcribed once); here are the three neighbouring choices -- plan_wgrad_h2, the
three-way choice of k_conv3x3_h2_dgrad_pool_sums and the two-way choice of k_convT_h2_fwd -- and the cases.  A case is (M, h, w): M output channels of the launch
(cout of a forward, cin of a data gradient), K = 16 channels on the contracted side; the batch is the smallest at which the launch takes the arm on the device's CU
count.  DISPATCH_SOURCES pins the source lines every transcription mirrors (test_conv_forms_host.py): a changed dispatch fails there instead of quietly turning a case
into a test of another instance."""
import re

from bnfold_checks import ARMS, cdiv, h2_arm

K_SIDE = 16                      # channels on the contracted side of every case

# arm -> template arguments of conv_h2_kernel that matter to a check: rows of a workgroup's tile (4 waves x RW rows), 32-channel blocks per workgroup
TILE_ROWS = {ARMS[0]: 4, ARMS[1]: 8, ARMS[2]: 8, ARMS[3]: 16, ARMS[4]: 8}
BLOCKS = {ARMS[0]: 1, ARMS[1]: 1, ARMS[2]: 1, ARMS[3]: 2, ARMS[4]: 2}

# (arm, (M, h, w), what is ragged).  "cols": the last 32-column tile is short (w % 32 != 0); "rows8": the last 8-row tile is short (h % 8 != 0); "rows16": h % 16 must
# lie in the stated range (the last 16-row tile); "half_block": M = 48, the second 32-channel block of the last group half empty
CASES = [
    (ARMS[1], (16, 125, 250), dict(cols=True, rows8=True)),
    (ARMS[1], (48, 125, 125), dict(cols=True, rows8=True, half_block=True)),
    (ARMS[1], (96, 61, 170), dict(cols=True, rows8=True)),
    (ARMS[2], (64, 125, 250), dict(cols=True, rows8=True)),
    (ARMS[2], (512, 29, 100), dict(cols=True, rows8=True)),
    (ARMS[3], (512, 125, 250), dict(cols=True, rows16=(13, 13))),               # last 16-row tile: 13 rows
    (ARMS[3], (512, 120, 248), dict(cols=True, rows16=(8, 8))),                 # last 16-row tile: 8 rows, its second half wholly outside the image; w % 8 == 0
    (ARMS[3], (512, 61, 250), dict(cols=True, rows16=(9, 15))),
    (ARMS[4], (512, 21, 250), dict(cols=True, rows8=True)),                     # (the 16-row grid is too small)
    (ARMS[4], (512, 130, 120), dict(cols=True, rows8=True)),                    # (h > 128)
    (ARMS[4], (64, 250, 250), dict(cols=True, rows8=True)),                     # (one channel group)
]


def case_id(case):
    arm, (M, h, w), _ = case
    return f"{arm.replace(' ', '_')}-M{M}-{h}x{w}"


def case_batch(cu, case):
    """the smallest batch at which the launch of `case` takes its arm on cu compute units (the search of bnfold_checks.arm_shape).  The cases were chosen on 256 CUs;
    they also hold on 128 and 192 (test_conv_forms_host.py).  On 304 CUs (512, 21, w) goes from `1,2,4 inb=2` straight to `2,4,2` and the search fails by name."""
    arm, (M, h, w), _ = case
    for n in range(1, 1025):
        if h2_arm(cu, n, h, w, M) == arm:
            return n
    raise AssertionError(f"no batch up to 1024 reaches arm {arm} at {cu} CUs with (M, h, w) = {(M, h, w)}")


def bits_case(case):
    """the case at a width the sign-bit words need (w % 8 == 0, M % 32 == 0) with the same tile counts and still a short last column tile, or None"""
    arm, (M, h, w), rag = case
    w8 = w - w % 8
    if M % 32 or w8 % 32 == 0 or cdiv(w8, 32) != cdiv(w, 32):
        return None
    return (arm, (M, h, w8), rag)


BITS_CASES = [c for c in map(bits_case, CASES) if c is not None]
# the ELU / dropout (GEN) instances: arms 2,4,2 and 2,2,2, where U-Net++ runs them, and one 1,2,4 case
GEN_CASES = [c for c in CASES if c[0] in (ARMS[3], ARMS[4])] + [CASES[2]]
# the folded-BatchNorm data gradient (cin = M, cout = 16): the same two arms plus (96, 61, 170)
FOLD_CASES = [c for c in CASES if c[0] in (ARMS[3], ARMS[4])] + [CASES[2]]
# the folded-BatchNorm forward (cin = 16, cout = M): unet_conv3x3_bnfold_supported takes cout only where 256 % cout == 0 (the border sums of its weight gradient), which
# leaves (16, 125, 250) and (64, 250, 250) of the table; M = 256 reaches the 16-row instance (both kinds of last tile) and the two-block 8-row one at one shape
FOLD_FWD_EXTRA = [
    (ARMS[3], (256, 125, 250), dict(cols=True, rows16=(13, 13))),
    (ARMS[3], (256, 120, 248), dict(cols=True, rows16=(8, 8))),
    (ARMS[4], (256, 125, 250), dict(cols=True, rows8=True)),
]
FOLD_FWD_CASES = [CASES[0], CASES[10]] + FOLD_FWD_EXTRA
# (so the `1,2,4 inb=1` folded forward runs M = 16 only.  The half-empty channel block M = 48 meets cout % 16 == 0 but, like M = 96, not 256 % cout == 0: a folded
#  forward with a half-empty block cannot be launched through the C ABI at all, and gets no test; the plain forward, data gradient and statistics run M = 48)

# ---- the statistics epilogue: launch_h2 takes an armed request only where the slot copies hold the sums, 2 c xw <= UNET_BN_SLOT_DOUBLES with xw = UNET_XW words per
# value in deterministic mode (exact window sums) and 1 otherwise; a launch that declines leaves the request to unet_bn_stats' ordinary pass, silently ---------------------
BN_SLOT_DOUBLES, XW = 2048, 4


def stats_epilogue_accepts(M, det):
    return 2 * M * (XW if det else 1) <= BN_SLOT_DOUBLES


STATS_CASES = CASES + FOLD_FWD_EXTRA                                                   # default context: every M up to 1024 is taken
STATS_DET_CASES = [c for c in STATS_CASES if stats_epilogue_accepts(c[1][0], True)]          # deterministic context: M <= 256 -- M = 256 reaches `2,4,2` and `2,2,2`


def is_ragged_as_named(case):
    """every property the case's dict names holds (and it names at least one)"""
    _, (M, h, w), rag = case
    ok = bool(rag)
    if rag.get("cols"):
        ok &= w % 32 != 0
    if rag.get("rows8"):
        ok &= h % 8 != 0
    if "rows16" in rag:
        lo, hi = rag["rows16"]
        ok &= lo <= h % 16 <= hi
    if rag.get("half_block"):
        ok &= M == 48
    return ok


# ---- plan_wgrad_h2 (kernels_wgrad_h2.hip), transcribed: ca = cin, cb = cout ------------------------------------------------------------------------------------------
def plan_wgrad_h2(n, h, w, ca, cb):
    R = 2
    WA = 2 if ca % 64 == 0 else 1
    WB = 2 if cb % 64 == 0 else 1
    WR = 4 // (WA * WB)
    if WR > R:
        R = 4
    tiles_a, tiles_b, strips = cdiv(ca, 32 * WA), cdiv(cb, 32 * WB), cdiv(w, 32)
    pairs, per = tiles_a * tiles_b, 9 * ca * cb
    units = n * strips
    target = 256 if (R == 4 and WA * WB > 1) else 512
    want = max(1, target // pairs)
    cap = max(1, (64 << 20) // per)
    want = min(want, cap)
    upb = max(1, units // want)
    ublocks = cdiv(units, upb)
    cps = max(1, want // ublocks)
    cps = min(cps, max(1, h // 8))
    rpc = cdiv(h, cps)
    rpc = cdiv(rpc, R) * R
    return dict(WA=WA, WB=WB, R=R, pairs=pairs, units=units, upb=upb, ublocks=ublocks, rows_per_chunk=rpc, chunks_per_strip=cdiv(h, rpc))


# (n, h, w, cin, cout): upb = 2 over 17 units -- nine unit blocks, the last one short, odd height -- and the even twin
WGRAD_CASES = [(17, 3, 20, 512, 512), (16, 4, 32, 512, 512)]


# ---- k_conv3x3_h2_dgrad_pool_sums: which instance of conv_h2_kernel<0, NB, RW, WPS, 2> ---------------------------------------------------------------------------------
POOL_FORMS = ("1,2,4", "2,4,2", "2,2,2")


def pool_sums_form(n, h, w, M):
    wgs16 = cdiv(w, 32) * cdiv(h, 16) * n * cdiv(M, 64)
    if M % 64 != 0:
        return POOL_FORMS[0]
    if h <= 128 and wgs16 >= 512:
        return POOL_FORMS[1]
    return POOL_FORMS[2]


POOL_CASE = ((1, 126, 250, 512, 16), 0.25)          # ((n, h, w, cin, cout), rate): even sizes for the 2 x 2 pool, wgs16 = 512


# ---- k_convT_h2_fwd: one block per workgroup on the four-block image, or the four-block form ----------------------------------------------------------------------------
CONVT_FORMS = ("1,2,2", "4,2,2")


def convT_fwd_form(cu, n, h, w, cout):
    if cdiv(w, 32) * cdiv(h, 8) * n * cdiv(4 * cout, 128) < cu and cout % 32 == 0:
        return CONVT_FORMS[0]
    return CONVT_FORMS[1]


CONVT_CASE = (2, 29, 250, 32, 128)          # (n, h, w, cin, cout): 256 four-block workgroups at 256 CUs, short last column tile


# ---- the source text the transcriptions mirror -----------------------------------------------------------------------------------------------------------------------
def normalised(text):
    return re.sub(r"\s+", " ", text)


DISPATCH_SOURCES = [
    # the four returns at the end of k_conv3x3_h2_fwd (bnfold_checks.h2_arm)
    ("kernels_conv_h2.hip", "static int h2_nb(int M) { return (M % 64) == 0 ? 2 : 1; }"),
    ("kernels_conv_h2.hip", "const int inb = h2_nb(M); const long long t8 = (long long)((wd + 31) / 32) * ((h + 7) / 8) * n;"),
    ("kernels_conv_h2.hip", "if (t8 * ((M + 31) / 32) < ctx->num_cu) return launch_h2<0, 1, 1, 4>(ctx, x, K, img, bias, mask, mask_mode, y, ldy, n, h, wd, K, M, act, rate, seed, s, mask_climit, h2_head_args(), inb);"),
    ("kernels_conv_h2.hip", "if (inb == 1) return launch_h2<0, 1, 2, 4>(ctx, x, K, img, bias, mask, mask_mode, y, ldy, n, h, wd, K, M, act, rate, seed, s, mask_climit);"),
    ("kernels_conv_h2.hip", "if (t8 * ((M + 63) / 64) < 2 * ctx->num_cu) return launch_h2<0, 1, 2, 4>(ctx, x, K, img, bias, mask, mask_mode, y, ldy, n, h, wd, K, M, act, rate, seed, s, mask_climit, h2_head_args(), 2);"),
    ("kernels_conv_h2.hip", "const long long wgs16 = (long long)((wd + 31) / 32) * ((h + 15) / 16) * n * ((M + 63) / 64); if (h <= 128 && wgs16 >= 512) return launch_h2<0, 2, 4, 2>(ctx, x, K, img, bias, mask, mask_mode, y, ldy, n, h, wd, K, M, act, rate, seed, s, mask_climit); "
                            "return launch_h2<0, 2, 2, 2>(ctx, x, K, img, bias, mask, mask_mode, y, ldy, n, h, wd, K, M, act, rate, seed, s, mask_climit); }"),
    # where launch_h2 takes an armed statistics request (stats_epilogue_accepts)
    ("common.h", "constexpr int UNET_BN_SLOTS = 64, UNET_BN_SLOTS_DET = 1024, UNET_BN_SLOT_DOUBLES = 2048;"),
    ("common.h", "constexpr int UNET_XW = 4;"),
    ("kernels_conv_h2.hip", "const int xw = ctx->opt_deterministic ? UNET_XW : 1; if ((mask_mode == MASK_NONE || mask_mode == MASK_BIAS_TAB) && 2 * c * xw <= UNET_BN_SLOT_DOUBLES && "
                            "c == (MODE == 1 ? M / 4 : M) && ctx->bn_slots) {"),
    # k_conv3x3_h2_dgrad_pool_sums
    ("kernels_conv_h2.hip", "if (h2_nb(M) == 1) r = launch_h2<0, 1, 2, 4, 2>(ctx, dy, K, img, nullptr, pooled, MASK_POOL_SUMS,"),
    ("kernels_conv_h2.hip", "else if (h <= 128 && wgs16 >= 512) r = launch_h2<0, 2, 4, 2, 2>(ctx, dy, K, img, nullptr, pooled, MASK_POOL_SUMS,"),
    ("kernels_conv_h2.hip", "else r = launch_h2<0, 2, 2, 2, 2>(ctx, dy, K, img, nullptr, pooled, MASK_POOL_SUMS,"),
    # k_convT_h2_fwd
    ("kernels_conv_h2.hip", "if ((long long)((wd + 31) / 32) * ((h + 7) / 8) * n * ((4 * cout + 127) / 128) < ctx->num_cu && (cout % 32) == 0) return launch_h2<1, 1, 2, 2>(ctx, x, cin, img, bias,"),
    ("kernels_conv_h2.hip", "return launch_h2<1, 4, 2, 2>(ctx, x, cin, img, bias, nullptr, MASK_NONE, y, ldy, n, h, wd, cin, 4 * cout, ACT_NONE, 0.0f, 0, s); }"),
    # plan_wgrad_h2
    ("kernels_wgrad_h2.hip", "constexpr int wgrad_h2_rows() { return 2; }"),
    ("kernels_wgrad_h2.hip", "p.WA = (ca % 64) == 0 ? 2 : 1; p.WB = (cb % 64) == 0 ? 2 : 1; p.WR = 4 / (p.WA * p.WB);"),
    ("kernels_wgrad_h2.hip", "if (p.WR > R) R = 4; p.tiles_a = (ca + 32 * p.WA - 1) / (32 * p.WA); p.tiles_b = (cb + 32 * p.WB - 1) / (32 * p.WB); p.strips = (w + 31) / 32; "
                             "const long long pairs = (long long)p.tiles_a * p.tiles_b, per = 9LL * ca * cb; const long long units = (long long)n * p.strips; "
                             "const long long target = R == 4 && p.WA * p.WB > 1 ? 256LL : 512LL;"),
    ("kernels_wgrad_h2.hip", "long long want = std::max<long long>(1, target / pairs); const long long cap = std::max<long long>(1, (64LL << 20) / per); want = std::min(want, cap); "
                             "p.units = (int)units; p.upb = (int)std::max<long long>(1, units / want); const long long ublocks = (units + p.upb - 1) / p.upb; "
                             "long long cps = std::max<long long>(1, want / ublocks); cps = std::min<long long>(cps, std::max<long long>(1, h / 8)); "
                             "int rpc = (int)((h + cps - 1) / cps); rpc = (rpc + R - 1) / R * R;"),
    ("kernels_wgrad_h2.hip", "p.rows_per_chunk = rpc; p.chunks_per_strip = (h + rpc - 1) / rpc; p.nsplit = (int)(ublocks * p.chunks_per_strip); p.nslabs = p.nsplit; "
                             "p.floats = (size_t)p.nslabs * (per + cb)"),
]


def strip_comments(src):
    """C++ source without its // comments (the pinned statements are separated by them in the files)"""
    return re.sub(r"//[^\n]*", "", src)
