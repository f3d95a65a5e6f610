"""The hot path's launch lists over the grid of tests/shape_classes.py, checked on the CPU (no GPU).

* every dry emission on ``GRID`` succeeds, eval and train outputs, and no conv launch of it asks the library for a
  form it refuses;
* ``CASES`` (what tests/test_gpu_shape_classes.py runs end to end) covers exactly the launch lists of ``GRID``: a
  threshold or form change that creates a new launch list fails here until a case is added
  (``python tests/shape_classes.py`` prints the list);
* ``THRESHOLDS``: every size constant of the rules has a grid point just on either side of it, the launch it
  decides differs between the two as the rule says, and both launch lists are among the ``CASES``;
* the near-tie condition of the ESMStereo-L cases holds on the oracle's own cost, so the GPU test's flip
  allowance can skip at most ``NEAR_TIE_CAP`` of the low-res pixels.
"""
import pytest
import torch

import shape_classes as S
from esmstereo_amd import engine
from parity import COST_REL_TOL

L_CASES = [c for c in S.CASES if S.CONFIGS[c[0]][3] == 4]


@pytest.fixture(scope="module")
def grid_classes():
    return S.classes(S.GRID)


def test_every_grid_emission_succeeds_eval_and_train():
    """The only errors a dry emission may raise are the reference's own (odd D, H or W not a multiple of 32), which
    the grid avoids; and every conv launch gets a form from the library (a negative value is its refusal)."""
    refused = []
    for p in S.GRID:
        for train in (False, True):
            sig = S.case_signature(*p, train)
            assert sig, p
            refused += [(p, train, e) for e in sig if e[1] == "conv" and str(e[2]).startswith("refused")]
        # the training outputs only add second, scaled stores: same launches, same forms, so the GPU cases (which
        # run the training outputs) stand for the eval launch lists as well
        assert S.case_signature(*p, False) == S.case_signature(*p, True), p
    assert not refused, refused[:8]


def test_cases_are_the_classes_of_the_grid(grid_classes):
    case_classes = S.classes(S.CASES)
    assert len(case_classes) == len(S.CASES), "two cases with one launch list"
    missing = [p for k, p in grid_classes.items() if k not in case_classes]
    assert not missing, f"launch lists of the grid without a case (python tests/shape_classes.py): {missing}"
    extra = [p for k, p in case_classes.items() if k not in grid_classes]
    assert not extra, f"cases whose launch list no grid point has: {extra}"
    # each case is its class's smallest member: fewest full-resolution pixels x B, then the smaller maxdisp
    assert sorted(grid_classes.values()) == sorted(S.CASES)
    assert set(S.CASES) <= set(S.GRID)


def test_every_conv_launch_of_every_case_has_a_form():
    for case in S.CASES:
        cfg, md, B, H, W = case
        for train in (False, True):
            for op in S.launches(cfg, md, B, H, W, train):
                if op["kind"] == "conv":
                    assert S.conv_form(op["key"], op["hint"]) >= 0, (case, train, op["name"], op["key"], hex(op["hint"]))


# ----------------------------------------------------------------------------- the size constants

Q4 = lambda c: c[2] * (c[3] // 4) * (c[4] // 4)      # noqa: E731  B x quarter-resolution pixels
Q2 = lambda c: c[2] * (c[3] // 2) * (c[4] // 2)      # noqa: E731  B x half-resolution pixels
Q16 = lambda c: c[2] * (c[3] // 16) * (c[4] // 16)   # noqa: E731
UP = "upsample_module."

# (rule, constant, which side of it takes the rule ("ge": quantity >= constant, "le": quantity <= constant), the
#  quantity of a grid point, the point off the rule and the launch it gets, the point on the rule and its launch).
# Each point's launch list is one of CASES' (test_cases_are_the_classes_of_the_grid), so both sides run on the GPU.
THRESHOLDS = [
    # engine.py
    ("gwc_stem_supported: B D h w", 1 << 16, "ge", lambda c: Q4(c) * (c[1] // 4),
     ("L-gwc", 48, 1, 256, 256), ("gwc_volume", "gwc"),
     ("L-gwc", 64, 1, 256, 256), ("gwc_volume+group_stem", "gwc_stem", "wreg", 0, 1)),
    ("pairk_auto PAIRK_MAX_VOX: B Ho Wo", engine.PAIRK_MAX_VOX, "le", Q16,
     ("S-gwc", 64, 2, 1024, 1024), (UP + "spx_2x.0", "conv", "small", 0),
     ("S-gwc", 64, 1, 1024, 1024), (UP + "spx_2x.0+1", "conv_pair", "ksplit")),
    ("FM2_MIN_PIX: B h w", engine.FM2_MIN_PIX, "ge", Q4,
     ("L-gwc", 64, 1, 480, 512), (UP + "blocks.0", "fmnet", 1),
     ("L-gwc", 64, 1, 512, 512), (UP + "blocks.0", "fmnet", 2)),
    ("shuffle_conv_supported SHUFFLE_CONV_MAX_PIX: B h w", engine.SHUFFLE_CONV_MAX_PIX, "le", Q4,
     ("L-gwc", 64, 1, 256, 544), (UP + "upsampling2+tail2x", "shuffle_tail", "window", 0),
     ("L-gwc", 64, 1, 256, 512), (UP + "upsampling2+tail2x+ref2x.conv1.0", "shuffle_conv", "window", 0)),
    ("XCD_SLAB_MIN_PIX: B H W", engine.XCD_SLAB_MIN_PIX, "ge", lambda c: c[2] * c[3] * c[4],
     ("S-gwc", 64, 1, 224, 256), (UP + "ref4x.conv1_up", "conv", "general", 0),
     ("S-gwc", 64, 1, 256, 256), (UP + "ref4x.conv1_up", "conv", "general", 1)),
    ("XCD_SLAB_MIN_VOX_WIDE: B D h w, >= 32 input channels", engine.XCD_SLAB_MIN_VOX_WIDE, "ge",
     lambda c: Q16(c) * (c[1] // 16),
     ("S-gwc", 64, 1, 1024, 992), ("group_stem", "conv", "stem", 0),
     ("S-gwc", 64, 1, 1024, 1024), ("group_stem", "conv", "stem", 1)),
    # the library's select_form
    ("tile3_auto: B Do Ho Wo", 1 << 16, "ge", lambda c: Q4(c) * (c[1] // 4),
     ("L-nc", 48, 1, 256, 256), ("corr_stem", "conv", "stem", 0),
     ("L-nc", 64, 1, 256, 256), ("corr_stem", "conv", "tile3", 1)),
    ("tile2_auto: B Ho Wo x 16-cout tiles (32 couts)", 1 << 19, "ge", lambda c: Q2(c) * 2,
     ("L-gwc", 64, 1, 1024, 992), (UP + "ref4x.conv1.1", "conv", "stem", 1),
     ("L-gwc", 64, 1, 1024, 1024), (UP + "ref4x.conv1.1", "conv", "tile2", 1)),
    ("pw_auto: B Hi Wi", 1 << 16, "ge", Q2,
     ("L-gwc", 64, 1, 480, 512), (UP + "ref4x.agg_1.0", "conv", "small", 0),
     ("L-gwc", 64, 1, 512, 512), (UP + "ref4x.agg_1.0", "conv", "pw", 1)),
    ("small_auto: B Ho Wo x one 16-cout tile", 1 << 17, "le", Q2,
     ("S-gwc", 64, 1, 544, 1024), (UP + "ref4x.agg_1.1", "conv", "general", 1),
     ("S-gwc", 64, 1, 512, 1024), (UP + "ref4x.agg_1.1", "conv", "small", 1)),
    ("stem_auto: B Ho Wo (32 -> 32)", 65536, "ge", Q2,
     ("L-gwc", 64, 1, 480, 512), (UP + "ref4x.conv1.1", "conv", "small", 0),
     ("L-gwc", 64, 1, 512, 512), (UP + "ref4x.conv1.1", "conv", "stem", 1)),
    ("c1in: B Ho Wo", 65536, "ge", Q2,
     ("L-gwc", 64, 1, 480, 512), (UP + "ref4x.conv1.0", "conv", "small", 1),
     ("L-gwc", 64, 1, 512, 512), (UP + "ref4x.conv1.0", "conv", "c1in", 1)),
]


@pytest.mark.parametrize("row", THRESHOLDS, ids=[r[0].split(":")[0].replace(" ", "_") for r in THRESHOLDS])
def test_threshold_has_a_case_on_either_side(row):
    rule, const, side, quantity, off, off_entry, on, on_entry = row
    q_off, q_on = quantity(off), quantity(on)
    if side == "ge":
        assert q_off < const <= q_on, (rule, q_off, const, q_on)
    else:
        assert q_on <= const < q_off, (rule, q_on, const, q_off)
    sig_off, sig_on = S.case_signature(*off), S.case_signature(*on)
    assert off_entry in sig_off and off_entry not in sig_on, (rule, off, [e for e in sig_off if e[0] == off_entry[0]])
    assert on_entry in sig_on and on_entry not in sig_off, (rule, on, [e for e in sig_on if e[0] == on_entry[0]])
    # both launch lists run end to end: each is the launch list of a case, which is then on the same side
    reps = {(c[0], S.case_signature(*c)): c for c in S.CASES}
    for p, sig in ((off, sig_off), (on, sig_on)):
        assert (p[0], sig) in reps, (rule, p, "its launch list has no case")
        q = quantity(reps[(p[0], sig)])
        assert (q >= const if side == "ge" else q <= const) == (p is on), (rule, p, reps[(p[0], sig)], q)
    print(f"{rule}: {const}; off the rule {S.case_id(reps[(off[0], sig_off)])}, on it {S.case_id(reps[(on[0], sig_on)])}")


def test_pair2_auto_pixel_cap_decides_no_hot_path_launch():
    """``pair2_auto``'s last clause (a 1x1 convA, at most 8192 output pixels) is the one size constant with no case
    on either side: the only pairs with a 1x1 first conv are the hourglasses' agg_N.0 + agg_N.1, and those either go
    to the fused ConvTranspose + 1x1 launch (CONVT1X1_PAIRED, the default, whatever pair2_auto says) or have a first
    conv the LDS-staged pair does not run (3-D, more than 64 input channels, or 32 outputs).  So no launch list of
    the grid holds an LDS-staged pair that starts with a 1x1; if one appears, the cap needs its two cases."""
    assert engine.CONVT1X1_PAIRED and engine.CONVT1X1_ENABLED
    for p in S.GRID:
        for op in S.launches(*p, True):
            if op["kind"] == "conv_pair":
                assert " k1s1 " not in op["shape"].split(" + ")[0], (p, op["name"], op["shape"])


# ----------------------------------------------------------------------------- ESMStereo-L: near ties

@pytest.fixture(scope="module")
def l_states():
    return {cfg: S.state(cfg) for cfg in S.CONFIGS if S.CONFIGS[cfg][3] == 4}


@pytest.mark.parametrize("case", L_CASES, ids=S.case_id)
def test_l_case_near_tie_share_within_the_cap(case, l_states):
    """A top-2 flip is legitimate only where the oracle's 2nd-minus-3rd margin is at most 2 x COST_REL_TOL x
    max |cost| (each cost may move by COST_REL_TOL x max |cost|); the case's input seed keeps the share of such
    pixels in the oracle's own cost within NEAR_TIE_CAP, so check (a) of the GPU test covers >= 98 % of them."""
    with torch.no_grad():
        cost = S.oracle_cost(case, l_states[case[0]])
    share = S.near_tie_share(cost, COST_REL_TOL)
    print(f"{S.case_id(case)}: {100 * share:.3f} % of the low-res pixels within the flip margin "
          f"{S.flip_margin(cost, COST_REL_TOL):.3g} (max |cost| {float(cost.abs().max()):.4f})")
    assert share <= S.NEAR_TIE_CAP, (S.case_id(case), share)
