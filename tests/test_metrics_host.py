"""CPU tests: the numpy restatement of the disparity metrics (tests/metrics_ref.py) against the reference's
recorded results (tests/golden/metrics_ref.npz, written by tests/golden/make_golden_metrics.py).  Rates, skip and
NaN decisions and the error images are bit-equal; the EPE is held to the bound the generator measured."""
import os

import numpy as np
import pytest

import metrics_ref as MR
from helpers import GOLDEN_DIR

GOLD = np.load(os.path.join(GOLDEN_DIR, "metrics_ref.npz"))
F32 = np.float32


def bits(a):
    """fp32 bit patterns, with every NaN as one pattern."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    return np.where(np.isnan(a), F32(np.nan), a).view(np.uint32)


def restated(name):
    est, gt, mask, _ = MR.make_inputs(name)
    counts = [MR.image_counts(est[i], gt[i], mask[i]) for i in range(gt.shape[0])]
    return counts, [MR.image_values(c) for c in counts]


def test_fixture_describes_the_cases():
    assert tuple(GOLD["thres"]) == MR.THRES and float(GOLD["maxdisp"]) == MR.MAXDISP
    for name, (B, H, W, seed) in MR.CASES.items():
        assert tuple(GOLD[f"{name}/shape"]) == (B, H, W) and int(GOLD[f"{name}/seed"]) == seed
        planted = MR.make_inputs(name)[3]
        assert dict(zip(GOLD[f"{name}/planted_names"].tolist(), GOLD[f"{name}/planted_pos"].tolist())) == planted
    assert 2.0 ** -23 <= float(GOLD["epe_rel_bound"]) < 1e-5
    assert float(GOLD["epe_rel_bound"]) == max(4 * float(GOLD["epe_rel_measured"]), 2.0 ** -23)


def test_planted_values_are_where_the_cases_say():
    est, gt, mask, planted = MR.make_inputs("c312")
    e, g, m = est[0].ravel(), gt[0].ravel(), mask[0].ravel()
    for name, gv, ev, mv in MR.PLANTS:
        p = planted[name]
        assert g[p] == F32(gv) and (np.isnan(ev) and np.isnan(e[p]) or e[p] == F32(ev)), name
        assert m[p] == (mv if mv is not None else False), name
    E = np.abs(g - e)
    assert [E[planted[k]] for k in ("E1", "E2", "E3")] == [1, 2, 3]
    p = planted["rel_100_105"]  # False against the fp32 constant; against the double 0.05 the same quotient is True
    assert not E[p] / np.abs(g[p]) > F32(0.05) and float(E[p] / np.abs(g[p])) > 0.05
    est, gt, mask, planted = MR.make_inputs("c219")
    assert np.isnan(est[1].ravel()[planted["nan_inside"]]) and mask[1].ravel()[planted["nan_inside"]]


@pytest.mark.parametrize("name", list(MR.CASES))
def test_per_image_rates_and_skips_bit_equal(name):
    _, vals = restated(name)
    ref, skipped = GOLD[f"{name}/image"], GOLD[f"{name}/skipped"]
    assert [v["skipped"] for v in vals] == skipped.tolist()
    for i, v in enumerate(vals):
        if skipped[i]:
            continue  # the reference forms no value for an image it skips
        assert np.array_equal(bits(v["thres"]), bits(ref[i, 1:4])), (i, v["thres"], ref[i, 1:4])
        assert np.array_equal(bits(v["d1"]), bits(ref[i, 4:7])), (i, v["d1"], ref[i, 4:7])
        assert np.isnan(v["epe"]) == np.isnan(ref[i, 0])
        if not np.isnan(ref[i, 0]):
            assert abs(float(v["epe"]) - float(ref[i, 0])) <= float(GOLD["epe_rel_bound"]) * float(ref[i, 0])


def batch_close(mine, ref, n_kept):
    """NaN and the all-skipped 0 by kind; else two sequential fp32 sums of n non-negative terms + 1 ulp."""
    if np.isnan(ref) or np.isnan(mine):
        return np.isnan(ref) and np.isnan(mine)
    if n_kept == 0:
        return mine == 0 and ref == 0
    tol = 2 * (n_kept - 1) * 2.0 ** -24 * abs(float(ref)) + float(np.spacing(F32(abs(ref))))
    return abs(float(mine) - float(ref)) <= tol


@pytest.mark.parametrize("name", list(MR.CASES))
def test_batch_means(name):
    _, vals = restated(name)
    skipped = [v["skipped"] for v in vals]
    n_kept = skipped.count(False)
    ref = GOLD[f"{name}/batch"]
    cols = [[v["epe"] for v in vals]] + [[v["thres"][k] for v in vals] for k in range(3)] + \
           [[v["d1"][k] for v in vals] for k in range(3)]
    for c, col in enumerate(cols):
        mine = MR.batch_mean(col, skipped)
        if c == 0 and n_kept and not np.isnan(ref[c]):  # the per-image EPEs differ by the EPE bound already
            assert abs(float(mine) - float(ref[c])) <= (float(GOLD["epe_rel_bound"]) + 2 * n_kept * 2.0 ** -24) * \
                float(ref[c]), (mine, ref[c])
        else:
            assert batch_close(mine, ref[c], n_kept), (c, mine, ref[c])


@pytest.mark.parametrize("name", MR.VIS_CASES)
def test_error_image_bit_equal(name):
    est, gt, _, _ = MR.make_inputs(name)
    got, ref = MR.error_map(est, gt), GOLD[f"{name}/vis"]
    assert got.dtype == ref.dtype == F32 and got.shape == ref.shape
    assert np.array_equal(bits(got), bits(ref))


def test_error_image_bucket_edges():
    lo, col = MR.colour_table()
    gt = np.full((1, 12, 210), 20.0, F32)
    est = gt.copy()
    est[0, 11, :10] = gt[0, 11, :10] + (lo * F32(3)).astype(F32)  # E / 3 on every lower bound (all exact here)
    img = MR.error_map(est, gt)
    for i in range(10):
        assert np.array_equal(img[0, :, 11, i], col[i]), i
        assert np.array_equal(img[0, :, 0, 20 * i], col[i])  # legend
    assert np.array_equal(img[0, :, 10, 0], col[0])  # E = 0 inside the mask: the first colour
