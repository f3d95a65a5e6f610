"""GPU tests of the disparity metrics and the KITTI error image (csrc/metrics.hip, esmstereo_amd/metrics.py) against
the reference's recorded results (tests/golden/metrics_ref.npz) and the numpy restatement (tests/metrics_ref.py,
pinned to the same fixture by tests/test_metrics_host.py).

Counts, rates, skip flags and error images are exact.  The derived bounds:
* EPE vs float32(fp64 mean): 1 fp32 ulp.  The kernel sums in fp64 (relative error <= n 2^-53 over n < 2^31
  non-negative terms), so only the final rounding and a double-rounding tie remain.
* EPE vs the reference's fp32 value: the fixture's `epe_rel_bound`, measured on the CPU by the generator between
  the reference and the fp64 mean (the code under test is not involved).
* batch mean vs torch.stack(kept).mean(): 2 (B - 1) 2^-24 relative + 1 ulp, two sequential fp32 sums of B
  non-negative terms; for the EPE column the per-image terms themselves differ by `epe_rel_bound`, which adds.
  NaN and the all-skipped 0 are compared by kind.
* fp64 error sum vs the restatement's (another order): 2 n 2^-53 relative."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import metrics_ref as MR  # noqa: E402
from helpers import GOLDEN_DIR  # noqa: E402

import esmstereo_amd  # noqa: E402
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd import metrics as EM  # noqa: E402

DEV = torch.device("cuda")
F32 = np.float32
GOLD = np.load(os.path.join(GOLDEN_DIR, "metrics_ref.npz"))
EPE_BOUND = float(GOLD["epe_rel_bound"])


def bits(a):
    """fp32 bit patterns, with every NaN as one pattern (0 / 0 has another sign bit on the host than on the GPU)."""
    a = np.ascontiguousarray(np.asarray(a, F32))
    return np.where(np.isnan(a), F32(np.nan), a).view(np.uint32)


def ulp(x):
    return float(np.spacing(F32(abs(x))))


@functools.lru_cache(maxsize=None)
def case(name):
    """(est, gt, mask, counts per image, values per image): computed once, shared, never written."""
    est, gt, mask, _ = MR.make_inputs(name)
    counts = [MR.image_counts(est[i], gt[i], mask[i]) for i in range(gt.shape[0])]
    for a in (est, gt, mask):
        a.setflags(write=False)
    return est, gt, mask, counts, [MR.image_values(c) for c in counts]


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(m):
    """DisparityMetrics -> numpy fields (one sync per field is fine in a test)."""
    return {k: getattr(m, k).cpu().numpy() for k in m.FIELDS}


def check_against_restatement(got, counts, vals, K=3):
    for i, (c, v) in enumerate(zip(counts, vals)):
        want = MR.record(c)
        rec = got["records"][i]
        assert np.array_equal(np.delete(rec, 2), np.delete(want, 2)), (i, rec, want)  # every count, exactly
        if np.isnan(want[2]):
            assert np.isnan(rec[2])
        else:
            assert abs(rec[2] - want[2]) <= 2 * c["n_mask"] * 2.0 ** -53 * want[2], (i, rec[2], want[2])
        assert got["n_valid"][i] == c["n_mask"] and bool(got["skipped"][i]) == v["skipped"]
        assert np.array_equal(bits(got["thres"][i]), bits(v["thres"][:K])), (i, got["thres"][i], v["thres"])
        assert np.array_equal(bits(got["d1"][i]), bits(v["d1"][:K])), (i, got["d1"][i], v["d1"])
        assert np.isnan(got["epe"][i]) == np.isnan(v["epe"])
        if not np.isnan(v["epe"]):
            assert abs(float(got["epe"][i]) - float(v["epe"])) <= ulp(v["epe"]), (i, got["epe"][i], v["epe"])


def batch_close(mine, ref, n_kept, extra_rel=0.0):
    if np.isnan(ref) or np.isnan(mine):
        return bool(np.isnan(ref) and np.isnan(mine))
    if n_kept == 0:
        return mine == 0 and ref == 0
    return abs(float(mine) - float(ref)) <= (2 * (n_kept - 1) * 2.0 ** -24 + extra_rel) * abs(float(ref)) + ulp(ref)


@pytest.mark.parametrize("name", list(MR.CASES))
def test_metrics_against_reference_and_restatement(name):
    est, gt, mask, counts, vals = case(name)
    got = host(EM.disparity_metrics(dev(est), dev(gt), dev(mask)))
    check_against_restatement(got, counts, vals)
    ref, skipped = GOLD[f"{name}/image"], GOLD[f"{name}/skipped"]
    assert got["skipped"].tolist() == skipped.tolist()
    for i in range(gt.shape[0]):
        if skipped[i]:
            continue  # the reference forms no value for an image it skips
        assert np.array_equal(bits(got["thres"][i]), bits(ref[i, 1:4])), (i, got["thres"][i], ref[i, 1:4])
        assert np.array_equal(bits(got["d1"][i]), bits(ref[i, 4:7])), (i, got["d1"][i], ref[i, 4:7])
        assert np.isnan(got["epe"][i]) == np.isnan(ref[i, 0])
        if not np.isnan(ref[i, 0]):
            assert abs(float(got["epe"][i]) - float(ref[i, 0])) <= EPE_BOUND * float(ref[i, 0]), (got["epe"][i], ref[i, 0])
    n_kept = skipped.tolist().count(False)
    bref = GOLD[f"{name}/batch"]
    mine = np.concatenate([got["batch_epe"][None], got["batch_thres"], got["batch_d1"]])
    assert batch_close(mine[0], bref[0], n_kept, EPE_BOUND), (mine[0], bref[0])
    for c in range(1, 7):
        assert batch_close(mine[c], bref[c], n_kept), (c, mine[c], bref[c])
        col = [(v["thres"] + v["d1"])[c - 1] for v in vals]  # same per-image bits, same order: same sum
        assert np.array_equal(bits(mine[c]), bits(MR.batch_mean(col, [v["skipped"] for v in vals])))


def test_kinds_of_image_are_all_there():
    """The decisions the cases were built for (so a change to the generator cannot quietly lose one)."""
    assert [v["skipped"] for v in case("c203")[4]] == [False, True, False]
    assert case("c203")[3][1]["n_mask"] == 0 and case("c203")[3][1]["n_gt_pos"] > 0
    assert case("c203")[3][2]["n_mask"] == 0 and case("c203")[3][2]["n_gt_pos"] == 0
    assert np.isnan(case("c203")[4][2]["epe"]) and np.isnan(case("c203")[4][2]["thres"][0])
    assert [v["skipped"] for v in case("c312")[4]] == [False, False, True] and case("c312")[3][2]["n_mask"] > 0
    assert all(v["skipped"] for v in case("skipall")[4])
    assert np.isnan(case("c219")[4][1]["epe"]) and not np.isnan(case("c219")[4][1]["thres"][0])
    got = host(EM.disparity_metrics(dev(case("skipall")[0]), dev(case("skipall")[1]), dev(case("skipall")[2])))
    assert got["batch_epe"] == 0 and not got["batch_thres"].any() and not got["batch_d1"].any()


def test_partials_per_image():
    per = _lib.METRICS_PARTIAL_BYTES
    assert _lib.lib.esm_disp_metrics_workspace(2, 7, 37) == 2 * per          # one partial per image
    assert _lib.lib.esm_disp_metrics_workspace(3, 96, 312) > 3 * 2 * per     # the second stage really sums
    assert _lib.lib.esm_disp_metrics_workspace(3, 96, 312) % (3 * per) == 0


@pytest.mark.parametrize("name", ["c312", "kitti"])
def test_two_runs_same_bits(name):
    est, gt, mask, _, _ = case(name)
    e, g, m = dev(est), dev(gt), dev(mask)
    a, b = host(EM.disparity_metrics(e, g, m)), host(EM.disparity_metrics(e, g, m))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def _embed(a, H, W, top, left, poison):
    """`a` [B, h, w] as the window (top, left) of a poisoned [B, H, W] device tensor: a view, not a copy."""
    big = torch.full((a.shape[0], H, W), poison, dtype=torch.bool if a.dtype == bool else torch.float32, device=DEV)
    big[:, top:top + a.shape[1], left:left + a.shape[2]] = dev(a)
    v = big[:, top:top + a.shape[1], left:left + a.shape[2]]
    assert v.data_ptr() != big.data_ptr() or (top, left) == (0, 0)
    return v


def test_kitti_crop_view_and_aligned_window():
    """The crop pred[:, 9:, 6:] of a padded 384 x 1248 map (row stride != W, base 8 bytes off a 16-byte boundary:
    every 16-byte group is misaligned), the contiguous tensor (row stride 1242: the groups' alignment changes from
    row to row) and a window of a 375 x 1244 buffer (aligned base and stride: aligned groups, scalar row tails) hold
    the same data and must give the same bits.  The surroundings are NaN (mask: True), so anything read outside
    the window shows."""
    est, gt, mask, counts, vals = case("kitti")
    plain = host(EM.disparity_metrics(dev(est), dev(gt), dev(mask)))
    crop = [_embed(est, 384, 1248, 9, 6, float("nan")), _embed(gt, 384, 1248, 9, 6, float("nan")),
            _embed(mask, 384, 1248, 9, 6, True)]
    vec = [_embed(est, 375, 1244, 0, 0, float("nan")), _embed(gt, 375, 1244, 0, 0, float("nan")),
           _embed(mask, 375, 1244, 0, 0, True)]
    assert crop[0].data_ptr() % 16 != 0 and crop[0].stride(1) == 1248
    assert all(t.data_ptr() % 16 == 0 and t.stride(1) == 1244 for t in vec)
    for views in (crop, vec):
        got = host(EM.disparity_metrics(*views))
        check_against_restatement(got, counts, vals)
        for k in plain:
            assert got[k].tobytes() == plain[k].tobytes(), k
        img = EM.vis(views[0], views[1]).cpu().numpy()
        assert np.array_equal(bits(img), bits(MR.error_map(est, gt)))


def test_innermost_stride_is_copied():
    est, gt, mask, counts, vals = case("c37")
    t = [dev(np.ascontiguousarray(a.transpose(0, 2, 1))).transpose(1, 2) for a in (est, gt, mask)]
    assert all(x.stride(2) != 1 for x in t)
    check_against_restatement(host(EM.disparity_metrics(*t)), counts, vals)
    assert np.array_equal(bits(EM.vis(t[0], t[1]).cpu().numpy()), bits(GOLD["c37/vis"]))


@pytest.mark.parametrize("name", list(MR.CASES))
def test_error_image_bit_equal(name):
    est, gt, _, _, _ = case(name)
    img = EM.vis(dev(est), dev(gt), abs_thres=3., rel_thres=.05, dilate_radius=1)
    assert img.dtype == torch.float32 and tuple(img.shape) == (gt.shape[0], 3) + gt.shape[1:] and img.is_cuda
    ref = GOLD[f"{name}/vis"] if name in MR.VIS_CASES else MR.error_map(est, gt)
    assert np.array_equal(bits(img.cpu().numpy()), bits(ref))
    assert esmstereo_amd.error_image is EM.vis


def test_error_image_bucket_edges():
    lo, col = MR.colour_table()
    gt = np.full((1, 12, 210), 20.0, F32)
    est = gt.copy()
    est[0, 11, :10] = gt[0, 11, :10] + (lo * F32(3)).astype(F32)  # E / 3 on every lower bound, e.g. gt = 20, E = 3
    est[0, 11, 10:13] = [np.nan, np.inf, -np.inf]                  # no row holds these: zero
    gt[0, 11, 13] = 0.0
    img = EM.vis(dev(est), dev(gt)).cpu().numpy()
    assert np.array_equal(bits(img), bits(MR.error_map(est, gt)))
    for i in range(10):
        assert np.array_equal(img[0, :, 11, i], col[i]), i
    assert not img[0, :, 11, 10:14].any()


def test_named_functions_agree_with_the_one_call():
    est, gt, mask, _, _ = case("c312")
    e, g, m = dev(est), dev(gt), dev(mask)
    all_ = EM.disparity_metrics(e, g, m)
    named = {"epe": EM.EPE_metric(e, g, m), "d1": EM.D1_metric(e, g, m),
             "d1_2": EM.D1_metric_thres(e, g, m, 2.0), "t1": EM.Thres_metric(e, g, m, 1.0),
             "t3": EM.Thres_metric(e, g, m, 3)}
    for v in named.values():
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda
    want = {"epe": all_.batch_epe, "d1": all_.batch_d1[2], "d1_2": all_.batch_d1[1], "t1": all_.batch_thres[0],
            "t3": all_.batch_thres[2]}
    for k in named:
        assert named[k].cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), k
    ref = GOLD["c312/batch"]
    assert batch_close(named["d1"].item(), ref[6], 2) and batch_close(named["t1"].item(), ref[1], 2)
    assert batch_close(named["epe"].item(), ref[0], 2, EPE_BOUND)
    for f in ("EPE_metric", "D1_metric", "D1_metric_thres", "Thres_metric", "disparity_metrics", "DisparityEvaluator"):
        assert getattr(esmstereo_amd, f) is getattr(EM, f)


@pytest.mark.parametrize("name", ["c37", "c312"])
def test_maxdisp_gate_equals_the_explicit_mask(name):
    est, gt, mask, _, _ = case(name)
    e, g = dev(est), dev(gt)
    rm = MR.range_mask(gt)
    counts = [MR.image_counts(est[i], gt[i], rm[i]) for i in range(gt.shape[0])]
    gated = host(EM.disparity_metrics(e, g, maxdisp=MR.MAXDISP))
    check_against_restatement(gated, counts, [MR.image_values(c) for c in counts])
    explicit = host(EM.disparity_metrics(e, g, (g > 0) & (g < MR.MAXDISP)))
    both = host(EM.disparity_metrics(e, g, dev(mask), maxdisp=MR.MAXDISP))
    anded = host(EM.disparity_metrics(e, g, dev(mask & rm)))
    for k in gated:
        assert gated[k].tobytes() == explicit[k].tobytes(), k
        assert both[k].tobytes() == anded[k].tobytes(), k
    nomask = host(EM.disparity_metrics(e, g))  # no mask at all: every pixel
    counts = [MR.image_counts(est[i], gt[i], None) for i in range(gt.shape[0])]
    check_against_restatement(nomask, counts, [MR.image_values(c) for c in counts])


def test_evaluator_nine_images_three_batches():
    est, gt, mask, _, _ = case("c312")
    ev = EM.DisparityEvaluator(capacity=4)  # grows twice
    vals, counts = [], []
    for k in range(3):
        e = (est + F32(0.25 * k)).astype(F32)
        ev.update(dev(e), dev(gt), dev(mask))
        counts += [MR.image_counts(e[i], gt[i], mask[i]) for i in range(3)]
    vals = [MR.image_values(c) for c in counts]
    s = ev.summary()
    kept = [v for v in vals if not v["skipped"]]
    assert len(ev) == s["images"] == 9 and s["kept"] == len(kept) == 6
    want = {"EPE": [v["epe"] for v in kept], "D1": [v["d1"][2] for v in kept]}
    want.update({f"Thres{t + 1}": [v["thres"][t] for v in kept] for t in range(3)})
    for k, col in want.items():
        m = float(np.mean(np.array(col, np.float64)))
        # rates: the same fp32 bits averaged in fp64 on both sides; EPE: each term within 1 ulp (2^-23 relative)
        assert abs(s[k] - m) <= (2.0 ** -23 if k == "EPE" else 1e-15) * m, (k, s[k], m)
    mae = float(np.mean([c["sum"] / c["n_mask"] for c in counts]))
    op = float(np.mean([c["n_abs"][2] / c["n_mask"] for c in counts]))
    assert abs(s["kitti_epe"] - mae) <= 1e-12 * mae and abs(s["kitti_gt3"] - op) <= 1e-15 * op
    gated = EM.DisparityEvaluator()
    gated.update(dev(est), dev(gt), maxdisp=MR.MAXDISP)
    rm = MR.range_mask(gt)
    c = [MR.image_counts(est[i], gt[i], rm[i]) for i in range(3)]
    assert abs(gated.summary()["kitti_gt3"] - np.mean([x["n_abs"][2] / x["n_mask"] for x in c])) <= 1e-15


def test_cpu_tensors_and_shape_mismatch_raise():
    est, gt, mask, _, _ = case("c37")
    e, g, m = (torch.from_numpy(np.array(a)) for a in (est, gt, mask))
    for f in (lambda: EM.disparity_metrics(e, g, m), lambda: EM.EPE_metric(e, g, m), lambda: EM.vis(e, g),
              lambda: EM.D1_metric(e.to(DEV), g, m.to(DEV)), lambda: EM.DisparityEvaluator().update(e, g, m)):
        with pytest.raises(RuntimeError):
            f()
    e, g, m = e.to(DEV), g.to(DEV), m.to(DEV)
    for f in (lambda: EM.EPE_metric(e[:, :5], g, m), lambda: EM.D1_metric(e, g, m[:1]),
              lambda: EM.Thres_metric(e[0], g[0], m[0], 1.0), lambda: EM.disparity_metrics(e, g[:, :, :30], m),
              lambda: EM.Thres_metric(e, g, m, torch.tensor(1.0))):
        with pytest.raises(AssertionError):  # utils/metrics.py:10-14 and :63 assert
            f()
    with pytest.raises(ValueError):
        EM.disparity_metrics(e, g, m, thres=(1, 2, 3, 4, 5))


def test_c_abi_error_paths():
    L = _lib.lib
    buf = torch.zeros(4096, device=DEV, dtype=torch.float32)
    p = buf.data_ptr()
    th = (ctypes.c_float * 5)(1, 2, 3, 4, 5)

    def call(B=1, H=2, W=2, nthres=3, work=p + 4096, est=p):
        return L.esm_disp_metrics_f32(est, 4, 2, p, 4, 2, None, 0, 0, B, H, W, 0.0, 192.0, 1, th, nthres, 0.05,
                                      work, p + 1024, p + 2048, p + 3072, None)

    assert call() == 0
    torch.cuda.synchronize()
    for bad in (dict(nthres=5), dict(nthres=-1), dict(work=None), dict(est=None), dict(H=65536, W=32768),
                dict(B=0), dict(W=0)):
        assert call(**bad) == -1, bad  # ESM_ERR_ARG, before anything is launched
        assert L.esm_last_error()
    assert L.esm_disp_metrics_workspace(1, 65536, 32768) == -1 and L.esm_disp_metrics_workspace(1, 0, 5) == -1
    assert L.esm_disp_metrics_workspace(1, 32768, 65535) > 0  # just below 2^31
    assert L.esm_disp_error_map_f32(p, 4, 2, p, 4, 2, None, 1, 2, 2, 3.0, 0.05, None) == -1
    assert L.esm_disp_error_map_f32(p, 4, 2, p, 4, 2, p + 1024, 1, 65536, 32768, 3.0, 0.05, None) == -1
    torch.cuda.synchronize()
