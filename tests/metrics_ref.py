"""A numpy restatement of the disparity metrics (utils/metrics.py) and the KITTI error image
(utils/visualization.py:vis), written from their definitions: exact integer counts, an fp64 error sum, and the
fp32 operations the reference rounds in.  tests/test_metrics_host.py pins it to the recorded reference results
(tests/golden/metrics_ref.npz); the GPU tests use it where the fixture holds nothing (large shapes, strided views).

Also the test inputs: every case is regenerated from its seed, so the fixture stores no input."""
import numpy as np

F32 = np.float32
THRES = (1.0, 2.0, 3.0)
REL = 0.05
MAXDISP = 192.0

# name -> (B, H, W, seed).  The smallest shapes that reach each path of csrc/metrics.hip: a single pixel; W no
# multiple of 4 in one partial; the legend inside the image with H = 10 and H > 10; the legend clipped both ways;
# several partials per image; the KITTI size.
CASES = {
    "c1": (1, 1, 1, 11),
    "c37": (2, 7, 37, 12),
    "c203": (3, 10, 203, 13),
    "c219": (2, 13, 219, 14),
    "c150": (2, 6, 150, 15),
    "c312": (3, 96, 312, 16),
    "skipall": (2, 7, 37, 17),
    "kitti": (1, 375, 1242, 18),
}
VIS_CASES = ("c1", "c37", "c203", "c219", "c150")  # the fixture holds the reference's error image for these

# planted (gt, est, in the mask) triples, written to image 0 at seeded positions in this order
PLANTS = [
    ("E1", 10.0, 11.0, True), ("E2", 10.0, 12.0, True), ("E3", 50.0, 53.0, True),
    ("rel_100_105", 100.0, 105.0, True),   # 5 / 100 rounds to 0.05f: not > 0.05f, but > the double 0.05
    ("rel_60_63", 60.0, 63.0, True),
    ("gt_zero", 0.0, 5.0, None),           # None: whatever (gt > 0) & (gt < maxdisp) says
    ("gt_maxdisp", MAXDISP, 190.0, None),
    ("gt_negative", -5.0, 1.0, True),      # only an explicit mask can hold it
    ("nan_outside", 0.0, np.nan, False),
    ("edge_abs", 20.0, 23.0, True),        # E / 3 = 1.0: the lower edge of the sixth colour
    ("edge_first", 16.0, 16.1875, True),   # E / 3 = 0.0625 = float32(0.1875 / 3.0): the edge of the second
    ("edge_rel", 1.0, 1.05, True),
]
NAN_INSIDE = ("c37", "c219")  # est = NaN inside the mask of the LAST image: its EPE is NaN, its counts are not


def make_inputs(name):
    """(est, gt, mask, planted) for a case: fp32, fp32, bool [B, H, W], {plant name: flat index in image 0}."""
    B, H, W, seed = CASES[name]
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.5, 230.0, size=(B, H, W)).astype(F32)
    gt[rng.random((B, H, W)) < 0.3] = 0.0  # sparse ground truth
    noise = rng.standard_normal((B, H, W)) * np.where(rng.random((B, H, W)) < 0.2, 6.0, 0.8)
    est = (gt + noise.astype(F32)).astype(F32)
    drop = rng.random((B, H, W)) < 0.1
    planted = {}
    forced = []
    if H * W >= len(PLANTS) + 1:
        pos = rng.choice(H * W, size=len(PLANTS) + 1, replace=False)
        for (pname, g, e, m), p in zip(PLANTS, pos):
            gt[0].flat[p], est[0].flat[p] = g, e
            planted[pname] = int(p)
            forced.append((0, int(p), m))
        if name in NAN_INSIDE:
            p = int(pos[-1])
            gt[B - 1].flat[p], est[B - 1].flat[p] = 30.0, np.nan
            planted["nan_inside"] = p
            forced.append((B - 1, p, True))
    mask = (gt > 0) & (gt < F32(MAXDISP)) & ~drop
    for b, p, m in forced:
        if m is not None:
            mask[b].flat[p] = m
    if name == "c203":
        mask[1] = False                      # empty mask, positive gt: skipped
        mask[2] = False                      # empty mask, no positive gt: 0 / 0 is not < 0.1, kept, NaN
        gt[2] = -np.abs(gt[2])
    if name == "c312":
        mask[2] &= rng.random((H, W)) < 0.05  # mean(mask) / mean(gt > 0) ~ 0.04: skipped by the ratio
    if name == "skipall":
        mask[:] = False
    return est, gt, mask, planted


def range_mask(gt, maxdisp=MAXDISP):
    return (gt > 0) & (gt < F32(maxdisp))


def image_counts(est, gt, mask, thres=THRES, rel=REL):
    """One image -> {"n_mask", "n_gt_pos", "sum" (fp64), "n_abs": [..], "n_both": [..]}: exact integers."""
    est, gt = np.asarray(est, F32), np.asarray(gt, F32)
    mask = np.ones(gt.shape, bool) if mask is None else np.asarray(mask, bool)
    g, e = gt[mask], est[mask]            # selected, so nothing outside the mask reaches a result
    E = np.abs(g - e)                      # one fp32 operation
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = E / np.abs(g) > F32(rel)   # fp32 division, fp32 constant
    n_abs = [int(np.count_nonzero(E > F32(t))) for t in thres]
    n_both = [int(np.count_nonzero((E > F32(t)) & ratio)) for t in thres]
    return {"n_mask": int(mask.sum()), "n_gt_pos": int(np.count_nonzero(gt > 0)),
            "sum": float(E.astype(np.float64).sum()), "n_abs": n_abs, "n_both": n_both, "npix": int(gt.size)}


def image_values(c):
    """Counts -> {"epe", "thres": [..], "d1": [..]} as fp32 and "skipped", formed as the reference forms them."""
    with np.errstate(divide="ignore", invalid="ignore"):
        nm = F32(c["n_mask"])
        epe = F32(np.float64(c["sum"]) / np.float64(c["n_mask"]))
        thres = [F32(n) / nm for n in c["n_abs"]]
        d1 = [F32(n) / nm for n in c["n_both"]]
        npix = F32(c["npix"])
        skipped = bool((nm / npix) / (F32(c["n_gt_pos"]) / npix) < F32(0.1))
    return {"epe": epe, "thres": thres, "d1": d1, "skipped": skipped}


def batch_mean(values, skipped):
    """torch.stack(kept).mean() in fp32, summed in image order; 0 when nothing is kept."""
    kept = [F32(v) for v, s in zip(values, skipped) if not s]
    if not kept:
        return F32(0)
    s = F32(0)
    for v in kept:
        s = F32(s + v)
    return F32(s / F32(len(kept)))


def record(c, nthres_max=4):
    """The 12 doubles esm_disp_metrics_f32 writes for an image."""
    pad = [0] * (nthres_max - len(c["n_abs"]))
    return np.array([c["n_mask"], c["n_gt_pos"], c["sum"], 0] + c["n_abs"] + pad + c["n_both"] + pad, np.float64)


_EDGES = (0.0, 0.1875, 0.375, 0.75, 1.5, 3.0, 6.0, 12.0, 24.0, 48.0)
_RGB = ((49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144),
        (253, 174, 97), (244, 109, 67), (215, 48, 39), (165, 0, 38))


def colour_table():
    """(lower bounds [10] fp32, colours [10, 3] fp32): float32(x / 3.0) and float32(c) / float32(255)."""
    lo = np.array([x / 3.0 for x in _EDGES], np.float64).astype(F32)
    return lo, np.array(_RGB, F32) / F32(255)


def error_map(est, gt, abs_thres=3.0, rel_thres=0.05):
    """[B, H, W] fp32 pair -> the KITTI error image [B, 3, H, W] fp32."""
    est, gt = np.asarray(est, F32), np.asarray(gt, F32)
    B, H, W = gt.shape
    lo, col = colour_table()
    valid = gt > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        E = np.abs(gt - est)
        err = np.minimum(E / F32(abs_thres), (E / gt) / F32(rel_thres))  # NaN if either is
    valid &= (err >= lo[0]) & (err < F32(np.inf))
    idx = np.zeros(gt.shape, np.int64)
    idx[valid] = np.searchsorted(lo, err[valid], side="right") - 1   # the row with lo <= err < next lo
    out = np.zeros((B, 3, H, W), F32)
    for c in range(3):
        out[:, c] = np.where(valid, col[idx, c], F32(0))
    for i in range(len(lo)):                                           # the legend goes in last
        out[:, :, :10, 20 * i:20 * (i + 1)] = col[i][None, :, None, None]
    return out
