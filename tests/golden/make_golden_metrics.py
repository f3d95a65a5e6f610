"""Record the reference's disparity metrics and error images: tests/golden/metrics_ref.npz.

    python tests/golden/make_golden_metrics.py [/path/to/reference]     (default /root/reference)

Loads the reference's utils/metrics.py and utils/visualization.py by file path and runs them on the CPU.
`import utils` itself needs torchvision (utils/experiment.py), so a stub `utils.experiment` that provides only
`make_nograd_func` stands in for it.  The inputs are the seeded cases of tests/metrics_ref.py, regenerated at
test time, so the file holds data only: per case the shape, the seed and the planted positions, the reference's
batch results, its per-image results (the reference called on [i:i+1]; whether it skipped the image is read
from the message it prints), and `vis` for the small cases.

`epe_rel_bound`: the reference sums |gt - est| in fp32 in an order it does not specify; the largest relative
distance between its fp32 EPE and the fp64 mean of the same data over all these cases, times 4 (one more rounding
on the other side, another summation order), floored at 2^-23.  Both sides run here on the CPU."""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import metrics_ref as MR  # noqa: E402


def load_reference(root):
    pkg = types.ModuleType("utils")
    pkg.__path__ = []
    exp = types.ModuleType("utils.experiment")
    exp.make_nograd_func = lambda f: torch.no_grad()(f)  # all the reference's metrics need of it
    sys.modules["utils"], sys.modules["utils.experiment"] = pkg, exp
    mods = []
    for name in ("metrics", "visualization"):
        spec = importlib.util.spec_from_file_location(f"utils.{name}", os.path.join(root, "utils", f"{name}.py"))
        m = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(m)
        mods.append(m)
    return mods


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    M, V = load_reference(root)

    def five(est, gt, mask):
        """(epe, thres1..3, d1_1..3), skipped: the reference on a batch."""
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), torch.no_grad():
            r = [M.EPE_metric(est, gt, mask)]
            r += [M.Thres_metric(est, gt, mask, t) for t in MR.THRES]
            r += [M.D1_metric_thres(est, gt, mask, t) for t in MR.THRES]
            d1 = M.D1_metric(est, gt, mask)
        assert all(x.dtype == torch.float32 for x in r)
        assert d1.numpy().tobytes() == r[6].numpy().tobytes()  # D1_metric is D1_metric_thres(3)
        return np.array([x.item() for x in r], np.float32), "skip" in buf.getvalue()

    out = {"thres": np.array(MR.THRES, np.float32), "maxdisp": np.float32(MR.MAXDISP)}
    worst = 0.0
    for name, (B, H, W, seed) in MR.CASES.items():
        est, gt, mask, planted = MR.make_inputs(name)
        te, tg, tm = torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask)
        out[f"{name}/shape"] = np.array([B, H, W], np.int64)
        out[f"{name}/seed"] = np.int64(seed)
        out[f"{name}/planted_names"] = np.array(sorted(planted))
        out[f"{name}/planted_pos"] = np.array([planted[k] for k in sorted(planted)], np.int64)
        out[f"{name}/batch"], _ = five(te, tg, tm)
        per, skip = zip(*[five(te[i:i + 1], tg[i:i + 1], tm[i:i + 1]) for i in range(B)])
        out[f"{name}/image"] = np.stack(per)
        out[f"{name}/skipped"] = np.array(skip, bool)
        for i in range(B):
            c = MR.image_counts(est[i], gt[i], mask[i])
            if c["n_mask"] and not skip[i] and np.isfinite(per[i][0]):
                exact = c["sum"] / c["n_mask"]
                worst = max(worst, abs(float(per[i][0]) - exact) / exact)
        if name in MR.VIS_CASES:
            out[f"{name}/vis"] = V.vis(est.copy(), gt.copy(), abs_thres=3., rel_thres=0.05, dilate_radius=1)
    out["epe_rel_measured"] = np.float64(worst)
    out["epe_rel_bound"] = np.float64(max(4 * worst, 2.0 ** -23))
    path = os.path.join(HERE, "metrics_ref.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes; fp32 EPE vs fp64 mean: {worst:.3e} relative at worst")


if __name__ == "__main__":
    main()
