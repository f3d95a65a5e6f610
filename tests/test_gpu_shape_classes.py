"""Every launch list the hot path's size rules produce, run end to end against the CPU oracle (MI355X).

One test per case of tests/shape_classes.py ``CASES``: the smallest grid member of each distinct launch list
(tests/test_shape_classes_host.py holds the list to the grid).  Inputs are built directly (helpers.fullsize_inputs:
smooth texture, planar disparity, no backbone), weights are seeded, and every case checks

* the real plan's launch list against the signature the case stands for: the dry and the real emission agree, and
  the library accepted every launch the Python rules chose;
* the eager modules' aggregated cost against the oracle's (COST_REL_TOL);
* S / M: every training-mode output against the oracle's (EPE <= EPE_TOL, relative max error <= 1e-4);
* L (``regression_topk`` is discontinuous, and one flip's dilated mask would cover these small images, so the
  metric is decomposed): (a) top-2 flips only where the oracle's 2nd-minus-3rd margin is within 2 x COST_REL_TOL x
  max |cost|, ``init`` within EPE_TOL over the non-flipped pixels, at least 1 - NEAR_TIE_CAP of all; (b) the plan's
  outputs bitwise equal to the eager upsampler on the HIP ``init``; (c) the eager upsampler on the ORACLE's
  ``init_pred`` against the oracle's outputs at every pixel.

The cases of one (config, maxdisp) share one model object, so its four-entry plan cache evicts and closes plans
with built graphs; after the group's last case its first one runs again and must give the same bits.  A failure
names the case and the first stage that is off: stem, agg, cost, init, then the disparities coarsest first.
"""
import contextlib
import io
import time

import pytest
import torch

import shape_classes as S
from hot_checks import DISP_REL_TOL, epe, flips_and_margin, hip_stages, rel
from parity import COST_REL_TOL, EPE_TOL, init_nonflip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd.backbone import StubFeature  # noqa: E402
from oracle import esm_oracle as O  # noqa: E402

DEV = torch.device("cuda")
_CFG = {c: i for i, c in enumerate(S.CONFIGS)}
ORDERED = sorted(S.CASES, key=lambda c: (_CFG[c[0]], c[1], c[2] * c[3] * c[4], c[2], c[3], c[4]))
LAST = {}  # (config, maxdisp) -> its last case in ORDERED
for _c in ORDERED:
    LAST[_c[:2]] = _c


@pytest.fixture(scope="module")
def group():
    """The model of the current (config, maxdisp), its CPU weights, and the first case run on it."""
    st = {"key": None, "model": None}
    yield st
    if st["model"] is not None:
        st["model"].invalidate_plans()


def _enter(st, cfg, md):
    if st["key"] != (cfg, md):
        if st["model"] is not None:
            st["model"].invalidate_plans()
        var, cv, bb, cvs, _ = S.CONFIGS[cfg]
        sd = S.state(cfg)
        with contextlib.redirect_stdout(io.StringIO()):  # (the constructor names its cost volume)
            model = E.ESMStereo(md, cv == "gwc", cv == "nc", bb, cvs, feature_cls=StubFeature)
        model.load_state_dict(sd)
        st.update(key=(cfg, md), model=model.eval().to(DEV), sd=sd, first=None)
    return st["model"], st["sd"]


class _Stages:
    """Measurements in pipeline order.  ``off`` marks a stage as wrong; only the asserted ones fail the test, and
    the message names the first stage that is off (an unasserted earlier stage locates the cause)."""

    def __init__(self, name):
        self.name, self.rows = name, []

    def add(self, stage, ok, detail, asserted=True):
        self.rows.append((stage, bool(ok), asserted, detail))

    def guard(self, stage, fn, asserted=True):
        """Run a check that asserts on its own (tests/parity.py) as one stage."""
        try:
            self.add(stage, True, fn(), asserted)
        except AssertionError as e:
            self.add(stage, False, str(e), asserted)

    def finish(self):
        off = [r for r in self.rows if not r[1]]
        for stage, ok, _, detail in self.rows:
            print(f"  {self.name} {stage}: {'ok' if ok else 'OFF'} {detail}")
        failed = [r for r in off if r[2]]
        assert not failed, (f"{self.name}: first stage off: {off[0][0]} ({off[0][3]}); failed checks: "
                            f"{[(r[0], r[3]) for r in failed]}")


def _disp_stage(st, stage, got, ref, asserted=True):
    e, r = epe(got, ref), rel(got, ref)
    st.add(stage, e <= EPE_TOL and r <= DISP_REL_TOL, f"EPE {e:.3g} rel max {r:.3g}", asserted)


@pytest.mark.parametrize("case", ORDERED, ids=S.case_id)
def test_launch_list_end_to_end(case, group):
    cfg, md, B, H, W = case
    cvs, gwc = S.CONFIGS[cfg][3], S.CONFIGS[cfg][1] == "gwc"
    D = md // cvs
    name = S.case_id(case)
    model, sd = _enter(group, cfg, md)
    t0 = time.perf_counter()
    ml, mr, att, up = S.case_inputs(case)
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    dml, dmr, datt, dup = dev(ml), dev(mr), dev(att), [dev(u) for u in up]
    outs = model.hot_path(dml, dmr, datt, dup, True)
    torch.cuda.synchronize()
    t_hip = time.perf_counter() - t0
    if group["first"] is None:
        group["first"] = (case, (dml, dmr, datt, dup), [o.clone() for o in outs])

    # the launch list the plan was built with is the one the case stands for
    hp = next(reversed(model._plans.values()))
    got_sig, want_sig = S.signature_of(hp.ctx.meta), S.case_signature(*case)
    diff = [(a, b) for a, b in zip(got_sig, want_sig) if a != b]
    assert got_sig == want_sig, (name, "real plan vs dry emission (got, predicted)", len(got_sig), len(want_sig), diff[:4])
    assert hp.num_ops == len(want_sig)

    t0 = time.perf_counter()
    with torch.no_grad():
        ref = O.hot_path(sd, cvs, md, gwc, ml, mr, att, up)
    t_ref = time.perf_counter() - t0
    n = len(outs)
    assert n == sum(1 for k in ref if k.startswith("disp_")), name
    hip = hip_stages(model, dml, dmr, datt, D)
    st = _Stages(name)
    for k in ("stem", "agg"):  # (no tolerance of their own: they locate a failure, they are not one)
        st.add(k, rel(hip[k], ref[k]) <= COST_REL_TOL, f"rel {rel(hip[k], ref[k]):.3g}", asserted=False)
    st.add("cost", rel(hip["cost"], ref["cost"]) <= COST_REL_TOL, f"rel {rel(hip['cost'], ref['cost']):.3g}")
    cost = hip["cost"].squeeze(1)
    if cvs != 4:
        with torch.no_grad():
            init = E.disparity_regression(cost, D)
        e = epe(init, ref["init_pred"][:, 0])
        st.add("init", e <= EPE_TOL, f"EPE {e:.3g}", asserted=False)
        for i in reversed(range(n)):
            assert outs[i].shape == ref[f"disp_{i}"].shape, (name, i)
            _disp_stage(st, f"disp_{i}", outs[i], ref[f"disp_{i}"])
    else:
        with torch.no_grad():
            init = E.regression_topk(cost, None, 2)
            eager = model.upsample_module(*dup, init)
            eager_ref = model.upsample_module(*dup, ref["init_pred"].to(DEV))
        # (a) flips only where the oracle's own margin allows them; init on every other pixel
        flips, margin = flips_and_margin(cost, ref["cost"][:, 0])
        allowed = S.flip_margin(ref["cost"], COST_REL_TOL)
        wrong = flips & (margin > allowed)
        st.add("init flips", not wrong.any(), f"{int(flips.sum())} flips, {int(wrong.sum())} above the margin {allowed:.3g} "
               f"(largest flipped margin {float(margin[flips].max()) if flips.any() else 0.0:.3g})")
        st.guard("init", lambda: init_nonflip(name, init[:, 0], ref["init_pred"][:, 0], flips, margin))
        share = float((~flips).double().mean())
        st.add("init coverage", share >= 1.0 - S.NEAR_TIE_CAP, f"non-flipped share {share:.5f}")
        for i in reversed(range(n)):
            # (b) the compiled list is the eager pieces; (c) the upsampler on the oracle's own init, every pixel
            st.add(f"disp_{i} plan == eager", torch.equal(outs[i], eager[i].squeeze(1) * 4), "bitwise")
            _disp_stage(st, f"disp_{i} upsampler on the oracle's init", eager_ref[i].squeeze(1) * 4, ref[f"disp_{i}"])
    print(f"{name}: {len(want_sig)} launches; plan build + run {t_hip:.2f} s, oracle {t_ref:.2f} s")
    st.finish()

    if case == LAST[(cfg, md)]:
        # the group's cases went through one four-entry plan cache (evicted plans are closed with their graphs):
        # the first case again, same input tensors, must give the bits it gave the first time
        first, ins, want = group["first"]
        again = model.hot_path(*ins, True)
        assert len(model._plans) <= 4
        for i, (a, b) in enumerate(zip(again, want)):
            assert torch.equal(a, b), f"{name}: {S.case_id(first)} run again after the group: disp_{i} differs"
