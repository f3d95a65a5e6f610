"""Checks the GPU hot-path tests share: the eager HIP stages up to the aggregated cost, and the disparity metrics
of tests/test_gpu_parity.py's docstring (S / M: EPE <= 1e-3 px and relative max error <= 1e-4; L: the
flip-masked metric of tests/parity.py)."""
from __future__ import annotations

from typing import Dict

import torch

import esmstereo_amd as E
from esmstereo_amd.engine import Ctx
from parity import EPE_TOL, flip_masked, top2_sets

DISP_REL_TOL = 1e-4  # whole hot path, S / M: relative max error


def rel(a, b) -> float:
    a = a.detach().double().cpu()
    b = torch.as_tensor(b).double().cpu()
    return float((a - b).detach().abs().max() / b.detach().abs().max().clamp_min(1e-30))


def epe(a, b) -> float:
    return float((a.detach().double().cpu() - torch.as_tensor(b).double().cpu()).abs().mean())


def flips_and_margin(cost_hip, cost_ref):
    """[B, D, h, w] HIP and reference costs -> (flip set, reference v2 - v3 margin), [B, h, w]."""
    cost_ref = torch.as_tensor(cost_ref).double().cpu()
    flips = (top2_sets(cost_hip.detach().cpu()) != top2_sets(cost_ref)).any(1)
    sv = torch.sort(cost_ref, dim=1, descending=True)[0]
    return flips, sv[:, 1] - sv[:, 2]


def check_disp(name, got, ref, L=None):
    """S / M (continuous): EPE <= 1e-3 and relative max error <= 1e-4.  L: ``L = (cost_hip,
    cost_ref)`` [B, D, h, w] -> the flip-masked metric of SURVEY.md §8(d)(iii) (tests/parity.py)."""
    if L is None:
        e = epe(got, ref)
        assert e <= EPE_TOL, (name, e)
        assert rel(got, ref) <= DISP_REL_TOL, (name, rel(got, ref))
        return {"epe": e}
    flips, margin = flips_and_margin(*L)
    return flip_masked(name, got, ref, flips, margin, 4)


def hip_stages(model, ml, mr, att, D) -> Dict[str, torch.Tensor]:
    """Cost volume -> stem -> agg -> hourglass through the eager HIP modules: {"stem", "agg", "cost"}, named as
    the oracle's ``hot_path`` names them."""
    with torch.no_grad():
        if model.gwc:
            V = E.build_gwc_volume(ml, mr, D, 32, att=att)
            stem = model.group_stem(V)
        else:
            V = E.build_norm_correlation_volume(ml, mr, D)
            mul = att.reshape(att.shape[0], -1, *att.shape[-2:]) if att is not None else None
            stem = model.corr_stem.emit(Ctx(ml.device), [V], mul=mul)
        agg = model.agg(stem)
        return {"stem": stem, "agg": agg, "cost": model.aggregation_out(agg)}


def hip_cost(model, ml, mr, att, D):
    """Cost volume -> stems -> hourglass through the eager HIP modules."""
    return hip_stages(model, ml, mr, att, D)["cost"]
