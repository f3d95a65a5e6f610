"""The descriptor domain of esm_conv_f32 on the CPU (tests/conv_domain.py): ``esm_conv_form`` over fake addresses.

For every generated descriptor the automatic rules (hint 0) must name a form whose ACCEPTS entry is true, and a forced
hint must be reported as the acceptance table's documented outcome says; outside the supported geometry the report is
ESM_FORM_GENERAL (whose launcher answers ESM_ERR_UNSUPPORTED: tests/test_gpu_conv_domain.py).  Coverage is a condition:
every (form, axis value) is accepted at least once or listed in ``NEVER``, and every form accepts at least 16 of its
random combinations.  Nothing is launched.
"""
import ctypes
from collections import defaultdict

import pytest
import torch

from conv_domain import (ACCEPTS, AXES, BASES, FORM_ID, FORM_NAME, FORMS, NEVER, OUTSIDE, SUPPORTED_GEOMETRY, all_cases,
                         axis_cases, expected, forced_form, random_cases)
from esmstereo_amd import _lib
from test_conv_forms_host import build_desc

CASES = all_cases()


def desc_of(c, hint):
    return build_desc(c.spec, hint, act=c.act, scale=c.bn == "bn", shift=c.bn != "none", post_scale=c.post)


def form_of(c, hint):
    d = desc_of(c, hint)
    return _lib.lib.esm_conv_form(ctypes.byref(d))


def test_generator_is_deterministic_and_unique():
    again = all_cases()
    assert [c.id for c in again] == [c.id for c in CASES]
    for f in FORMS:
        assert len(random_cases(f)) >= 64 and len({c.id for c in random_cases(f)}) == len(random_cases(f))


def test_conv_check_accepts_every_generated_descriptor():
    """The generator means to produce no descriptor that conv_check refuses: the count is zero, with either hint."""
    refused = [(c.id, _lib.lib.esm_last_error()) for c in CASES + OUTSIDE for h in (0, c.hint) if form_of(c, h) < 0]
    assert not refused, refused[:5]


@pytest.mark.parametrize("field,value,word", [("cin_pad", 8, b"cin_pad"), ("Cout", 0, b"Cout"), ("Wo", 1, b"extent"),
                                              ("stride", 3, b"stride"), ("kw", 2, b"kh"), ("nsrc", 0, b"nsrc")])
def test_a_refused_descriptor_has_a_negative_status_and_a_message(field, value, word):
    d = desc_of(axis_cases(BASES[0])[0], 0)
    setattr(d, field, value)
    assert _lib.lib.esm_conv_form(ctypes.byref(d)) == -1
    assert word in _lib.lib.esm_last_error()


@pytest.mark.parametrize("base", BASES, ids=lambda b: b.name)
def test_hint0_never_picks_a_form_that_refuses(base):
    """esm_conv_form with hint 0: the reported form's ACCEPTS is true (``*_auto`` within ``*_ok`` within what the
    launcher instantiates); with the forced hint: the acceptance table's outcome."""
    bad = []
    for c in axis_cases(base) + [r for r in random_cases(base.form) if r.base == base.name]:
        assert SUPPORTED_GEOMETRY(c), c.id  # (the generator varies neither kernel nor stride)
        auto = form_of(c, 0)
        if not ACCEPTS[FORM_NAME[auto]](c):
            bad.append((c.id, "hint 0", FORM_NAME[auto]))
        kind, form = expected(c)
        got = form_of(c, c.hint)
        if kind == "runs" and got != FORM_ID[form]:
            bad.append((c.id, "forced", got, form))
        if kind == "auto" and got != auto:
            bad.append((c.id, "steps aside", got, auto))
        if kind == "refused" and got != FORM_ID[forced_form(c)]:  # reported as forced: its launcher refuses
            bad.append((c.id, "refusing form", got))
    assert not bad, bad[:8]


@pytest.mark.parametrize("case", OUTSIDE, ids=lambda c: c.value)
def test_outside_the_supported_geometry_the_report_is_general(case):
    assert not SUPPORTED_GEOMETRY(case)
    assert form_of(case, 0) == _lib.FORM_GENERAL


def _never(form):
    out = {}
    for axis, values, reason in NEVER.get(form, []):
        assert reason
        for v in (values if values is not None else [None]):
            out[(axis, None if v is None else str(v))] = reason
    return out


@pytest.mark.parametrize("form", FORMS)
def test_coverage_every_axis_value_is_accepted_or_listed(form):
    accepted = defaultdict(int)
    hints = set()
    for b in BASES:
        if b.form != form:
            continue
        hints |= {("hint", hex(h)) for h in b.hints}
        for c in axis_cases(b):
            accepted[(c.axis, c.value)] += ACCEPTS[form](c)
    never = _never(form)
    want = {(ax, "+".join(map(str, v)) if isinstance(v, tuple) else str(v)) for ax, vals in AXES.items() for v in vals} | hints
    missing = sorted(k for k in want if not accepted[k] and k not in never and (k[0], None) not in never)
    stale = sorted(k for k in want if accepted[k] and (k in never or (k[0], None) in never))
    assert not missing, f"{form}: no accepted case for {missing}"
    assert not stale, f"{form}: NEVER lists values the form runs: {stale}"
    n = sum(ACCEPTS[form](c) for c in random_cases(form))
    assert n >= 16, f"{form}: only {n} accepted random combinations"


# ----------------------------------------------------------------------------- the fused launches' predicates


def _shape_only(*shape):
    return torch.empty(shape, device="meta")


def test_fused_predicates_answer_on_shape_only_tensors():
    """engine._pair2_lds_supported, pairk_supported and convt_1x1_supported need shapes alone; their answers are part
    of the GPU cases' ids (tests/test_gpu_conv_domain.py holds the launchers to them)."""
    from conv_domain_fused import PAIR_CASES, UP1_CASES, pair_query, up1_query
    ids = [f"{c.id} lds={int(l)} ksplit={int(k)}" for c in PAIR_CASES for l, k in [pair_query(c, _shape_only)]]
    ids += [f"{c.id} fused={int(up1_query(c, _shape_only))}" for c in UP1_CASES]
    assert len(set(ids)) == len(ids)
    assert any("lds=1" in i for i in ids) and any("lds=0" in i for i in ids)
    assert any("ksplit=1" in i for i in ids) and any("ksplit=0" in i for i in ids)
    assert any("fused=1" in i for i in ids) and any("fused=0" in i for i in ids)
