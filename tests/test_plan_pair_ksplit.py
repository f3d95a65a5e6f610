"""The K-split conv pair's automatic rule (engine.pair2_auto / pairk_auto) on the S-K plan, without a GPU: the
plan is emitted dry with the rule on and with its switch off (engine.PAIRK_ENABLED, the ESM_PAIRK A/B knob).
Each pair the rule takes replaces two conv launches by one ``conv_pair`` op whose bytes are the two convs'
minus the intermediate map's store and re-read."""
import math
import re

import pytest

from esmstereo_amd import engine as EN
from test_plan_cost import CASES, _plan

B = CASES["S-K"][3]


def _ops(enabled, case="S-K"):
    on0 = EN.PAIRK_ENABLED
    EN.PAIRK_ENABLED = enabled
    try:
        return _plan(case)[2]
    finally:
        EN.PAIRK_ENABLED = on0


def test_rule_replaces_two_launches_by_one_pair():
    on, off = _ops(True), _ops(False)
    n = len(off) - len(on)
    assert n > 0, "the rule takes at least one pair of the S-K plan"
    off_by = {x["name"]: x for x in off}
    new = [x for x in on if x["kind"] == "conv_pair" and x["name"] not in off_by]
    pairs = lambda ops: sum(x["kind"] == "conv_pair" for x in ops)  # noqa: E731
    assert pairs(on) - pairs(off) == n == len(new)
    for x in new:
        assert x["name"].endswith(".0+1"), x["name"]
        first = x["name"][:-2]
        a, b = off_by[first], off_by[first[:-1] + "1"]
        assert a["kind"] == b["kind"] == "conv"
        assert x["flops"] == a["flops"] + b["flops"]
        g = re.search(r"->(\d+) in \S+ out (\S+)", a["shape"])
        mid = 4 * B * int(g.group(1)) * math.prod(int(v) for v in g.group(2).split("x"))  # the intermediate map
        assert x["bytes"] == a["bytes"] + b["bytes"] - 2 * mid, x["name"]
    # every launch the rule does not touch is unchanged
    gone = {x["name"][:-2] for x in new} | {x["name"][:-3] + "1" for x in new}
    assert [x["name"] for x in off if x["name"] not in gone] == [x["name"] for x in on if x not in new]


@pytest.mark.parametrize("case", ["L-K B4", "Mid"])
def test_rule_leaves_the_large_plans_alone(case):
    """ESMStereo-L's volumes and maps are far above the rule's range (and its 3-D levels wider than the form)."""
    assert [x["name"] for x in _ops(True, case)] == [x["name"] for x in _ops(False, case)]
