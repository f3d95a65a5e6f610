"""The tuned-hint table as data, checked on the CPU (no GPU): every key parses and round-trips, the windowed fp64
reference of tests/tuned_rows.py equals the slice of the full fp64 result, and every row is looked up by some plan
(recorded at ``engine.TUNED_HINTS`` itself during dry emissions, so rows met inside fused launches count)."""
import contextlib
import dataclasses
import io

import pytest
import torch
import torch.nn.functional as F

import esmstereo_amd as E
from esmstereo_amd import engine
from esmstereo_amd.backbone import StubFeature
from esmstereo_amd.model import plan_ops
from helpers import UP_LAYOUT, load_spec, seeded_state
from tuned_rows import format_key, load_table, parse_key, window_expect, window_ref, windows

TABLE = load_table()


def test_shipped_table_is_what_the_engine_loaded():
    assert TABLE and engine.TUNED_HINTS == TABLE


@pytest.mark.parametrize("key", sorted(TABLE))
def test_key_roundtrip(key):
    spec = parse_key(key)
    assert format_key(spec) == key
    assert spec.cin == sum(spec.cins) and len(spec.out_ext) == spec.nd


def test_key_flags_and_rejects():
    s = parse_key("2dT k4s2p1 16->1 B1 1x48x156 sh1u")
    assert (s.nd, s.transposed, s.k, s.s, s.p, s.cins, s.cout, s.B, s.Di, s.Hi, s.Wi, s.shuffle) == \
        (2, True, 4, 2, 1, (16,), 1, 1, 1, 48, 156, 1)
    assert (s.u, s.m, s.r, s.two) == (True, False, False, False) and s.out_ext == (96, 312)
    full = parse_key("3d k3s1p1 8+4->8 B32 48x96x312 sh1mr2")
    assert (full.u, full.m, full.r, full.two) == (False, True, True, True) and full.cins == (8, 4)
    assert parse_key("2d k1s1p0 8->64 B2 1x9x21 sh4").shuffle == 4
    # each flag alone and all together survive the round trip (a parser that drops one fails here)
    base = parse_key("2d k3s1p1 16->1 B3 1x10x38 sh1")
    for u in (False, True):
        for m in (False, True):
            for r in (False, True):
                for two in (False, True):
                    sp = dataclasses.replace(base, u=u, m=m, r=r, two=two)
                    assert parse_key(format_key(sp)) == sp
    for bad in ("2d k3s1p1 16->16 B1 1x24x78 sh1x",      # an unknown flag
                "2d k3s1p1 16->16 B1 1x24x78 sh1ru",     # flags out of conv_key's order
                "2d k3s1p1 16->16 B1 1x24x78 sh1 ",      # trailing text
                "4d k3s1p1 16->16 B1 1x24x78 sh1",       # an unknown layout
                "2d k3s1p1 16->16 B1 2x24x78 sh1",       # depth on a 2-D launch
                "2d k3s1p1 16->16 B1 24x78 sh1",         # extent of two
                "2dT k3s1p1 16->16 B1 1x24x78 sh1",      # a transposed conv that is not k4 s2 p1
                "2d k3s1p1 16+16+16+16->16 B1 1x24x78 sh1",  # more sources than a launch has
                "2d k3s1p1 016->16 B1 1x24x78 sh1",      # not conv_key's spelling
                "2d k5s1p0 16->16 B1 1x3x78 sh1",        # empty output
                "2d k3s1p1 16->16 B1 1x24x78"):
        with pytest.raises(ValueError):
            parse_key(bad)


# ----------------------------------------------------------------------------- window_ref == slice of the full result

REF_LAYERS = [  # (key of a small launch of the layer type, seed)
    "2d k3s1p1 5->7 B1 1x37x95 sh1", "2d k3s2p1 5->7 B1 1x37x95 sh1", "2d k3s2p1 4->6 B1 1x38x96 sh1",
    "2d k1s1p1 6->5 B1 1x30x90 sh1", "2d k5s1p1 1->6 B1 1x33x91 sh1", "2d k1s1p0 3+4->5 B1 1x29x85 sh1",
    "2dT k4s2p1 5->6 B1 1x19x47 sh1",
    "3d k3s1p1 4->5 B1 9x17x45 sh1", "3d k3s2p1 4->5 B1 9x17x45 sh1", "3d k3s2p1 3->4 B1 10x18x46 sh1",
    "3d k1s1p1 3->4 B1 7x15x43 sh1", "3d k5s1p1 1->3 B1 9x17x45 sh1", "3dT k4s2p1 4->3 B1 5x9x23 sh1",
]


def _full_ref(x, w, spec):
    if spec.transposed:
        return (F.conv_transpose3d if spec.nd == 3 else F.conv_transpose2d)(x[None], w, None, spec.s, spec.p)[0]
    return (F.conv3d if spec.nd == 3 else F.conv2d)(x[None], w, None, spec.s, spec.p)[0]


@pytest.mark.parametrize("key", REF_LAYERS)
def test_window_ref_equals_slice_of_full(key):
    """<= 1e-12 absolute on values of order 1 (fp64 sums of a few hundred products: ~1e-14), over the windows the
    GPU test takes (both corners, the mixed one, the seeded interior), 1-wide slivers at every border and random
    windows, with the extents of ``windows`` shrunk so that the small maps still have an interior."""
    spec = parse_key(key)
    g = torch.Generator().manual_seed(len(key))
    x = torch.randn(spec.cin, *spec.in_ext, generator=g, dtype=torch.float64)
    wshape = (spec.cin, spec.cout) if spec.transposed else (spec.cout, spec.cin)
    w = torch.randn(*wshape, *(spec.k,) * spec.nd, generator=g, dtype=torch.float64) / (spec.cin * spec.k ** spec.nd) ** 0.5
    full = _full_ref(x, w, spec)
    ext = spec.out_ext
    assert tuple(full.shape[1:]) == ext
    srcs = list(torch.split(x, list(spec.cins), 0))
    wins = [(lo, hi) for _, lo, hi in windows(spec, (3, 5, 12) if spec.nd == 3 else (8, 24))]
    assert len(wins) == 4
    assert wins[0][0] == (0,) * spec.nd and wins[1][1] == ext  # the two all-low / all-high corners are there
    for d in range(spec.nd):  # one-cell slivers at both ends of every dim, whole extent in the others
        for a in (0, ext[d] - 1):
            wins.append((tuple(a if i == d else 0 for i in range(spec.nd)),
                         tuple(a + 1 if i == d else ext[i] for i in range(spec.nd))))
    for _ in range(12):
        lo = tuple(int(torch.randint(0, e, (1,), generator=g)) for e in ext)
        hi = tuple(a + 1 + int(torch.randint(0, e - a, (1,), generator=g)) for a, e in zip(lo, ext))
        wins.append((lo, hi))
    worst = 0.0
    for lo, hi in wins:
        got = window_ref(srcs, w, spec, lo, hi)
        ref = full[(slice(None),) + tuple(slice(a, b) for a, b in zip(lo, hi))]
        assert got.shape == ref.shape and got.dtype == torch.float64
        worst = max(worst, float((got - ref).abs().max()))
    print(f"{key}: {len(wins)} windows, worst |window - slice| {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("key", ["2d k3s1p1 6->1 B2 1x20x44 sh1u", "2dT k4s2p1 6->1 B2 1x10x22 sh1umr",
                                 "3d k3s1p1 4->5 B2 5x9x21 sh1mr", "2d k3s2p1 3+4->5 B2 1x21x45 sh1r"])
def test_window_expect_equals_slice_of_full_epilogue(key):
    """The epilogue the GPU test pushes its windows through (BN, GELU, * mul over D, + res, + bilinear(up, 2)) equals
    the slice of the same chain on the whole tensor, <= 1e-12."""
    spec = parse_key(key)
    g = torch.Generator().manual_seed(len(key))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    x = rn(spec.B, spec.cin, *spec.in_ext)
    w = rn(*((spec.cin, spec.cout) if spec.transposed else (spec.cout, spec.cin)), *(spec.k,) * spec.nd) / 4
    scale, shift = rn(spec.cout), rn(spec.cout)
    ext = spec.out_ext
    mul = rn(spec.B, spec.cout, *ext[-2:]) if spec.m else None
    res = rn(spec.B, spec.cout, *ext) if spec.r else None
    up = rn(spec.B, 1, ext[-2] // 2, ext[-1] // 2) if spec.u else None
    bc = (None, slice(None)) + (None,) * spec.nd
    full = F.gelu(torch.stack([_full_ref(xb, w, spec) for xb in x]) * scale[bc] + shift[bc])
    if spec.m:
        full = full * (mul.unsqueeze(2) if spec.nd == 3 else mul)
    if spec.r:
        full = full + res
    upf = F.interpolate(up, scale_factor=2, mode="bilinear", align_corners=False) if spec.u else None
    if spec.u:
        full = full + upf
    for b, lo, hi in windows(spec, (3, 5, 12) if spec.nd == 3 else (8, 24)):
        got = window_expect(list(torch.split(x[b], list(spec.cins), 0)), w, spec, lo, hi, scale, shift, F.gelu,
                            mul_b=mul[b] if spec.m else None, res_b=res[b] if spec.r else None,
                            up_b=upf[b] if spec.u else None)
        ref = full[(b, slice(None)) + tuple(slice(a, e) for a, e in zip(lo, hi))]
        assert float((got - ref).abs().max()) <= 1e-12, (key, b, lo, hi)


def test_windows_cover_corners_items_and_ragged_strip():
    s = parse_key("2d k3s1p1 32->32 B32 1x190x622 sh1")
    w = windows(s)
    assert sorted({b for b, _, _ in w}) == [0, 16, 31] and len(w) == 12
    los = {lo for _, lo, _ in w}
    assert {(0, 0), (190 - 24, 622 - 80), (0, 622 - 80)} <= los
    assert all(0 <= a and b <= e and b - a == n for _, lo, hi in w for a, b, e, n in zip(lo, hi, (190, 622), (24, 80)))
    inner = [lo for lo in los if all(0 < a < e - n for a, e, n in zip(lo, (190, 622), (24, 80)))]
    assert len(inner) == 1 and w == windows(s)  # seeded by the key: the same on every run
    small = parse_key("3dT k4s2p1 24->16 B1 2x3x10 sh1")  # the map is smaller than the window: taken whole, once
    assert windows(small) == [(0, (0, 0, 0), (4, 6, 20))]


# ----------------------------------------------------------------------------- reachability

PLANS = {  # name: (variant, cost volume, backbone, cv_scale, B, H, W, maxdisp)
    "S-K gwc B1": ("S", "gwc", "mobilenetv2_100", 16, 1, 384, 1248, 192),
    "S-K nc B1": ("S", "nc", "mobilenetv2_100", 16, 1, 384, 1248, 192),
    "M-K B1": ("M", "gwc", "efficientnet_b2", 8, 1, 384, 1248, 192),
    "L-K gwc B1": ("L", "gwc", "efficientnet_b2", 4, 1, 384, 1248, 192),
    "L-K gwc B4": ("L", "gwc", "efficientnet_b2", 4, 4, 384, 1248, 192),
    "L-K gwc B32": ("L", "gwc", "efficientnet_b2", 4, 32, 384, 1248, 192),
    "L-K nc B1": ("L", "nc", "efficientnet_b2", 4, 1, 384, 1248, 192),
    "L SceneFlow B8": ("L", "gwc", "efficientnet_b2", 4, 8, 544, 960, 192),
    "Middlebury md256": ("L", "gwc", "efficientnet_b2", 4, 1, 1024, 1504, 256),
}

# Rows with B != 2 that no hot-path plan asks for, each decided from the code (none is stale: ESMStereo._prefix
# runs these layers through run_conv on the LEFT half of the backbone batch, so at B = 1 for a KITTI pair)
KNOWN_UNREACHED = {
    "2d k3s1p1 16->24 B1 1x192x624 sh1": "ESMStereo-S prefix: conv_f0 on the left 1/2-scale feature (model._prefix)",
    "2d k3s1p1 96->32 B1 1x24x78 sh1": "ESMStereo-S prefix: conv_f2, and semantic[0] of the norm-correlation variant",
    "2d k3s1p1 96->64 B1 1x24x78 sh1": "ESMStereo-S prefix: semantic[0] of the gwc variant (model._seq_fast)",
    "2d k3s1p1 64->32 B1 1x24x78 sh1": "ESMStereo-S prefix: semantic[1] of the gwc variant (model._seq_fast)",
}


class _Recording(dict):
    """``engine.TUNED_HINTS`` with every key it is asked for written down."""

    def __init__(self, *a):
        super().__init__(*a)
        self.asked = []

    def get(self, key, default=None):
        self.asked.append(key)
        return super().get(key, default)


def row_plans():
    """{table row: sorted names of the plans (eval or train outputs) whose emission looks it up}."""
    rec = _Recording(engine.TUNED_HINTS)
    saved, engine.TUNED_HINTS = engine.TUNED_HINTS, rec
    reached = {}
    try:
        for name, (var, cv, bb, cvs, B, H, W, md) in PLANS.items():
            with contextlib.redirect_stdout(io.StringIO()):  # (the constructor names its cost volume)
                m = E.ESMStereo(md, cv == "gwc", cv == "nc", bb, cvs, feature_cls=StubFeature)
            m.load_state_dict(seeded_state(load_spec(f"spec_{var}_{cv}.json"), 1))
            m.eval()
            ups = [(B, c, H // s, W // s) for c, s in UP_LAYOUT[cvs]]
            att = 0 if cvs != 16 else (32 if cv == "gwc" else 8)
            for train in (False, True):
                meta = plan_ops(m, B, H // cvs, W // cvs, att, ups, train)
                assert meta and rec.asked, name
                # what a plain conv launch reports is what the lookup gave it
                for op in meta:
                    if op["kind"] == "conv" and op.get("key") in TABLE and not op["name"].endswith("[side]"):
                        assert op["hint"] & ~engine.HINT_XCD_SLAB == TABLE[op["key"]], (name, op["name"])
                for k in rec.asked:
                    if k in TABLE:
                        reached.setdefault(k, set()).add(name)
                rec.asked.clear()
    finally:
        engine.TUNED_HINTS = saved
    return {k: sorted(v) for k, v in reached.items()}


def test_every_row_is_reached_by_a_plan():
    reached = row_plans()
    print("row -> plans that look it up")
    for k in sorted(TABLE):
        print(f"  {k}: {', '.join(reached.get(k, [])) or KNOWN_UNREACHED.get(k, '-')}")
    loose = [k for k in TABLE if parse_key(k).B != 2 and k not in reached and k not in KNOWN_UNREACHED]
    assert not loose, f"rows no plan looks up (stale, or to be listed with a reason): {loose}"
    assert not [k for k in KNOWN_UNREACHED if k in reached or k not in TABLE], "KNOWN_UNREACHED lists a reached / deleted row"
    # the headline batch: every B32 row belongs to the L-K B = 32 plan
    assert all(reached[k] == ["L-K gwc B32"] for k in TABLE if parse_key(k).B == 32)


def test_dry_emission_keys_carry_the_epilogue_flags():
    """A dry emission's shape-only tensors have no address; its keys must still name the epilogue operands, or
    the dry plan looks up another row than the real one (the refinement heads' bilinear add: flag u)."""
    var, cv, bb, cvs, B, H, W, md = PLANS["S-K gwc B1"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = E.ESMStereo(md, True, False, bb, cvs, feature_cls=StubFeature)
    m.load_state_dict(seeded_state(load_spec("spec_S_gwc.json"), 1))
    m.eval()
    ups = [(B, c, H // s, W // s) for c, s in UP_LAYOUT[cvs]]
    keys = {op["name"]: op["key"] for op in plan_ops(m, B, H // cvs, W // cvs, 32, ups) if op["kind"] == "conv"}
    assert keys["upsample_module.ref2x.conv1_up"] == "2dT k4s2p1 16->1 B1 1x48x156 sh1u"
    keys = {op["name"]: op["key"] for op in plan_ops(m, B, H // cvs, W // cvs, 32, ups, True) if op["kind"] == "conv"}
    assert parse_key(keys["upsample_module.ref2x.conv1_up"]).u
