"""The launch lists the hot path's size rules produce, as test input (no GPU needed).

For given input shapes the hot path compiles to one launch list.  Which list is decided by about a dozen size
rules in two layers: engine.py (``gwc_stem_supported``, ``pairk_auto``, ``pair2_auto``, ``FM2_MIN_PIX``,
``SHUFFLE_CONV_MAX_PIX``, the ``XCD_SLAB`` thresholds, ``convt_1x1_supported``, ``shuffle_conv(_pre)_supported``)
and the library's ``select_form`` (``tile3_auto``, ``tile2_auto``, ``pw_auto``, ``small_auto``, ``stem_auto``,
``c1in``).  This module walks a grid of drop-in input sizes with dry emissions (``model.plan_ops``), reduces each
launch list to its ``signature`` (per launch: name, kind and whatever tells its kernel apart) and keeps one
smallest member per distinct signature in ``CASES``:

* tests/test_shape_classes_host.py holds ``CASES`` to the grid (same set of classes), and checks that every size
  constant has a case on either side of it;
* tests/test_gpu_shape_classes.py runs every case end to end against the CPU oracle.

What a signature does not see: a conv's form is asked of ``esm_conv_form`` for the descriptor its shape key names
(``test_conv_forms_host.build_desc``: contiguous operands at arena-like addresses), so a launch whose source is a
cropped view may take another form than the one listed; and the tile sizes a launcher picks inside one form.  The
GPU cases check the numbers end to end whichever kernel ran.

``python tests/shape_classes.py`` prints the ``CASES`` literal for the current ``GRID`` and rules (paste it below
after a deliberate threshold or form change).
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import io
import os
import sys
from typing import Dict, List, Tuple

import numpy as np
import torch

if __name__ == "__main__":  # (under pytest, tests/conftest.py has done this)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import esmstereo_amd as E  # noqa: E402
from esmstereo_amd import _lib  # noqa: E402
from esmstereo_amd.backbone import StubFeature  # noqa: E402
from esmstereo_amd.model import plan_ops  # noqa: E402
from helpers import UP_LAYOUT, fullsize_inputs, load_spec, seeded_state  # noqa: E402
from oracle import esm_oracle as O  # noqa: E402
from test_conv_forms_host import build_desc  # noqa: E402
from tuned_rows import parse_key  # noqa: E402

# config: (variant, cost volume, backbone, cv_scale, attention channels)
CONFIGS: Dict[str, Tuple[str, str, str, int, int]] = {
    "S-gwc": ("S", "gwc", "mobilenetv2_100", 16, 32),
    "S-nc": ("S", "nc", "mobilenetv2_100", 16, 8),
    "M-gwc": ("M", "gwc", "efficientnet_b2", 8, 0),
    "L-gwc": ("L", "gwc", "efficientnet_b2", 4, 0),
    "L-nc": ("L", "nc", "efficientnet_b2", 4, 0),
}
WEIGHT_SEED = 15
MAXDISPS = (48, 64, 96, 128, 192, 256)
# H x W, multiples of 32 (the reference's hourglasses raise on anything else): what test_kitti.py's padding, the
# SceneFlow crops and the Middlebury / ETH3D quarter- and half-size images give
SIZES = ((64, 64), (64, 128), (96, 160), (128, 128), (128, 256), (160, 320), (192, 320), (192, 640), (256, 256),
         (256, 512), (320, 480), (384, 640), (384, 1248), (512, 960), (544, 960))
BATCHES = (1, 2, 3)
# further points, each putting one rule's quantity just below / just above its constant (see THRESHOLDS in
# tests/test_shape_classes_host.py): (config, maxdisp, B, H, W)
EXTRA = (
    ("S-gwc", 64, 1, 224, 256),    # 57,344 full-resolution pixels, against 256 x 256 = 2^16: XCD_SLAB_MIN_PIX
    ("S-gwc", 64, 1, 512, 1024),   # 256 x 512 = 2^17 half-resolution pixels x one 16-cout tile: small_auto, exactly
    ("S-gwc", 64, 1, 544, 1024),   # ... and just above
    ("S-gwc", 64, 1, 1024, 992),   # D h w = 4 x 64 x 62 = 15,872 group_stem voxels: XCD_SLAB_MIN_VOX_WIDE, just below
    ("S-gwc", 64, 1, 1024, 1024),  # ... and 2^14 exactly; 64 x 64 = 4096 low-res pixels: PAIRK_MAX_VOX, exactly
    ("S-gwc", 64, 2, 1024, 1024),  # ... and twice that
    ("M-gwc", 64, 1, 512, 512),    # D h w = 8 x 64 x 64 = 2^15 voxels; B 2 makes them 2^16 (gwc_stem_supported)
    ("M-gwc", 64, 2, 512, 512),
    ("L-gwc", 48, 1, 256, 256),    # D h w = 12 x 64 x 64, just below 2^16: gwc_stem_supported / tile3_auto
    ("L-gwc", 64, 1, 256, 256),    # ... and 16 x 64 x 64 = 2^16 exactly
    ("L-nc", 48, 1, 256, 256),
    ("L-nc", 64, 1, 256, 256),
    ("L-gwc", 64, 1, 256, 544),    # 64 x 136 = 8704 quarter-resolution pixels (256 x 512: 8192): SHUFFLE_CONV_MAX_PIX
    ("L-gwc", 64, 1, 480, 512),    # 120 x 128 = 15,360 quarter- / 61,440 half-resolution pixels, just below ...
    ("L-gwc", 64, 1, 512, 512),    # ... 2^14 (FM2_MIN_PIX) and 2^16 (pw_auto, stem_auto, c1in) exactly
    ("L-nc", 64, 1, 480, 512),
    ("L-nc", 64, 1, 512, 512),
    ("L-gwc", 64, 1, 1024, 992),   # 512 x 496 half-resolution pixels x two 16-cout tiles, just below 2^19: tile2_auto
    ("L-gwc", 64, 1, 1024, 1024),  # ... and 2^19 exactly
)


def _grid() -> List[Tuple[str, int, int, int, int]]:
    out = []
    for cfg, (_, _, _, cvs, _) in CONFIGS.items():
        for md in MAXDISPS:
            if (md // cvs) % 2 or md % cvs:  # the reference's aggregation returns 2 * ceil(D / 2) planes
                continue
            for H, W in SIZES:
                for B in BATCHES:
                    out.append((cfg, md, B, H, W))
    return out + [e for e in EXTRA if e not in out]


GRID = _grid()


@functools.lru_cache(maxsize=None)
def cpu_model(cfg: str, maxdisp: int):
    """The config's module tree on the CPU with seeded weights (a dry emission reads only their shapes)."""
    var, cv, bb, cvs, _ = CONFIGS[cfg]
    with contextlib.redirect_stdout(io.StringIO()):  # (the constructor names its cost volume)
        m = E.ESMStereo(maxdisp, cv == "gwc", cv == "nc", bb, cvs, feature_cls=StubFeature)
    m.load_state_dict(seeded_state(load_spec(f"spec_{var}_{cv}.json"), WEIGHT_SEED))
    return m.eval()


def up_shapes(cfg: str, B: int, H: int, W: int) -> List[Tuple[int, int, int, int]]:
    return [(B, c, H // s, W // s) for c, s in UP_LAYOUT[CONFIGS[cfg][3]]]


def launches(cfg: str, maxdisp: int, B: int, H: int, W: int, train: bool = True) -> List[dict]:
    """``Ctx.meta`` of the dry emission for this point (cached: read only)."""
    return _launches(cfg, maxdisp, B, H, W, bool(train))


@functools.lru_cache(maxsize=None)
def _launches(cfg: str, maxdisp: int, B: int, H: int, W: int, train: bool) -> List[dict]:
    cvs, att = CONFIGS[cfg][3], CONFIGS[cfg][4]
    return plan_ops(cpu_model(cfg, maxdisp), B, H // cvs, W // cvs, att, up_shapes(cfg, B, H, W), train)


def conv_form(key: str, hint: int) -> int:
    """The library's form for a conv launch of this shape key and hint (negative: refused)."""
    d = build_desc(parse_key(key), hint)
    return int(_lib.lib.esm_conv_form(ctypes.byref(d)))


FORM_NAMES = ("general", "stem", "c1in", "small", "wide", "wide3", "widet", "tile3", "tile2", "pw")


def entry(op: dict) -> tuple:
    """One launch of a signature: (name, kind, what tells its kernel apart...)."""
    name, kind = op["name"], op["kind"]
    slab = int(bool(op.get("hint", 0) & _lib.HINT_XCD_SLAB))
    if kind == "conv":
        f = conv_form(op["key"], op["hint"])
        return (name, kind, FORM_NAMES[f] if f >= 0 else f"refused({f})", slab)
    if kind == "conv_pair":
        return (name, kind, op["form"])
    if kind == "conv_up1":
        return (name, kind, op["form"], slab)
    if kind in ("shuffle_tail", "shuffle_conv"):
        return (name, kind, op["form"], op["slab"])
    if kind == "fmnet":
        return (name, kind, op["launches"])
    if kind == "gwc_stem":
        return (name, kind, op["form"], (op["hint"] & _lib.HINT_ROWS_MASK) >> _lib.HINT_ROWS_SHIFT, slab)
    return (name, kind)


def signature_of(meta: List[dict]) -> tuple:
    return tuple(entry(op) for op in meta)


def signature(model, B: int, H: int, W: int, maxdisp: int, train: bool = True) -> tuple:
    """The launch list ``model`` (an ESMStereo, on any device) compiles to for B x H x W images, one entry per
    launch, from a dry emission."""
    cvs = model.vol_size
    ups = [(B, c, H // s, W // s) for c, s in UP_LAYOUT[cvs]]
    att_ch = 0 if cvs != 16 else (32 if model.gwc else 8)  # ESMStereo-S: `semantic`'s channels
    saved, model.maxdisp = model.maxdisp, maxdisp
    try:
        return signature_of(plan_ops(model, B, H // cvs, W // cvs, att_ch, ups, train))
    finally:
        model.maxdisp = saved


def case_signature(cfg: str, maxdisp: int, B: int, H: int, W: int, train: bool = True) -> tuple:
    """The signature of a grid point's launch list (cached)."""
    return _case_signature(cfg, maxdisp, B, H, W, bool(train))


@functools.lru_cache(maxsize=None)
def _case_signature(cfg: str, maxdisp: int, B: int, H: int, W: int, train: bool) -> tuple:
    return signature_of(_launches(cfg, maxdisp, B, H, W, train))


def classes(points) -> Dict[tuple, Tuple[str, int, int, int, int]]:
    """{(config, signature): the member with the fewest full-resolution pixels x B, ties to the smaller maxdisp}."""
    best: Dict[tuple, Tuple[str, int, int, int, int]] = {}
    for p in points:
        cfg, md, B, H, W = p
        k = (cfg, case_signature(*p))
        rank = (B * H * W, md, B, H, W)
        q = best.get(k)
        if q is None or rank < (q[2] * q[3] * q[4], q[1], q[2], q[3], q[4]):
            best[k] = p
    return best


def case_id(case) -> str:
    cfg, md, B, H, W = case
    return f"{cfg}-md{md}-B{B}-{H}x{W}"


# ----------------------------------------------------------------------------- inputs and the L near-tie share

INPUT_SEED = 7
# L cases whose oracle cost has more than NEAR_TIE_CAP of its pixels within the flip margin at INPUT_SEED get
# another input seed here (never a wider cap): {case: seed}
SEEDS: Dict[Tuple[str, int, int, int, int], int] = {}
NEAR_TIE_CAP = 0.02  # of the low-res pixels: what check (a) of the L cases may skip


def state(cfg: str) -> Dict[str, torch.Tensor]:
    var, cv = CONFIGS[cfg][:2]
    return seeded_state(load_spec(f"spec_{var}_{cv}.json"), WEIGHT_SEED)


def case_inputs(case):
    """(match_left, match_right, att or None, [upsampler features]) of a case as float32 CPU tensors:
    helpers.fullsize_inputs (smooth texture, planar disparity, no backbone), attention with the variant's channels."""
    cfg, md, B, H, W = case
    cvs, att_ch = CONFIGS[cfg][3], CONFIGS[cfg][4]
    ml, mr, att, up = fullsize_inputs(cvs, B, H, W, md, SEEDS.get(tuple(case), INPUT_SEED), att=att_ch > 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    return t(ml), t(mr), None if att is None else t(att[:, :att_ch]), [t(u) for u in up]


def oracle_cost(case, sd=None):
    """The oracle's aggregated cost [B, 1, D, h, w] of a case (oracle.hot_path up to ``cost``, lines 700-712)."""
    cfg, md, B, H, W = case
    cvs, gwc = CONFIGS[cfg][3], CONFIGS[cfg][1] == "gwc"
    sd = sd or state(cfg)
    ml, mr, att, _ = case_inputs(case)
    D = md // cvs
    with torch.no_grad():
        if gwc:
            vol = O.gwc_volume(ml, mr, D, 32)
            if cvs == 16:
                vol = vol * att.unsqueeze(2)
            vol = O.basic_conv(sd, "group_stem.", vol, k=3, pad=1)
        else:
            vol = O.basic_conv(sd, "corr_stem.", O.normcorr_volume(ml, mr, D), k=3, pad=1)
            if cvs == 16:
                vol = vol * att.unsqueeze(2)
        return O.aggregation(sd, "aggregation_out.", O.basic_conv(sd, "agg.", vol, k=3, pad=1))


def flip_margin(cost, cost_rel_tol: float) -> float:
    """The largest oracle 2nd-minus-3rd margin at which a top-2 flip is legitimate: each of the two costs may move
    by ``cost_rel_tol`` x max |cost|."""
    return 2.0 * cost_rel_tol * float(cost.detach().abs().max())


def near_tie_share(cost, cost_rel_tol: float) -> float:
    """Share of the low-res pixels of ``cost`` [B, 1, D, h, w] (or [B, D, h, w]) whose 2nd-minus-3rd largest
    cost is within ``flip_margin``."""
    c = cost.detach().double().reshape(cost.shape[0], -1, *cost.shape[-2:])
    sv = torch.sort(c, dim=1, descending=True)[0]
    return float(((sv[:, 1] - sv[:, 2]) <= flip_margin(c, cost_rel_tol)).double().mean())


# One case per launch list of GRID: (config, maxdisp, B, H, W), as `python tests/shape_classes.py` prints them.
CASES: List[Tuple[str, int, int, int, int]] = [
    ('S-gwc', 64, 1, 64, 64),
    ('S-gwc', 64, 1, 256, 256),
    ('S-gwc', 64, 3, 128, 256),
    ('S-gwc', 64, 2, 256, 512),
    ('S-gwc', 256, 2, 256, 512),
    ('S-gwc', 64, 2, 320, 480),
    ('S-gwc', 256, 2, 320, 480),
    ('S-gwc', 64, 1, 384, 1248),
    ('S-gwc', 192, 1, 384, 1248),
    ('S-gwc', 256, 1, 384, 1248),
    ('S-gwc', 64, 1, 544, 1024),
    ('S-gwc', 96, 3, 384, 640),
    ('S-gwc', 64, 2, 384, 1248),
    ('S-gwc', 96, 2, 384, 1248),
    ('S-gwc', 64, 1, 1024, 1024),
    ('S-gwc', 64, 3, 384, 1248),
    ('S-gwc', 192, 3, 384, 1248),
    ('S-gwc', 64, 2, 1024, 1024),
    ('S-nc', 64, 1, 64, 64),
    ('S-nc', 64, 1, 256, 256),
    ('S-nc', 64, 3, 128, 256),
    ('S-nc', 64, 2, 256, 512),
    ('S-nc', 64, 2, 320, 480),
    ('S-nc', 64, 1, 384, 1248),
    ('S-nc', 192, 1, 384, 1248),
    ('S-nc', 64, 3, 384, 640),
    ('S-nc', 64, 2, 384, 1248),
    ('S-nc', 64, 3, 384, 1248),
    ('S-nc', 192, 3, 384, 1248),
    ('M-gwc', 48, 1, 64, 64),
    ('M-gwc', 48, 3, 64, 128),
    ('M-gwc', 256, 1, 128, 256),
    ('M-gwc', 48, 3, 96, 160),
    ('M-gwc', 192, 3, 96, 160),
    ('M-gwc', 48, 1, 256, 256),
    ('M-gwc', 128, 1, 256, 256),
    ('M-gwc', 48, 3, 128, 256),
    ('M-gwc', 96, 3, 128, 256),
    ('M-gwc', 256, 1, 256, 512),
    ('M-gwc', 48, 1, 320, 480),
    ('M-gwc', 64, 1, 320, 480),
    ('M-gwc', 256, 1, 320, 480),
    ('M-gwc', 48, 2, 256, 512),
    ('M-gwc', 128, 2, 256, 512),
    ('M-gwc', 48, 2, 320, 480),
    ('M-gwc', 128, 2, 320, 480),
    ('M-gwc', 48, 1, 384, 1248),
    ('M-gwc', 96, 1, 384, 1248),
    ('M-gwc', 192, 1, 384, 1248),
    ('M-gwc', 48, 3, 384, 640),
    ('M-gwc', 48, 2, 384, 1248),
    ('M-gwc', 48, 3, 384, 1248),
    ('M-gwc', 192, 3, 384, 1248),
    ('L-gwc', 48, 1, 64, 64),
    ('L-gwc', 256, 1, 64, 64),
    ('L-gwc', 256, 1, 128, 128),
    ('L-gwc', 256, 1, 128, 256),
    ('L-gwc', 48, 3, 96, 160),
    ('L-gwc', 96, 3, 96, 160),
    ('L-gwc', 192, 3, 96, 160),
    ('L-gwc', 48, 1, 256, 256),
    ('L-gwc', 64, 1, 256, 256),
    ('L-gwc', 128, 1, 256, 256),
    ('L-gwc', 48, 3, 128, 256),
    ('L-gwc', 96, 3, 128, 256),
    ('L-gwc', 256, 1, 256, 512),
    ('L-gwc', 64, 1, 256, 544),
    ('L-gwc', 48, 1, 320, 480),
    ('L-gwc', 256, 1, 320, 480),
    ('L-gwc', 48, 2, 256, 512),
    ('L-gwc', 128, 2, 256, 512),
    ('L-gwc', 256, 2, 256, 512),
    ('L-gwc', 48, 2, 320, 480),
    ('L-gwc', 128, 2, 320, 480),
    ('L-gwc', 256, 2, 320, 480),
    ('L-gwc', 48, 1, 384, 1248),
    ('L-gwc', 96, 1, 384, 1248),
    ('L-gwc', 192, 1, 384, 1248),
    ('L-gwc', 256, 1, 384, 1248),
    ('L-gwc', 48, 3, 384, 640),
    ('L-gwc', 96, 3, 384, 640),
    ('L-gwc', 48, 2, 384, 1248),
    ('L-gwc', 96, 2, 384, 1248),
    ('L-gwc', 64, 1, 1024, 1024),
    ('L-gwc', 48, 3, 384, 1248),
    ('L-gwc', 192, 3, 384, 1248),
    ('L-nc', 48, 1, 64, 64),
    ('L-nc', 256, 1, 128, 128),
    ('L-nc', 256, 1, 128, 256),
    ('L-nc', 48, 3, 96, 160),
    ('L-nc', 96, 3, 96, 160),
    ('L-nc', 192, 3, 96, 160),
    ('L-nc', 48, 1, 256, 256),
    ('L-nc', 64, 1, 256, 256),
    ('L-nc', 128, 1, 256, 256),
    ('L-nc', 48, 3, 128, 256),
    ('L-nc', 96, 3, 128, 256),
    ('L-nc', 256, 1, 256, 512),
    ('L-nc', 48, 1, 320, 480),
    ('L-nc', 64, 1, 320, 480),
    ('L-nc', 256, 1, 320, 480),
    ('L-nc', 48, 2, 256, 512),
    ('L-nc', 128, 2, 256, 512),
    ('L-nc', 256, 2, 256, 512),
    ('L-nc', 48, 2, 320, 480),
    ('L-nc', 128, 2, 320, 480),
    ('L-nc', 256, 2, 320, 480),
    ('L-nc', 48, 1, 384, 1248),
    ('L-nc', 96, 1, 384, 1248),
    ('L-nc', 192, 1, 384, 1248),
    ('L-nc', 256, 1, 384, 1248),
    ('L-nc', 48, 3, 384, 640),
    ('L-nc', 96, 3, 384, 640),
    ('L-nc', 48, 2, 384, 1248),
    ('L-nc', 96, 2, 384, 1248),
    ('L-nc', 48, 3, 384, 1248),
    ('L-nc', 192, 3, 384, 1248),
]


if __name__ == "__main__":
    best = classes(GRID)
    order = {c: i for i, c in enumerate(CONFIGS)}
    print(f"# {len(GRID)} grid points, {len(best)} launch lists")
    print("CASES: List[Tuple[str, int, int, int, int]] = [")
    for p in sorted(best.values(), key=lambda p: (order[p[0]], p[2] * p[3] * p[4], p[1], p[2], p[3], p[4])):
        print(f"    {p!r},")
    print("]")
