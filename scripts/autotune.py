"""Pick each conv's tile form by measuring it inside the hot path's own launch sequence.

    ESM_NO_TUNED=1 python scripts/autotune.py [--variants S] [--out esmstereo_amd/tuned_hints.json]

For every conv op of the compiled hot path (bench.py's model and synthetic input), each tile
hint the library accepts is forced on that op alone (esm_plan_set_conv_hint), the plan is
replayed as a hipGraph with a hipEvent probe around the op, and the median duration is
recorded.  Ops are tuned in launch order and keep their best hint, so each op is measured
behind the already-chosen producers (the cache state it will run in).  A hint replaces the
automatic choice only when it is faster by more than `--margin`.  The table is keyed by
engine.conv_key (geometry, channel split, batch, extent, epilogue), merged into --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

os.environ.setdefault("ESM_AB", "1")  # the package reads A/B knobs only with ESM_AB=1
os.environ.setdefault("ESM_NO_TUNED", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import esmstereo_amd as E  # noqa: E402
from esmstereo_amd._lib import (HINT_C1, HINT_C1IN, HINT_C1T, HINT_DIRECT, HINT_KS_SHIFT, HINT_NO_STEM,  # noqa: E402
                                HINT_NO_TILE, HINT_ROWS, HINT_ROWS_FORM, HINT_RPW_SHIFT, HINT_SMALL, HINT_SMALL_W8,
                                HINT_STEM, HINT_TILE, HINT_TILE_WLDS, HINT_WIDE, HINT_WIDE3, HINT_WIDE_KS2, HINT_WIDET,
                                check, lib)


def _tile(nt: int, ks: int, extra: int = 0, rpw: int = 0) -> int:
    """The general form's explicit tile: N tiles, K split, | C1 / DIRECT, DIRECT's rows per wave."""
    return nt | ks << HINT_KS_SHIFT | extra | rpw << HINT_RPW_SHIFT


# 0 = automatic; the fields are the header's (include/esmstereo_amd.h, the table above esm_conv_desc)
CANDIDATES = (
    [0] + [_tile(nt, ks) for ks in (1, 4) for nt in ((1, 2, 4) if ks == 1 else (1, 2))]        # LDS-staged
    + [_tile(nt, ks, HINT_DIRECT) for ks in (1, 4) for nt in (1, 2)]                            # direct
    + [_tile(1, 1, HINT_DIRECT, r) for r in (1, 2, 4)] + [_tile(2, 1, HINT_DIRECT, r) for r in (1, 2)]
    + [HINT_ROWS_FORM, _tile(4, 1, HINT_C1), HINT_C1T, HINT_STEM, HINT_NO_STEM, HINT_C1IN, HINT_SMALL, HINT_WIDE,
       HINT_WIDE3, HINT_WIDET]
    + [HINT_WIDE | HINT_ROWS(r) for r in (1, 2, 3)] + [HINT_WIDET | HINT_ROWS(r) for r in (1, 2)]
    + [HINT_WIDE | HINT_ROWS(r) | HINT_WIDE_KS2 for r in (0, 2, 3)] + [HINT_SMALL | HINT_SMALL_W8]
    # round 4: the LDS-tiled form (rows per wave automatic / 1 / 2 / 4) and the rules without it
    + [HINT_TILE | HINT_ROWS(r) for r in range(4)] + [HINT_NO_TILE]
    # round 6: the LDS-tiled form's LDS-staged weights / padded MT (A/B of the register forms)
    + [HINT_TILE | HINT_ROWS(r) | HINT_TILE_WLDS for r in range(4)])


def op_time(hp, i: int, reps: int) -> float:
    hp.set_probe(i, reps + 2)
    for _ in range(reps + 2):
        hp.launch()
    torch.cuda.synchronize()
    t = sorted(hp.probe_read()[2:])
    return t[len(t) // 2] * 1e3


def step_time(hp, reps: int = 50) -> float:
    hp.set_probe(-1, 1)
    for _ in range(5):
        hp.launch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        hp.launch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def tune_variant(variant: str, dev, reps: int, margin: float) -> dict:
    backbone, cvs = bench.VARIANTS[variant]
    model = E.ESMStereo(192, True, False, backbone, cvs)
    bench.seeded_init(model, 1234)
    model = model.eval().to(dev)
    left, right = bench.synthetic_pair(1, 384, 1248, 192, 100, dev)
    with torch.no_grad():
        ml, mr, att, up = model.prefix(left, right)
    B, C, h, w = (int(v) for v in ml.shape)
    hp = E.HotPath(model, B, h, w, 0 if att is None else int(att.shape[1]), [tuple(u.shape) for u in up], dev,
                   channels=C)
    hp.load_inputs(ml, mr, att, up)
    plan = hp.ctx.plan
    meta = hp.ctx.meta
    base_step = step_time(hp)
    rows = []
    chosen = {}
    for i, m in enumerate(meta):
        if m["kind"] != "conv":
            continue
        res = {}
        for h in CANDIDATES:
            if check(lib.esm_plan_set_conv_hint(plan, i, h), "set_conv_hint") < 0:
                continue
            hp._graph_ready = False
            try:
                res[h] = op_time(hp, i, reps)
            except E.EsmError:
                res[h] = None
        ok = {h: t for h, t in res.items() if t is not None}
        best = min(ok, key=ok.get)
        if best != 0 and ok[best] > ok[0] * (1 - margin):
            best = 0
        lib.esm_plan_set_conv_hint(plan, i, best)
        hp._graph_ready = False
        chosen[m["key"]] = best
        rows.append({"op": m["name"], "key": m["key"], "auto_us": round(ok[0], 2), "best": hex(best),
                     "best_us": round(ok[best], 2), "all": {hex(h): (None if t is None else round(t, 2))
                                                           for h, t in res.items()}})
        print(f"{variant} {m['name'][:44]:44s} auto {ok[0]:7.2f}  best {hex(best):>8s} {ok[best]:7.2f}", flush=True)
    tuned_step = step_time(hp)
    print(f"{variant}: step {base_step:.1f} us (automatic) -> {tuned_step:.1f} us (tuned)", flush=True)
    hp.close()
    return {"variant": variant, "step_auto_us": round(base_step, 1), "step_tuned_us": round(tuned_step, 1),
            "ops": rows, "hints": {k: v for k, v in chosen.items() if v}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", default="S")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--margin", type=float, default=0.03)
    ap.add_argument("--out", default=os.path.join(ROOT, "esmstereo_amd", "tuned_hints.json"))
    ap.add_argument("--report", default=os.path.join(ROOT, "gpurun_out", "autotune_report.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    reports = [tune_variant(v, dev, args.reps, args.margin) for v in args.variants.split(",")]
    table = {"hints": {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            table = json.load(f)
    for r in reports:
        for op in r["ops"]:  # a key whose best is now the automatic choice drops its old hint
            if op["best"] == "0x0":
                table["hints"].pop(op["key"], None)
        table["hints"].update(r["hints"])
    table["source"] = ("scripts/autotune.py on " + torch.cuda.get_device_name(0) + ": " +
                       ", ".join(f"{r['variant']} {r['step_auto_us']}->{r['step_tuned_us']} us/step" for r in reports))
    os.makedirs(os.path.dirname(args.report), exist_ok=True)
    with open(args.report, "w") as f:
        json.dump(reports, f, indent=1)
    with open(args.out, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
