"""Build the gfx950 shared library ``esmstereo_amd/libesmstereo_amd.so`` in-tree.

``python esmstereo_amd/build.py`` (or ``__graft_entry__.build()``) compiles every
``csrc/*.hip`` with ``hipcc --offload-arch=gfx950`` into objects (in parallel, skipping
up-to-date ones) and links one C-ABI shared library.  No torch headers are involved: the
library's interface is ``include/esmstereo_amd.h``.
"""
from __future__ import annotations

import concurrent.futures as cf
import json
import os
import re
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
BUILD = os.path.join(PKG, "_build")
LIB = os.path.join(PKG, "libesmstereo_amd.so")
HEADER = os.path.join(ROOT, "include", "esmstereo_amd.h")
ARCH = os.environ.get("ESM_OFFLOAD_ARCH", "gfx950")
CXXFLAGS = ["-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-result"]


def _hipcc() -> str:
    h = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(h):
        raise RuntimeError("hipcc not found: the esmstereo_amd HIP library cannot be built")
    return h


def _deps():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [HEADER]


# diagnostic build (per-wave timeline stamps in the direct conv kernels): separate objects and
# library, loaded only when ESM_LIB points at it; never used for results
DIAG_BUILD = os.path.join(PKG, "_build_diag")
DIAG_LIB = os.path.join(DIAG_BUILD, "libesmstereo_amd.so")


def _stale(obj: str, src: str) -> bool:
    if not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(p) > t for p in [src] + _deps())


# kernels whose results must be bit-exact with the reference's separately rounded ops
NO_CONTRACT = {"volumes.hip", "regression.hip"}


# Kernels allowed to use scratch (private) memory, bytes per lane: the direct conv's 2-D 5x5 forms and a few
# of its 3-D forms (measured with them; none is on the S-K chain's hot forms).  Any other kernel that spills
# or keeps a dynamically indexed array in scratch fails the build: the round-4 conv pair did, at 650-980
# bytes per lane, through a lambda over the staging array, and lost ~25 % of the S-K step before it was seen.
SCRATCH_OK = {
    "_ZN3esm4conv12dconv_kernelILb0ELi5ELi1ELb0ELi2ELi2ELi1ELi4ELb1EEEv13esm_conv_desc": 204,
    "_ZN3esm4conv12dconv_kernelILb0ELi5ELi1ELb0ELi2ELi2ELi1ELi4ELb0EEEv13esm_conv_desc": 200,
    "_ZN3esm4conv12dconv_kernelILb1ELi1ELi1ELb0ELi2ELi2ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb1ELi3ELi1ELb0ELi1ELi1ELi4ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb1ELi3ELi1ELb0ELi1ELi2ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb1ELi3ELi2ELb0ELi1ELi1ELi4ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb1ELi3ELi2ELb0ELi1ELi1ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    # 2-D multi-source direct forms: 5 dwords spilled since the GELU's hardware exp2 (round 5) changed their
    # schedule; on neither hot chain (the lean / wide / tiled forms run there)
    "_ZN3esm4conv12dconv_kernelILb0ELi1ELi1ELb0ELi1ELi1ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb0ELi1ELi1ELb0ELi2ELi1ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb0ELi3ELi1ELb0ELi1ELi1ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb0ELi3ELi2ELb0ELi1ELi1ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb1ELi1ELi1ELb0ELi1ELi2ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb0ELi3ELi1ELb0ELi1ELi1ELi4ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb0ELi3ELi2ELb0ELi1ELi1ELi4ELi4ELb1EEEv13esm_conv_desc": 20,
    # their two-N-tile twins: the same 5 dwords since the one-branch GELU (round 10) changed the schedule again
    "_ZN3esm4conv12dconv_kernelILb0ELi3ELi1ELb0ELi1ELi2ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
    "_ZN3esm4conv12dconv_kernelILb0ELi3ELi2ELb0ELi1ELi2ELi1ELi4ELb1EEEv13esm_conv_desc": 20,
}


def kernel_resources(stderr: str) -> dict:
    """{mangled kernel: {"vgpr": n, "scratch": bytes per lane}} from hipcc's kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and cur is not None:
            cur["vgpr" if m.group(1) == "VGPRs" else "scratch"] = int(m.group(2))
    return out


def _compile(src: str, obj: str, defines=()) -> str:
    extra = ["-ffp-contract=off"] if os.path.basename(src) in NO_CONTRACT else []
    extra += [f"-D{d}" for d in defines]
    cmd = [_hipcc()] + CXXFLAGS + extra + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {os.path.basename(src)}:\n{r.stderr}")
    res = kernel_resources(r.stderr)
    with open(obj + ".res.json", "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    bad = {k: v["scratch"] for k, v in res.items() if v.get("scratch", 0) > SCRATCH_OK.get(k, 0)}
    if bad and not defines:  # (the diagnostic build's stamps may spill)
        os.remove(obj)  # rebuilt (and re-checked) next time
        raise RuntimeError(f"{os.path.basename(src)}: kernels using scratch memory (bytes per lane): {bad}")
    return obj


def build(verbose: bool = False, jobs: int = 8, diag: bool = False) -> str:
    bdir, lib_path = (DIAG_BUILD, DIAG_LIB) if diag else (BUILD, LIB)
    defines = ("ESM_CONV_STAMPS",) if diag else ()
    os.makedirs(bdir, exist_ok=True)
    srcs = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    objs = []
    todo = []
    for f in srcs:
        src = os.path.join(CSRC, f)
        obj = os.path.join(bdir, f[:-4] + ".o")
        objs.append(obj)
        if _stale(obj, src):
            todo.append((src, obj))
    if todo:
        with cf.ThreadPoolExecutor(max_workers=max(1, min(jobs, len(todo)))) as ex:
            for fut in [ex.submit(_compile, s, o, defines) for s, o in todo]:
                o = fut.result()
                if verbose:
                    print("compiled", os.path.relpath(o, ROOT))
    if todo or not os.path.exists(lib_path) or any(os.path.getmtime(o) > os.path.getmtime(lib_path) for o in objs):
        tmp = lib_path + ".tmp"
        cmd = [_hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr}")
        os.replace(tmp, lib_path)
        if verbose:
            print("linked", os.path.relpath(lib_path, ROOT))
    return lib_path


if __name__ == "__main__":
    build(verbose=True, diag="--diag" in sys.argv)
    sys.exit(0)
