"""Every export of include/esmstereo_amd.h that takes a stream is replayed from a graph on a side stream by
tests/test_gpu_graph_replay.py, or is named there with the reason it is not.  A new export without an entry fails here,
on a machine without a GPU."""
import os
import re

import test_gpu_graph_replay as T

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "esmstereo_amd.h")


def stream_exports():
    with open(HEADER) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    decls = re.findall(r"\b(esm_\w+)\s*\(([^;{}()]*)\)\s*;", text)
    return {name for name, params in decls if re.search(r"\bvoid\s*\*\s*stream\b", params)}


def test_the_header_is_read():
    names = stream_exports()
    assert len(names) >= 38 and {"esm_conv_f32", "esm_jpeg_encode_rgb8", "esm_plan_run_op", "esm_lds_fill_u32"} <= names


def test_every_stream_export_is_replayed_or_listed():
    names = stream_exports()
    missing = sorted(names - T.REPLAYED - set(T.ELSEWHERE))
    assert not missing, f"exports with a stream and no graph-replay case or reason: {missing}"
    assert not T.REPLAYED & set(T.ELSEWHERE)
    stale = sorted((T.REPLAYED | set(T.ELSEWHERE)) - names)
    assert not stale, f"entries that name no stream-taking export of the header: {stale}"


def test_listed_reasons_are_the_two_kinds():
    for name, why in T.ELSEWHERE.items():
        assert why == "debug only" or why.startswith("replayed inside a graph already by tests/"), (name, why)
        if why == "debug only":
            assert name.startswith("esm_lds_")
        else:  # the test it names exists
            path, test = why.split(" by ", 1)[1].split("::")
            with open(os.path.join(os.path.dirname(HEADER), os.pardir, path)) as f:
                assert f"def {test}(" in f.read(), why
