"""CPU tests of the point cloud op (esm_cloud_desc, esmstereo_amd/cloud.py): the numpy reference against an fp64
evaluation and a hand-written example, every argument error of the descriptor through esm_cloud_check and
esm_plan_add_cloud, the size queries, the PLY writer, and the refusals of the Python entry points."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cloud_ref as R
from esmstereo_amd import _lib, cloud, node

lib = _lib.lib
T = lib.esm_cloud_tile_points()


# ---- the reference itself ----
def test_reference_against_fp64_on_normal_range_inputs():
    """Z takes one fp32 rounding, X and Y four (the subtraction, the product with the rounded Z, which carries Z's
    own, and the division): (1 + 2^-24)^4 - 1 < 5 * 2^-24 relative to the exact value.  Inputs and camera are fp32
    values, so the fp64 evaluation starts from the same numbers; cx, cy are half-integers away from every pixel, so no
    difference cancels."""
    rng = np.random.default_rng(5)
    H, W = 37, 53
    d = rng.uniform(0.5, 192.0, (H, W)).astype(np.float32)
    num, fx, fy, cx, cy = (np.float32(v) for v in (721.5377 * 0.54, 721.5377, 700.25, 25.5, 17.5))
    got = R.cloud(d, num, fx, fy, cx, cy)
    assert len(got) == H * W
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    Z = np.float64(num) / d.astype(np.float64)
    X = (x - np.float64(cx)) * Z / np.float64(fx)
    Y = (y - np.float64(cy)) * Z / np.float64(fy)
    bound = 5 * 2.0 ** -24
    for name, want in (("x", X), ("y", Y), ("z", Z)):
        err = np.abs(got[name].astype(np.float64) - want.ravel()) / np.abs(want.ravel())
        assert err.max() <= bound, (name, err.max(), bound)


def test_reference_order_and_counts_on_a_hand_written_example():
    # 3 x 4, num = 8, fx = fy = 2, cx = cy = 1: Z = 8 / d, X = (x - 1) * Z / 2, Y = (y - 1) * Z / 2
    d = np.array([[1.0, 0.0, 2.0, -1.0],
                  [4.0, np.nan, 8.0, 16.0],
                  [np.inf, 2.0, 0.5, 1.0]], dtype=np.float32)
    color = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    got = R.cloud(d, 8, 2, 2, 1, 1, z_min=1.0, z_max=8.0, color=color, bgr=True)
    # kept (y, x): (0,0) Z 8; (0,2) Z 4; (1,0) Z 2; (1,2) Z 1; (2,1) Z 4; (2,3) Z 8.  (1,3) Z 0.5 < z_min, (2,2) Z 16 >
    # z_max, (2,0) Z 0, d <= 0 and NaN dropped
    assert got["z"].tolist() == [8.0, 4.0, 2.0, 1.0, 4.0, 8.0]
    assert got["x"].tolist() == [-4.0, 2.0, -1.0, 0.5, 0.0, 8.0]
    assert got["y"].tolist() == [-4.0, -2.0, 0.0, 0.0, 2.0, 4.0]
    pix = [0, 2, 4, 6, 9, 11]
    assert got["blue"].tolist() == [3 * p for p in pix] and got["red"].tolist() == [3 * p + 2 for p in pix]
    assert set(got["alpha"].tolist()) == {255}
    rgb = R.cloud(d, 8, 2, 2, 1, 1, z_min=1.0, z_max=8.0, color=color, bgr=False, packing=R.PCL)["rgb"]
    assert rgb.tolist() == [(3 * p) << 16 | (3 * p + 1) << 8 | (3 * p + 2) for p in pix]
    assert got.tobytes()[12:16] == bytes([2, 1, 0, 255]) and rgb[:1].tobytes() == bytes([2, 1, 0, 0])
    valid = np.zeros((3, 4), np.uint8)
    valid[:, 2:] = 7
    assert R.cloud(d, 8, 2, 2, 1, 1, z_min=1.0, z_max=8.0, valid=valid)["z"].tolist() == [4.0, 1.0, 8.0]
    # step 2 takes rows 0, 2 and columns 0, 2 only
    assert R.cloud(d, 8, 2, 2, 1, 1, step=2)["z"].tolist() == [8.0, 4.0, 0.0, 16.0]
    assert R.max_points(3, 4, 2) == 4 and R.record_dtype(False).itemsize == 12 and R.record_dtype(True).itemsize == 16


# ---- the descriptor's argument errors ----
def good_desc(**kw):
    """A descriptor esm_cloud_check accepts; its pointers are never followed."""
    d = _lib.EsmCloudDesc()
    d.disp, d.disp_sb, d.disp_sh = 0x10000, 40 * 72, 72
    d.color, d.valid = 0x20001, 0x30003  # byte arrays: any alignment
    d.out, d.slot_points, d.counts, d.work = 0x40000, 40 * 72, 0x50004, 0x60004
    d.B, d.H, d.W, d.step, d.bgr, d.packing = 2, 40, 72, 1, 1, 0
    d.num, d.fx, d.fy, d.cx, d.cy, d.z_min, d.z_max = 389.0, 721.0, 721.0, 35.5, 19.5, 0.0, math.inf
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD = [
    ("null", dict(disp=None)), ("null", dict(out=None)), ("null", dict(counts=None)), ("null", dict(work=None)),
    ("aligned", dict(disp=0x10002)), ("aligned", dict(out=0x40008)), ("aligned", dict(counts=0x50002)),
    ("aligned", dict(work=0x60001)),
    ("positive", dict(B=0)), ("positive", dict(H=0)), ("positive", dict(W=-3)), ("positive", dict(step=0)),
    ("positive", dict(step=-1)),
    ("stride", dict(disp_sb=-1)), ("stride", dict(disp_sh=-72)),
    ("65535", dict(B=65536)),
    ("2^31", dict(H=1 << 16, W=1 << 15, slot_points=1 << 31)),
    ("slot_points", dict(slot_points=40 * 72 - 1)), ("slot_points", dict(step=2, slot_points=20 * 36 - 1)),
    ("2^40", dict(slot_points=(1 << 40) // 32)), ("2^40", dict(color=None, slot_points=-(-(1 << 40) // 24))),
    ("packing", dict(packing=2)), ("packing", dict(packing=-1)),
    ("fx", dict(fx=0.0)), ("fx", dict(fx=math.inf)), ("fy", dict(fy=math.nan)), ("fy", dict(fy=-0.0)),
    ("z_min", dict(z_min=2.0, z_max=1.0)), ("z_min", dict(z_min=math.nan)), ("z_min", dict(z_max=math.nan)),
]


@pytest.mark.parametrize("word,change", BAD, ids=[f"{w}-{'-'.join(c)}-{i}" for i, (w, c) in enumerate(BAD)])
def test_descriptor_errors_are_refused_before_any_device_call(word, change):
    d = good_desc(**change)
    assert lib.esm_cloud_check(ctypes.byref(d)) == -1
    assert word.encode() in lib.esm_last_error(), lib.esm_last_error()
    plan = lib.esm_plan_create()
    try:
        assert lib.esm_plan_add_cloud(plan, ctypes.byref(d)) == -1
        assert word.encode() in lib.esm_last_error(), lib.esm_last_error()
        assert lib.esm_plan_num_ops(plan) == 0
    finally:
        lib.esm_plan_destroy(plan)


def test_accepted_descriptors_and_the_plan_op_kind():
    assert lib.esm_cloud_check(None) == -1 and b"null" in lib.esm_last_error()
    plan = lib.esm_plan_create()
    try:
        assert lib.esm_plan_add_cloud(plan, None) == -1 and lib.esm_plan_num_ops(plan) == 0
        assert lib.esm_plan_add_cloud(None, ctypes.byref(good_desc())) == -1
        cases = [(dict(), 16), (dict(color=None), 12), (dict(valid=None, packing=1, bgr=0), 16),
                 (dict(step=3, slot_points=14 * 24), 16), (dict(z_min=5.0, z_max=5.0), 16),
                 (dict(slot_points=(1 << 40) // 32 - 1), 16),                    # the largest B * slot * 16 < 2^40
                 (dict(color=None, slot_points=-(-(1 << 40) // 24) - 1), 12),
                 (dict(B=65535, slot_points=40 * 72), 16), (dict(disp_sb=0, disp_sh=0), 16)]
        for i, (change, rec) in enumerate(cases):
            d = good_desc(**change)
            assert lib.esm_cloud_check(ctypes.byref(d)) == rec, (change, lib.esm_last_error())
            assert lib.esm_plan_add_cloud(plan, ctypes.byref(d)) == i
            assert lib.esm_plan_num_ops(plan) == i + 1 and lib.esm_plan_op_kind(plan, i) == 16
        # a refusal in between leaves the plan as it was
        assert lib.esm_plan_add_cloud(plan, ctypes.byref(good_desc(packing=9))) == -1
        assert lib.esm_plan_num_ops(plan) == len(cases)
        # a rebind moves the six pointers of an op and nothing else
        n = 6
        olds = (_lib.c_void_p * n)(0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000)
        size = (ctypes.c_uint64 * n)(*[0x1000] * n)
        news = (_lib.c_void_p * n)(*[0x100000 * (k + 1) for k in range(n)])
        want = sum(6 - (c.get("color", 1) is None) - (c.get("valid", 1) is None) for c, _ in cases)
        assert lib.esm_plan_rebind(plan, n, olds, size, news) == want
        assert lib.esm_plan_rebind(plan, n, olds, size, news) == 0
    finally:
        lib.esm_plan_destroy(plan)
    assert lib.esm_struct_size(10) == ctypes.sizeof(_lib.EsmCloudDesc) == 128


def test_size_queries():
    assert T >= 256 and T % 256 == 0
    assert 2 * T * 16 + 1024 <= 163840  # two workgroups' staging of 16-byte records fit a CU's LDS
    for H, W, step in ((1, 1, 1), (3, 4, 2), (375, 1242, 1), (375, 1242, 3), (40, 72, 5), (7, 9, 100)):
        assert lib.esm_cloud_max_points(H, W, step) == R.max_points(H, W, step)
        tiles = -(-R.max_points(H, W, step) // T)
        one = lib.esm_cloud_workspace_bytes(1, H, W, step)
        assert one >= 4 * tiles and one % 4 == 0
        for B in (2, 3, 64):
            assert lib.esm_cloud_workspace_bytes(B, H, W, step) == B * one  # linear in B
    # monotone: more pixels or a finer step never need less
    prev_p = prev_w = 0
    for n in range(1, 200, 7):
        p, w = lib.esm_cloud_max_points(n, 3 * n, 2), lib.esm_cloud_workspace_bytes(2, n, 3 * n, 2)
        assert p >= prev_p and w >= prev_w
        prev_p, prev_w = p, w
    for step in range(1, 9):
        assert lib.esm_cloud_max_points(100, 300, step) >= lib.esm_cloud_max_points(100, 300, step + 1)
        assert lib.esm_cloud_workspace_bytes(1, 100, 300, step) >= lib.esm_cloud_workspace_bytes(1, 100, 300, step + 1)
    for bad in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (-1, 4, 1), (1 << 16, 1 << 15, 1)):
        assert lib.esm_cloud_max_points(*bad) == -1
        assert lib.esm_cloud_workspace_bytes(1, *bad) == -1
    assert lib.esm_cloud_workspace_bytes(0, 4, 4, 1) == -1 and lib.esm_cloud_workspace_bytes(65536, 4, 4, 1) == -1
    assert lib.esm_cloud_max_points(46340, 46340, 1) == 46340 * 46340  # H * W just below 2^31


# ---- the PLY writer ----
def read_ply(data: bytes):
    """A reader of what ply_bytes writes, and of nothing more: the header's properties -> a structured array."""
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    types = {"float": "<f4", "uchar": "u1"}
    count, fields = None, []
    for line in lines[2:]:
        w = line.split()
        if w[0] == "element":
            assert w[1] == "vertex" and count is None
            count = int(w[2])
        elif w[0] == "property":
            fields.append((w[2], types[w[1]]))
        else:
            raise AssertionError(line)
    a = np.frombuffer(body, dtype=np.dtype(fields))
    assert len(a) == count
    return a


@pytest.mark.parametrize("color", [False, True])
def test_ply_bytes_round_trip(color, tmp_path):
    rng = np.random.default_rng(2)
    d = rng.uniform(-1.0, 50.0, (9, 11)).astype(np.float32)
    c = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8) if color else None
    pts = R.cloud(d, 100.0, 50.0, 60.0, 5.0, 4.0, z_max=40.0, color=c)
    assert 0 < len(pts) < 99 and pts.dtype == cloud.point_dtype(color, "ply")
    back = read_ply(cloud.ply_bytes(pts))
    assert back.dtype.names == pts.dtype.names and back.tobytes() == pts.tobytes()
    cloud.write_ply(tmp_path / "a.ply", pts)
    assert (tmp_path / "a.ply").read_bytes() == cloud.ply_bytes(pts)
    assert len(read_ply(cloud.ply_bytes(pts[:0]))) == 0
    with pytest.raises(ValueError):
        cloud.ply_bytes(np.zeros(3, dtype=cloud.point_dtype(True, "pcl")))


def test_point_dtypes_match_the_reference():
    assert cloud.point_dtype(False) == R.XYZ and cloud.point_dtype(True, "ply") == R.XYZ_PLY
    assert cloud.point_dtype(True, "pcl") == R.XYZ_PCL
    with pytest.raises(ValueError):
        cloud.point_dtype(True, "xyz")


# ---- the Python entry points ----
def test_camera_defaults():
    cam = cloud.Camera(721.5377, 0.54)
    num, fx, fy, cx, cy = cam.values(375, 1242)
    assert (fx, fy, cx, cy) == (721.5377, 721.5377, 620.5, 187.0)
    assert num == float(np.float32(721.5377 * 0.54))
    assert cloud.Camera(700.0, 0.5, fy=710.0, cx=3.0, cy=4.0).values(10, 10)[1:] == (700.0, 710.0, 3.0, 4.0)


def test_cpu_tensors_are_refused():
    cam = cloud.Camera(100.0, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud.disparity_to_points(torch.ones(4, 6), cam)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud.CloudBuilder(1, 4, 6, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cloud.CloudBuilder.build(object.__new__(cloud.CloudBuilder), torch.ones(1, 4, 6), cam)


def test_resize_node_has_no_points():
    n = object.__new__(node.ResizeNode)  # (the constructor allocates on the device)
    frame = np.zeros((4, 6, 3), np.uint8)
    with pytest.raises(NotImplementedError):
        n.process_points(frame, frame, cloud.Camera(100.0, 0.5))
    assert node.ConfidenceNode.process_points is node.StereoNode.process_points
