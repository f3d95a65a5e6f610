"""The point cloud op (csrc/cloud.hip, esm_plan_add_cloud) on the GPU against tests/cloud_ref.py: bitwise equality of
``counts`` and of the first ``counts[b]`` records of every slot; the slots are pre-filled with 0xFF and every byte
behind the last record stays 0xFF.  Shapes sit on the tile size T = esm_cloud_tile_points() and on the scan's rounds of
256 tiles; the op is run eagerly, behind poisoned LDS, on strided crops, and replayed from graphs on a side stream."""
import ctypes
import math

import numpy as np
import pytest
import torch

import cloud_ref as R
import graph_replay
import layouts as LY
import lds_poison
from esmstereo_amd import _lib, cloud
from esmstereo_amd.node import StereoNode

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a ROCm GPU")]

lib = _lib.lib
T = lib.esm_cloud_tile_points()
DEV = "cuda"
CAM = dict(num=float(np.float32(721.5377 * 0.54)), fx=721.5377, fy=707.0912, cx=30.25, cy=11.75)
SPECIALS = (0.0, -1.0, math.nan, math.inf)


def disparities(B, H, W, seed, special=0.25):
    """fp32 [B, H, W] in [0.5, 192) with a share of 0, -1, NaN and +inf; image b + 1 has more of them than image b."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 192.0, (B, H, W)).astype(np.float32)
    for b in range(B):
        hit = rng.random((H, W)) < special * (b + 1) / B
        d[b][hit] = rng.choice(np.array(SPECIALS, dtype=np.float32), int(hit.sum()))
    return d


def colours(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


class Op:
    """One cloud op in a plan of its own, over buffers prepared as the definition allows the worst: the slots and the
    counts spoiled, the workspace arbitrary."""

    def __init__(self, disp, color=None, valid=None, step=1, z_min=0.0, z_max=math.inf, packing=R.PLY, bgr=True,
                 slot=None, out_records=None, cam=CAM):
        self.disp, self.color, self.valid = disp, color, valid
        self.B, self.H, self.W = (int(v) for v in disp.shape)
        self.step, self.rec = step, 16 if color is not None else 12
        self.bound = lib.esm_cloud_max_points(self.H, self.W, step)
        self.slot = self.bound if slot is None else slot
        self.kw = dict(z_min=z_min, z_max=z_max, step=step, bgr=bgr, packing=packing, **cam)
        nrec = self.B * self.slot if out_records is None else out_records
        self.out = torch.full((nrec * self.rec,), 0xFF, dtype=torch.uint8, device=DEV)
        self.counts = torch.full((self.B,), -7, dtype=torch.int32, device=DEV)
        nwork = lib.esm_cloud_workspace_bytes(self.B, self.H, self.W, step)
        assert nwork > 0
        self.tiles = nwork // 4 // self.B
        self.work = torch.full((nwork,), 0xA5, dtype=torch.uint8, device=DEV)
        d = self.desc = _lib.EsmCloudDesc()
        d.disp, d.disp_sb, d.disp_sh = disp.data_ptr(), disp.stride(0), disp.stride(1)
        assert disp.stride(2) == 1 or self.W == 1
        d.color = color.data_ptr() if color is not None else None
        d.valid = valid.data_ptr() if valid is not None else None
        d.out, d.slot_points, d.counts, d.work = self.out.data_ptr(), self.slot, self.counts.data_ptr(), self.work.data_ptr()
        d.B, d.H, d.W, d.step, d.bgr, d.packing = self.B, self.H, self.W, step, int(bgr), packing
        d.num, d.fx, d.fy, d.cx, d.cy = (cam[k] for k in ("num", "fx", "fy", "cx", "cy"))
        d.z_min, d.z_max = z_min, z_max
        assert lib.esm_cloud_check(ctypes.byref(d)) == self.rec, lib.esm_last_error()
        self.plan = lib.esm_plan_create()
        assert lib.esm_plan_add_cloud(self.plan, ctypes.byref(d)) == 0, lib.esm_last_error()

    def run(self):
        _lib.check(lib.esm_plan_run(self.plan, graph_replay.stream()), "plan_run")

    def reference(self, disp=None):
        """One structured array per image, from the tensors the op reads (``disp``: other values for it)."""
        d = (self.disp if disp is None else disp).cpu().numpy()
        return R.cloud_batch(d, self.kw["num"], self.kw["fx"], self.kw["fy"], self.kw["cx"], self.kw["cy"],
                             color=None if self.color is None else self.color.cpu().numpy(),
                             valid=None if self.valid is None else self.valid.cpu().numpy(),
                             **{k: self.kw[k] for k in ("z_min", "z_max", "step", "bgr", "packing")})

    def check(self, want=None, what=""):
        """counts, the records and the untouched rest of every slot (whole slots: ``out`` holds them all)."""
        torch.cuda.synchronize()
        want = self.reference() if want is None else want
        counts = self.counts.cpu().tolist()
        assert counts == [len(w) for w in want], (what, counts, [len(w) for w in want])
        out = self.out.cpu().numpy().reshape(self.B, self.slot * self.rec)
        for b, w in enumerate(want):
            n = len(w) * self.rec
            assert w.dtype.itemsize == self.rec
            if out[b, :n].tobytes() != w.tobytes():
                got = np.frombuffer(out[b, :n].tobytes(), dtype=w.dtype)
                bad = np.nonzero(got != w)[0]
                raise AssertionError(f"{what}: image {b}: {len(bad)} of {len(w)} records differ, first at {bad[:4]}: "
                                     f"{got[bad[:2]]} for {w[bad[:2]]}")
            assert bool((out[b, n:] == 0xFF).all()), f"{what}: image {b}: bytes behind record {len(w)} were written"
        return counts

    def close(self):
        lib.esm_plan_destroy(self.plan)
        self.plan = None


def run_case(d, c=None, v=None, **kw):
    """Upload, run once, compare; returns the counts."""
    op = Op(torch.from_numpy(d).to(DEV), None if c is None else torch.from_numpy(c).to(DEV),
            None if v is None else torch.from_numpy(v).to(DEV), **kw)
    try:
        op.run()
        return op.check(what=str(kw))
    finally:
        op.close()


# (H, W, step, the candidate count the case was chosen for): 1-row images, widths that are no multiple of the step
TILE_CASES = [
    (1, T - 1, 1, T - 1), (1, T, 1, T), (1, T + 1, 1, T + 1), (1, 3 * T + 5, 1, 3 * T + 5),
    (1, 2 * T + 1, 2, T + 1), (45, 177, 2, T - 1), (94, 190, 3, T), (31, 1676, 3, 3 * T + 5),
    (1, 1, 1, 1), (3, 5, 3, 2),
]


@pytest.mark.parametrize("H,W,step,cands", TILE_CASES)
def test_tile_boundaries_with_two_images(H, W, step, cands):
    assert T == 2048 and lib.esm_cloud_max_points(H, W, step) == cands and (step == 1 or W % step)
    d = disparities(2, H, W, seed=H * 31 + W)
    if cands <= 2:
        d[0], d[1] = 3.0, -1.0
    counts = run_case(d, colours(2, H, W, 1), step=step, z_min=0.01, z_max=500.0)
    assert counts[0] != counts[1] and counts[0] > 0


@pytest.mark.parametrize("what", ["zeros", "nans", "z_max", "all", "all12"])
def test_nothing_kept_and_everything_kept(what):
    H, W = 3, T + 9  # three tiles and a bit
    d = disparities(1, H, W, seed=3, special=0.0)
    kw = dict(z_max=math.inf)
    if what == "zeros":
        d[:] = 0.0
    elif what == "nans":
        d[:] = math.nan
    elif what == "z_max":
        kw = dict(z_max=float(np.float32(CAM["num"]) / np.float32(192.0)) * 0.5)  # below every Z
    counts = run_case(d, None if what == "all12" else colours(1, H, W, 2), **kw)
    assert counts == [H * W if what.startswith("all") else 0]


def test_special_values_and_a_mask_that_alone_drops_half():
    H, W = 5, 1031
    d = disparities(2, H, W, seed=9, special=0.0)
    d[0].reshape(-1)[::3] = np.resize(np.array(SPECIALS, dtype=np.float32), len(d[0].reshape(-1)[::3]))
    counts = run_case(d, colours(2, H, W, 4), z_min=0.5)  # +inf gives Z = 0 < z_min
    assert counts[1] == H * W and counts[0] == H * W - len(d[0].reshape(-1)[::3])
    v = np.zeros((2, H, W), np.uint8)
    v[0].reshape(-1)[::2] = 1
    v[1].reshape(-1)[1::2] = 200
    d = disparities(2, H, W, seed=10, special=0.0)
    assert run_case(d, colours(2, H, W, 5), v) == [(H * W + 1) // 2, H * W // 2]
    assert run_case(d, None, v.astype(bool).view(np.uint8), step=2)[0] > 0


@pytest.mark.parametrize("packing", [R.PLY, R.PCL])
@pytest.mark.parametrize("bgr", [True, False])
def test_colour_packings_and_orders(packing, bgr):
    d = disparities(2, 7, 333, seed=12)
    assert run_case(d, colours(2, 7, 333, 6), packing=packing, bgr=bgr, z_min=1.0, z_max=300.0)[0] > 0


def test_records_of_twelve_bytes():
    d = disparities(2, 7, 333, seed=13)
    assert run_case(d, None, step=2, z_min=1.0, z_max=300.0)[0] > 0


@pytest.mark.parametrize("H,W,tiles", [(1, 257 * T, 257), (513, T, 513)])
def test_more_than_one_scan_round(H, W, tiles):
    """257 tiles: a second round of one tile behind a full one; 513: two full rounds and one more."""
    d = disparities(1, H, W, seed=tiles)
    op = Op(torch.from_numpy(d).to(DEV), torch.from_numpy(colours(1, H, W, 7)).to(DEV), z_min=2.5, z_max=400.0)
    try:
        assert op.tiles == tiles
        op.run()
        assert 0 < op.check()[0] < H * W
    finally:
        op.close()


@pytest.mark.parametrize("where", LY.PLACEMENTS)
def test_disparity_as_a_strided_crop_with_poisoned_surroundings(where):
    B, H, W = 2, 9, 2 * T // 9 + 5
    d = torch.from_numpy(disparities(B, H, W, seed=21))
    c = torch.from_numpy(colours(B, H, W, 8)).to(DEV)
    flat = Op(d.to(DEV), c, step=2, z_min=1.0, z_max=300.0)
    view = LY.embed(d, where, device=DEV)  # [B, H, W] laid out as LY's [C, H, W]
    assert view.stride(2) == 1 and view.stride(1) > W and view.stride(0) > H * view.stride(1)
    snap = LY.guard_snapshot(view)
    crop = Op(view, c, step=2, z_min=1.0, z_max=300.0)
    try:
        flat.run()
        crop.run()
        want = flat.reference()
        flat.check(want)
        crop.check(want, where)
        assert torch.equal(flat.out, crop.out)
        LY.assert_guards_intact(view, snap, f"cloud disp ({where})")
    finally:
        flat.close()
        crop.close()


@pytest.mark.parametrize("color", [True, False])
def test_result_does_not_depend_on_lds_leftovers(color):
    B, H, W = 2, 3, T + 77
    op = Op(torch.from_numpy(disparities(B, H, W, seed=30)).to(DEV),
            torch.from_numpy(colours(B, H, W, 9)).to(DEV) if color else None, z_min=1.0, z_max=300.0)
    try:
        # assert_leftover_free zeroes the outputs between runs, so the plain run starts from zeros too: the rest of a
        # slot is 0 here, not 0xFF
        op.out.zero_()
        op.counts.zero_()
        lds_poison.assert_leftover_free(op.run, [op.out, op.counts], "cloud")
        want = op.reference()
        assert op.counts.cpu().tolist() == [len(w) for w in want]
        out = op.out.cpu().numpy().reshape(B, -1)
        for b, w in enumerate(want):
            assert out[b, :len(w) * op.rec].tobytes() == w.tobytes() and not out[b, len(w) * op.rec:].any()
    finally:
        op.close()


def test_two_calls_give_the_same_bytes():
    op = Op(torch.from_numpy(disparities(2, 4, 3 * T // 4 + 1, seed=40)).to(DEV),
            torch.from_numpy(colours(2, 4, 3 * T // 4 + 1, 10)).to(DEV), z_min=1.0)
    try:
        op.run()
        op.check()
        first, n = op.out.clone(), op.counts.clone()
        op.out.fill_(0xFF)
        op.counts.fill_(-7)
        op.run()
        torch.cuda.synchronize()
        assert torch.equal(op.out, first) and torch.equal(op.counts, n)
    finally:
        op.close()


def test_plan_run_replays_from_a_graph_on_a_side_stream():
    B, H, W = 2, 3, T + 100
    a = [torch.from_numpy(disparities(B, H, W, seed=50, special=0.1)), torch.from_numpy(colours(B, H, W, 11))]
    b = [torch.from_numpy(disparities(B, H, W, seed=51, special=0.6)), torch.from_numpy(colours(B, H, W, 12))]
    op = Op(a[0].to(DEV), a[1].to(DEV), z_min=1.0, z_max=300.0)
    try:
        na = [len(w) for w in op.reference(a[0])]
        nb = [len(w) for w in op.reference(b[0])]
        assert all(x != y for x, y in zip(na, nb))  # the two data sets' counts differ, image by image
        graph_replay.assert_replays(op.run, [op.disp, op.color], a, b, [op.out, op.counts], "esm_plan_run (cloud)")
    finally:
        op.close()


def test_plan_graph_launch_and_a_rebind_between_two_launches():
    B, H, W = 2, 3, T + 100
    first = torch.from_numpy(disparities(B, H, W, seed=60, special=0.1)).to(DEV)
    other = torch.from_numpy(disparities(B, H, W, seed=61, special=0.5)).to(DEV)
    op = Op(first, torch.from_numpy(colours(B, H, W, 13)).to(DEV), z_min=1.0, z_max=300.0)
    side = torch.cuda.Stream()
    sp = ctypes.c_void_p(side.cuda_stream)
    try:
        torch.cuda.synchronize()
        _lib.check(lib.esm_plan_graph_build(op.plan, sp), "plan_graph_build")
        torch.cuda.synchronize()
        assert bool((op.out == 0xFF).all()) and op.counts.cpu().tolist() == [-7] * B  # building runs nothing
        _lib.check(lib.esm_plan_graph_launch(op.plan, sp), "plan_graph_launch")
        side.synchronize()
        n_first = op.check(op.reference(first), "graph launch")
        op.out.fill_(0xFF)
        op.counts.fill_(-7)
        torch.cuda.synchronize()
        olds, size = (_lib.c_void_p * 1)(first.data_ptr()), (ctypes.c_uint64 * 1)(first.numel() * 4)
        news = (_lib.c_void_p * 1)(other.data_ptr())
        assert lib.esm_plan_rebind(op.plan, 1, olds, size, news) == 1  # disp alone lies in that range
        _lib.check(lib.esm_plan_graph_launch(op.plan, sp), "plan_graph_launch")
        side.synchronize()
        assert op.check(op.reference(other), "graph launch after rebind") != n_first
    finally:
        op.close()


def test_records_behind_four_gib_sit_where_the_64_bit_offset_says():
    """B = 2 with slots of 2^28 + 16 records of 16 bytes: image 1's first record is 2^32 + 256 bytes into ``out``.  An
    offset held in 32 bits would put it 256 bytes in, on image 0's records."""
    free, _ = torch.cuda.mem_get_info()
    if free < 6 << 30:
        pytest.skip(f"needs 6 GiB of free device memory for a 4 GiB output buffer, {free >> 20} MiB are free")
    B, H, W = 2, 8, 40
    slot = (1 << 28) + 16
    assert slot * 16 > 1 << 32
    d = disparities(B, H, W, seed=70, special=0.2)
    # `out` ends behind image 1's last possible record: nothing is written behind counts[1] records of its slot
    op = Op(torch.from_numpy(d).to(DEV), torch.from_numpy(colours(B, H, W, 14)).to(DEV), z_min=1.0, slot=slot,
            out_records=slot + H * W)
    try:
        op.run()
        torch.cuda.synchronize()
        want = op.reference()
        assert op.counts.cpu().tolist() == [len(w) for w in want] and all(len(w) * 16 > 256 for w in want)
        n0, n1 = (len(w) * 16 for w in want)
        assert op.out[:n0].cpu().numpy().tobytes() == want[0].tobytes()
        assert op.out[slot * 16:slot * 16 + n1].cpu().numpy().tobytes() == want[1].tobytes()
        words = op.out.view(torch.int64)  # every other byte is still 0xFF
        touched = 0
        for lo in range(0, words.numel(), 1 << 27):
            touched += int((words[lo:lo + (1 << 27)] != -1).sum())
        mine = int((op.out[:n0].view(torch.int64) != -1).sum()) + int(
            (op.out[slot * 16:slot * 16 + n1].view(torch.int64) != -1).sum())
        assert touched == mine
    finally:
        op.close()
        del op
        torch.cuda.empty_cache()


class _FixedMap(torch.nn.Module):
    """A model that returns one fixed map, whatever it is fed."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, left, right):
        return self.m.clone()


def test_stereo_node_process_points():
    H, W = 40, 72
    rng = np.random.default_rng(80)
    m = rng.uniform(-5.0, 80.0, (1, 64, 96)).astype(np.float32)  # the padded size of a 40 x 72 frame
    m[:, :, :20], m[:, :10, :] = -3.0, 100.0                     # a band below 0 and one above max_disp: invalid
    left, right = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    node = StereoNode(_FixedMap(torch.from_numpy(m).to(DEV)), H, W, max_disp=64.0)
    u16_plain, _ = node.process(left, right)
    cam = cloud.Camera(721.5377, 0.54)
    for kw in (dict(), dict(step=2, z_min=6.0, z_max=60.0, packing="pcl", order="rgb")):
        u16, pts, ms = node.process_points(left, right, cam, **kw)
        assert np.array_equal(u16, u16_plain) and ms > 0
        filtered, frame = node.filtered.cpu().numpy(), node.dev_u8[0].cpu().numpy()
        assert np.array_equal(frame, left) and (filtered == 0).any() and (filtered > 0).any()
        want = R.cloud(filtered, *cam.values(H, W), z_min=kw.get("z_min", 0.0), z_max=kw.get("z_max", math.inf),
                       step=kw.get("step", 1), color=frame, bgr=kw.get("order", "bgr") == "bgr",
                       packing=R.PCL if kw.get("packing") == "pcl" else R.PLY)
        assert pts.dtype == want.dtype and 0 < len(want) < H * W and pts.tobytes() == want.tobytes()
    # a moved input goes through the same builder: the convenience call on a fresh tensor, twice
    d = torch.from_numpy(disparities(1, H, W, seed=81)).to(DEV)
    for t in (d, d.clone()):
        got = cloud.disparity_to_points(t, cam, z_min=1.0)
        want = R.cloud(t[0].cpu().numpy(), *cam.values(H, W), z_min=1.0)
        assert len(got) == 1 and got[0].tobytes() == want.tobytes()
    builder = list(cloud._builders.values())[-1]
    assert (builder.H, builder.W, builder.color) == (H, W, False) and len(builder._plans) == 1  # rebound, not rebuilt


@pytest.mark.parametrize("B", [2, 1])
def test_one_builder_on_a_crop_then_on_a_contiguous_map_of_the_same_shape(B):
    """The plan holds the strides of ``disp``: a builder that saw a crop of a padded allocation must not address a
    contiguous map of the same shape with the crop's strides (wrong points, and reads past the map's end), nor the
    other way round.  Every layout is compared with the reference; the crop's surroundings are poison."""
    H, W = 9, 2 * T // 9 + 5
    cam = cloud.Camera(CAM["fx"], 0.54, fy=CAM["fy"], cx=CAM["cx"], cy=CAM["cy"])
    builder = cloud.CloudBuilder(B, H, W, 1, False, DEV)
    layouts = []
    for seed, where in ((90, "odd"), (91, None), (92, "gapped16"), (93, None), (90, "odd")):
        d = torch.from_numpy(disparities(B, H, W, seed=seed))
        t = d.to(DEV) if where is None else LY.embed(d, where, device=DEV)
        assert t.is_contiguous() == (where is None)
        got = builder.build(t, cam, z_min=1.0, z_max=300.0)
        want = R.cloud_batch(d.numpy(), *cam.values(H, W), z_min=1.0, z_max=300.0)
        assert [len(g) for g in got] == [len(w) for w in want] and min(len(w) for w in want) > 0, where
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), where
        layouts.append((t.stride(0) if B > 1 else 0, t.stride(1)))
    assert len(builder._plans) == len(set(layouts)) == 3  # one plan per layout, found again when the layout returns
    # a single row or a single image: the stride that addresses nothing does not split plans
    row = cloud.CloudBuilder(1, 1, T + 3, 1, False, DEV)
    d = torch.from_numpy(disparities(1, 1, T + 3, seed=94))
    for t in (d.to(DEV), LY.embed(d, "odd", device=DEV)):
        got = row.build(t, cam, z_min=1.0)
        assert got[0].tobytes() == R.cloud(d[0].numpy(), *cam.values(1, T + 3), z_min=1.0).tobytes()
    assert len(row._plans) == 1
