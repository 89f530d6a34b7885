"""Camera motion, operator level (vt_op_camera_motion: the four launches of csrc/k_camera_motion.hip alone), on the MI355X.

Every comparison is np.array_equal against the NumPy model of tests/camera_motion_util.py: thumbnails, SAD tables, records
and states, bit for bit. The hook keeps thumbnails, records and tables between guard bands (a changed guard byte is an error
of the call) and fills the tables with 0xff first: what a launch must leave alone has to come back as it went in. Frames are
about 160x96 with cell 4 and R 4 unless stated."""
import importlib

import numpy as np
import pytest

import camera_motion_util as cm

pytestmark = pytest.mark.gpu

F = np.float32
W, H, C, R = 160, 96, 4, 4
CELLS = 4096
BOX = (60.0, 40.0, 20.0, 20.0)
CANVAS = cm.texture(420, 420, seed=11)


def _states(gpu, boxes, w, h, frames_done=3):
    st = np.zeros(len(boxes), importlib.import_module(gpu.__name__ + ".snapshot").STATE)
    for i, b in enumerate(boxes):
        st[i]["box"] = b
        st[i]["frame_w"], st[i]["frame_h"] = w, h
        st[i]["frames_done"] = frames_done
        st[i]["initialized"] = 1
    return st


def views(d, w=W, h=H, c=C, canvas=CANVAS):
    """two views whose content moves by d cells from the first to the second"""
    x0, y0 = 80, 80
    return cm.view(canvas, x0, y0, w, h), cm.view(canvas, x0 - d[0] * c, y0 - d[1] * c, w, h)


class Rig:
    """one stream through successive calls of the hook, its model beside it"""

    def __init__(self, gpu, fmt="rgb8", box=BOX, **pol):
        self.gpu, self.fmt, self.box = gpu, fmt, np.asarray(box, F)
        self.pol = dict(cell=C, rng=R, max_cells=CELLS, mode=2, conf_pm=800)
        self.pol.update(pol)
        self.model = cm.Stream()
        self.carry = {}
        self.frames_done = 3

    def step(self, rgb, device_frames=True, **pol):
        p = dict(self.pol, **pol)
        h, w, _ = rgb.shape
        dev = cm.DevFrame(self.gpu, self.fmt, cm.from_rgb(self.fmt, rgb), w, h)
        st = _states(self.gpu, [self.box], w, h, self.frames_done)
        got = self.gpu.op_camera_motion([dev.frame], st, device_frames=device_frames, **p, **self.carry)
        want = self.model.step(dev.rgb, self.box, mode=p["mode"], cell=p["cell"], R=p["rng"], conf_pm=p["conf_pm"],
                               max_cells=p["max_cells"], device=device_frames, frames_done=self.frames_done)
        cm.check_stream(got, 0, want, self.model, p["max_cells"])
        self.carry = dict(thumbs=got["thumbs"], records=got["records"])
        self.box = got["states"][0]["box"].copy()
        self.frames_done += 1
        return got, want


@pytest.mark.parametrize("fmt", cm.FORMATS)
@pytest.mark.parametrize("size", [(W, H), (157, 93)])
def test_formats(gpu, fmt, size):
    """every format, whole cells and partial edge cells (dropped)"""
    w, h = size
    if fmt == "yuy2":
        w &= ~1                      # packed pixel pairs: the one format that needs an even width
    a, b = views((2, -1), w, h)
    rig = Rig(gpu, fmt)
    _, first = rig.step(a)
    _, r = rig.step(b)
    assert first["status"] == 5 and (r["Wg"], r["Hg"]) == (w // C, h // C)
    assert r["status"] == 1 and (r["dx"], r["dy"]) == (2, -1) and r["applied"] == 1, r
    _, again = rig.step(b)          # a still pair behind it: the third thumbnail goes where the first was
    assert again["status"] == 1 and (again["dx"], again["dy"]) == (0, 0) and again["applied"] == 0


@pytest.mark.parametrize("size", [(156, 96), (160, 96), (164, 96), (160, 64), (160, 68), (160, 92), (160, 100)])
def test_central_sizes_around_the_search_tile(gpu, size):
    """the search tile is 32 x 8 central cells: central widths of 31, 32, 33 cells, central heights of 8, 9 (one tile and one
    row more), 15, 16 (two tiles), 17; a central height of 7 is refused by the geometry rule"""
    w, h = size
    a, b = views((-3, 2), w, h)
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(b)
    assert r["status"] == 1 and (r["dx"], r["dy"]) == (-3, 2) and r["n"] == (w // C - 2 * R) * (h // C - 2 * R)
    assert (w // C - 2 * R, h // C - 2 * R) in [(31, 16), (32, 16), (33, 16), (32, 8), (32, 9), (32, 15), (32, 17)]


def test_range_2(gpu):
    a, b = views((1, -1))
    rig = Rig(gpu, rng=2)
    rig.step(a)
    _, r = rig.step(b)
    assert r["status"] == 1 and (r["dx"], r["dy"]) == (1, -1) and r["sad"].shape == (5, 5)


def test_range_16(gpu):
    """every thread of the search owns up to five of the 1089 displacements; 192 x 160: a central 16 x 8"""
    a, b = views((-11, 13), 192, 160)
    rig = Rig(gpu, rng=16)
    rig.step(a)
    _, r = rig.step(b)
    assert r["status"] == 1 and (r["dx"], r["dy"]) == (-11, 13) and r["n"] == 16 * 8 and r["sad"].shape == (33, 33)


def test_sub_cell_shift(gpu):
    canvas = cm.texture(320, 420, seed=7, smooth=6)
    a, b = cm.view(canvas, 80, 80, W, H), cm.view(canvas, 74, 83, W, H)     # +1.5, -0.75 cells
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(b)
    assert r["status"] == 1 and r["S_best"] > 0 and r["off"].any() and r["applied"] == 1
    assert abs(float(r["shift"][0]) - 6) <= C / 2 and abs(float(r["shift"][1]) + 3) <= C / 2


def test_automatic_cell(gpu):
    """max_cells is at least 4096 and 160 x 96 has 960 cells of 4 px: the automatic cell comes out as 8 on 320 x 240 (4800
    cells of 4 px) with max_cells 4096, and as 4 on the same frame with 8192"""
    a, b = views((1, -1), 320, 240, c=8)
    rig = Rig(gpu, cell=0, max_cells=4096)
    rig.step(a)
    _, r = rig.step(b)
    assert (r["c"], r["Wg"], r["Hg"], r["status"], r["dx"], r["dy"]) == (8, 40, 30, 1, 1, -1)
    rig = Rig(gpu, cell=0, max_cells=8192)
    rig.step(a)
    _, r = rig.step(b)
    assert (r["c"], r["Wg"], r["Hg"], r["status"], r["dx"], r["dy"]) == (4, 80, 60, 1, 2, -2)


def test_status_2(gpu):
    a, b = views((1, 0))
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(b, rng=9)           # 24 - 18 < 8: the grid is too small for the range
    assert r["status"] == 2 and (r["c"], r["Wg"], r["Hg"]) == (4, 40, 24) and rig.model.has_prev == 0
    _, r = rig.step(b)
    assert r["status"] == 5             # the previous thumbnail went with the status 2
    big = views((1, 0), 320, 240)[0]
    rig = Rig(gpu, cell=4, max_cells=4096)
    _, r = rig.step(big)                # a fixed cell over max_cells: nothing is written to the thumbnails
    assert r["status"] == 2 and (r["Wg"], r["Hg"]) == (80, 60)
    assert not rig.carry["thumbs"].any()


def test_status_3_flat(gpu):
    a = np.full((H, W, 3), 93, np.uint8)
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(a)
    assert r["status"] == 3 and r["S2"] == 0 and r["applied"] == 0 and rig.model.evaluated == 1


def test_status_5_and_geometry_change(gpu):
    a, b = views((1, 0))
    rig = Rig(gpu)
    assert rig.step(a)[1]["status"] == 5
    assert rig.step(b)[1]["status"] == 1
    assert rig.step(views((1, 0), 164, 96)[0])[1]["status"] == 5        # another frame size
    assert rig.step(views((1, 0), 164, 96)[1])[1]["status"] == 1
    assert rig.step(views((1, 0), 164, 96)[1], cell=8, rng=2)[1]["status"] == 5      # another cell
    assert rig.model.evaluated == 2


@pytest.mark.parametrize("d", [(R, 1), (-2, -R)])
def test_status_6_border(gpu, d):
    a, b = views(d)
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(b)
    assert r["status"] == 6 and (r["dx"], r["dy"]) == d and r["S_best"] == 0 and not r["shift"].any() and r["applied"] == 0


def test_status_7_noise(gpu):
    a, b = (cm.texture(H, W, seed=s, smooth=0) for s in (1, 2))
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(b)
    assert r["status"] == 7 and r["S_best"] * 1000 > 800 * r["S2"] and r["applied"] == 0
    _, r = rig.step(a, conf_pm=1000)        # S_best <= S2 always: the same pair backwards is good at 1000 per mille
    assert r["status"] in (1, 6)


def test_tie_rule_on_a_periodic_picture(gpu):
    col = cm.texture(H + 64, 3 * C, seed=5, smooth=1)
    canvas = np.tile(col, (1, 40, 1))
    a, b = cm.view(canvas, 32, 32, W, H), cm.view(canvas, 32 - 2 * C, 32, W, H)        # +2 cells and -1 cell are one picture
    rig = Rig(gpu)
    rig.step(a)
    _, r = rig.step(b)
    assert (r["dx"], r["dy"], r["S_best"], r["S2"], r["status"]) == (-1, 0, 0, 0, 3)
    assert r["sad"][R, R + 2] == 0 and r["sad"][R, R - 4] == 0


def test_modes_0_and_1_and_host_pass(gpu):
    a, b = views((2, 1))
    rig = Rig(gpu, mode=1)
    rig.step(a)
    got, r = rig.step(b)
    assert r["status"] == 1 and r["applied"] == 0 and got["states"][0]["box"].tolist() == list(BOX) and rig.model.moved == 0
    _, r = rig.step(a, mode=0)
    assert r["status"] == 0 and rig.model.has_prev == 0
    assert rig.step(a)[1]["status"] == 5
    _, r = rig.step(b, device_frames=False)
    assert r["status"] == 4 and rig.model.has_prev == 0
    assert rig.step(b)[1]["status"] == 5


def test_apply_and_mirrors(gpu):
    """applied and not applied (the moved centre leaves the frame); the pinned mirrors take the moved box and the record"""
    a, b = views((3, 0))
    st_dt = importlib.import_module(gpu.__name__ + ".snapshot").STATE
    for box, applied in (((100.0, 40.0, 20.0, 20.0), 1), ((139.0, 40.0, 20.0, 20.0), 0)):
        da, db = (cm.DevFrame(gpu, "rgb8", cm.from_rgb("rgb8", x), W, H) for x in (a, b))
        st = _states(gpu, [box], W, H)
        first = gpu.op_camera_motion([da.frame], st, cell=C, rng=R, max_cells=CELLS)
        hst = np.frombuffer(b"\xa5" * st_dt.itemsize, st_dt).copy()
        hrec = np.frombuffer(b"\xa5" * gpu.CAMERA_REC_DTYPE.itemsize, gpu.CAMERA_REC_DTYPE).copy()
        got = gpu.op_camera_motion([db.frame], st, cell=C, rng=R, max_cells=CELLS, thumbs=first["thumbs"], records=first["records"],
                                   host_states=hst, host_records=hrec)
        rec = got["records"][0]
        assert (rec["status"], rec["dx"], rec["applied"], rec["moved"]) == (1, 3, applied, applied)
        want_box = [box[0] + 12 * applied, box[1], box[2], box[3]]
        assert got["states"][0]["box"].tolist() == want_box
        assert got["host_records"].tobytes() == got["records"].tobytes()
        raw, want = got["host_states"].tobytes(), bytearray(b"\xa5" * st_dt.itemsize)
        if applied:
            want[0:8] = np.asarray(want_box[:2], F).tobytes()
        assert raw == bytes(want)
        for k in st_dt.names:       # every other word of the state stays
            if k != "box":
                assert got["states"][0][k].tobytes() == st[0][k].tobytes(), k


def test_candidate_map_and_partial_list(gpu):
    """a stream named by three slots is worked once, by its first slot; a stream no slot names keeps every byte"""
    a, b = views((2, 2))
    other = cm.texture(H, W, seed=9)
    fa, fb, fo = (cm.DevFrame(gpu, "rgb8", cm.from_rgb("rgb8", x), W, H) for x in (a, b, other))
    st = _states(gpu, [BOX, (10.0, 10.0, 30.0, 30.0), BOX], W, H)
    rng = np.random.default_rng(3)
    thumbs = rng.integers(0, 4081, (3, 2, CELLS)).astype(np.uint16)
    recs = np.frombuffer(rng.integers(0, 256, 3 * gpu.CAMERA_REC_DTYPE.itemsize).astype(np.uint8).tobytes(), gpu.CAMERA_REC_DTYPE).copy()
    recs["has_prev"] = 0
    recs["evaluated"], recs["moved"] = 7, 5
    smap = [2, 2, 0, 2]
    pol = dict(cell=C, rng=R, max_cells=CELLS, slot_stream=smap)
    one = gpu.op_camera_motion([fa.frame, fo.frame, fa.frame, fo.frame], st, thumbs=thumbs, records=recs, **pol)
    two = gpu.op_camera_motion([fb.frame, fo.frame, fb.frame, fa.frame], st, thumbs=one["thumbs"], records=one["records"], **pol)
    for s in (0, 2):
        m = cm.Stream()
        m.evaluated, m.moved = 7, 5
        w1 = m.step(fa.rgb, BOX, cell=C, R=R, max_cells=CELLS, frames_done=3)
        cm.check_stream(one, s, w1, m, CELLS)
        w2 = m.step(fb.rgb, BOX, cell=C, R=R, max_cells=CELLS, frames_done=3)
        cm.check_stream(two, s, w2, m, CELLS)
        assert (w2["status"], w2["dx"], w2["dy"], w2["applied"], w2["evaluated"], w2["moved"]) == (1, 2, 2, 1, 8, 6)
        assert np.array_equal(two["thumbs"][s, :, w2["Wg"] * w2["Hg"]:], thumbs[s, :, w2["Wg"] * w2["Hg"]:])
    for got in (one, two):      # stream 1: in no slot
        assert got["thumbs"][1].tobytes() == thumbs[1].tobytes() and got["records"][1].tobytes() == recs[1].tobytes()
        assert got["states"][1].tobytes() == st[1].tobytes() and (got["sad"][1] == -1).all()


def test_refusals(gpu):
    a, _ = views((0, 0))
    dev = cm.DevFrame(gpu, "rgb8", cm.from_rgb("rgb8", a), W, H)
    st = _states(gpu, [BOX], W, H)
    for bad in (dict(cell=5), dict(cell=64), dict(rng=1), dict(rng=17), dict(mode=3), dict(conf_pm=1001), dict(slot_stream=[1])):
        with pytest.raises(gpu.VtError):
            gpu.op_camera_motion([dev.frame], st, **dict(dict(cell=C, rng=R, max_cells=CELLS), **bad))


def test_sums_beyond_31_bits(gpu):
    """one GRAY8 pair, all 255 against all 0, 4096 x 4096 at cell 4 with max_cells 1,048,576 and R 2: every cell 4080 against
    0, every S = 1020 * 1020 * 4080 = 4,244,832,000 - above 2^31, where a signed 32-bit sum goes wrong (with fewer than 2^20
    cells of at most 4080 no sum reaches 2^32). Expected values in closed form: (0, 0) wins every tie, S_best == S2: status 7"""
    import torch
    n, cells = 4096, 1 << 20
    st = _states(gpu, [(100.0, 100.0, 50.0, 50.0)], n, n)
    carry = {}
    for value in (0, 255):
        t = torch.full((n * n,), value, dtype=torch.uint8, device="cuda")
        frame = gpu.CFrame(t.data_ptr(), None, n, n, n, 0, gpu.PIX_GRAY8, 0, 0, 0, 0, 0)
        got = gpu.op_camera_motion([frame], st, cell=4, rng=2, max_cells=cells, **carry)
        carry = dict(thumbs=got["thumbs"], records=got["records"])
        del t
    rec = got["records"][0]
    S = 1020 * 1020 * 4080
    assert S > 1 << 31
    assert (got["thumbs"][0, 1] == 4080).all() and not got["thumbs"][0, 0].any()
    assert (got["sad"][0, :25] == S).all() and (got["sad"][0, 25:] == -1).all()
    assert (rec["status"], rec["dx"], rec["dy"], rec["n"], rec["S_best"], rec["S0"], rec["S2"]) == (7, 0, 0, 1020 * 1020, S, S, S)
    assert (rec["Wg"], rec["Hg"], rec["c"], rec["applied"]) == (1024, 1024, 4, 0) and not rec["shift"].any()
