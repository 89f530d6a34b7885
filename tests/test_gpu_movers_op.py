"""Moving regions, operator level (vt_op_movers: the launches of csrc/k_movers.hip alone), on the MI355X.

Every comparison is np.array_equal against the NumPy model of tests/movers_util.py: thumbnails, backgrounds, masks, labels,
extents, accumulators, headers, records, counters and states, value for value. The hook keeps every array a launch may write
between guard bands (a changed guard byte is an error of the call); thumbnails, labels, extents and accumulators start as
0xff bytes, and so do the backgrounds and masks of a first call: what a launch must leave alone has to come back as it went
in. Frames of 64 x 48 at cell 4 (16 x 12 cells) unless stated; a grey cell of value v has the thumbnail value 16 v."""
import importlib

import numpy as np
import pytest

import movers_util as mv

pytestmark = pytest.mark.gpu

C, CELLS, HG, WG = 4, 4096, 12, 16
CANVAS = mv.texture(300, 400, seed=47)
OPEN = dict(min_nb=1, min_area=1, global_pm=1000)       # the kept cells are the mask's, every component is listed


def _states(gpu, n, w, h, frames_done=3, initialised=1, box=(10.0, 10.0, 20.0, 20.0)):
    st = np.zeros(n, importlib.import_module(gpu.__name__ + ".snapshot").STATE)
    st["box"] = box
    st["frame_w"], st["frame_h"], st["frames_done"], st["initialized"] = w, h, frames_done, initialised
    return st


def carry_of(got):
    return {k: got[k] for k in ("bg", "mask", "records", "counts")}


def empty_store(gpu, n, max_cells):
    """no background; backgrounds and masks as 0xff bytes: a cell no launch stores shows"""
    return dict(bg=np.full((n, max_cells), 0xFFFF, np.uint16), mask=np.full((n, max_cells), 0xFF, np.uint8),
                records=np.zeros(n, gpu.MOVERS_REC_DTYPE), counts=np.zeros(n, gpu.MOVERS_COUNT_DTYPE))


class Rig:
    """one stream through successive calls of the hook over one store, its model beside it"""

    def __init__(self, gpu, fmt="rgb8", box=(10.0, 10.0, 20.0, 20.0), **pol):
        self.gpu, self.fmt, self.box = gpu, fmt, box
        self.pol = dict(cell=C, max_cells=CELLS)
        self.pol.update(pol)
        self.model = mv.Stream()
        self.carry = empty_store(gpu, 1, self.pol["max_cells"])
        self.frames_done = 0

    def step(self, rgb, device_frames=True, frame=None, **pol):
        p = dict(self.pol, **pol)
        h, w, _ = rgb.shape
        dev = mv.DevFrame(self.gpu, self.fmt, mv.from_rgb(self.fmt, rgb), w, h)
        st = _states(self.gpu, 1, w, h, self.frames_done, box=self.box)
        got = self.gpu.op_movers([frame or dev.frame], st, device_frames=device_frames, **p, **self.carry)
        want = self.model.step(dev.rgb, box=self.box, device=device_frames, whole=frame is None, frames_done=self.frames_done, **p)
        mv.check_stream(got, 0, want, self.model, self.carry)
        head = got["heads"][0]
        assert (int(head["status"]), int(head["stream"]), int(head["frames_done"])) == (1 if want["status"] == 6 else want["status"], 0, self.frames_done)
        if want["status"] in (1, 5, 6):
            assert tuple(int(head[k]) for k in ("c", "Wg", "Hg")) == (want["c"], want["Wg"], want["Hg"])
        assert got["states"].tobytes() == st.tobytes()
        self.carry = carry_of(got)
        self.frames_done += 1
        return got, want


def painted(gpu, mask, c=C, fmt="rgb8", **pol):
    """a fresh rig: a flat grey frame, then the frame with `mask` painted -> (got, want) of the second call"""
    rig = Rig(gpu, fmt, **dict(OPEN, cell=c, **pol))
    _, a = rig.step(mv.paint(np.zeros_like(mask), c))
    assert a["status"] == 5
    return rig.step(mv.paint(mask, c))


def boxes(rec):
    return [(b["box"], b["area"], b["label"]) for b in rec["boxes"]]


def counts(rec):
    return tuple(rec[k] for k in ("status", "n", "moving", "kept", "components"))


# ---- the cases of tests/test_movers_cases.py, painted into frames ------------------------------------------------------------

def test_empty_one_cell_and_a_diagonal_touch(gpu):
    _, r = painted(gpu, np.zeros((HG, WG), bool))
    assert counts(r) == (1, 0, 0, 0, 0)
    _, r = painted(gpu, mv.place(mv.parse(["#"]), HG, WG, 3, 5))
    assert counts(r) == (1, 1, 1, 1, 1) and boxes(r) == [((20, 12, 4, 4), 1, 53)]
    m = mv.place(mv.parse(["##", "##"]), HG, WG, 2, 2) | mv.place(mv.parse(["##", "##"]), HG, WG, 4, 4)
    _, r = painted(gpu, m)
    assert counts(r) == (1, 1, 8, 8, 1) and boxes(r) == [((8, 8, 16, 16), 8, 34)]


def test_u_spiral_comb_and_serpentine(gpu):
    """the shapes whose labels have to travel: a labelling that stops early leaves more than one label"""
    _, r = painted(gpu, mv.place(mv.U_SHAPE, HG, WG, 1, 2))
    assert counts(r) == (1, 1, 11, 11, 1) and boxes(r) == [((8, 4, 20, 16), 11, 18)]
    got, r = painted(gpu, mv.place(mv.SPIRAL, HG, WG, 1, 1))
    assert counts(r) == (1, 1, 49, 49, 1) and boxes(r) == [((4, 4, 36, 36), 49, 17)]
    assert set(np.unique(got["labels"][0, :HG * WG])) == {-1, 17}
    _, r = painted(gpu, mv.place(mv.COMB, HG, WG, 2, 2))
    assert counts(r) == (1, 1, 29, 29, 1) and boxes(r) == [((8, 8, 44, 16), 29, 34)]
    got, r = painted(gpu, mv.serpentine(HG, WG))
    assert counts(r) == (1, 1, 101, 101, 1) and boxes(r) == [((0, 0, 64, 44), 101, 0)]
    got, r = painted(gpu, mv.serpentine(WG, HG).T)      # the same upright: labels travel against the row-major order
    assert counts(r)[1:] == (1, 8 * HG + 7, 8 * HG + 7, 1) and boxes(r)[0][2] == 0


def test_four_borders_the_cut_with_a_tie_and_min_area(gpu):
    m = np.zeros((HG, WG), bool)
    m[6, :] = True
    m[:, 8] = True
    _, r = painted(gpu, m)
    assert counts(r) == (1, 1, 27, 27, 1) and boxes(r) == [((0, 0, 64, 48), 27, 8)]
    m = mv.place(mv.parse(["###"]), HG, WG, 9, 1) | mv.place(mv.parse(["##"]), HG, WG, 2, 8) | mv.place(mv.parse(["#", "#"]), HG, WG, 5, 3)
    _, r = painted(gpu, m, max_n=2)
    assert counts(r) == (1, 2, 7, 7, 3) and boxes(r) == [((4, 36, 12, 4), 3, 145), ((32, 8, 8, 4), 2, 40)]
    _, r = painted(gpu, m, max_n=8)
    assert boxes(r)[2] == ((12, 20, 4, 8), 2, 83) and r["n"] == 3
    m = mv.place(mv.parse(["##", "##"]), HG, WG, 5, 5)
    for min_area, n in ((3, 1), (4, 1), (5, 0)):
        _, r = painted(gpu, m, min_area=min_area)
        assert counts(r) == (1, n, 4, 4, 1)
    nine = np.zeros((HG, WG), bool)
    nine[1::4, 1::2] = True         # 3 rows of 8 lone cells: 24 components, eight listed in label order
    _, r = painted(gpu, nine, max_n=8)
    assert counts(r) == (1, 8, 24, 24, 24) and [b[2] for b in boxes(r)] == [17, 19, 21, 23, 25, 27, 29, 31]


def test_global_change_at_below_and_above(gpu):
    for cells, status in ((47, 1), (48, 1), (49, 6)):
        m = np.zeros(HG * WG, bool)
        m[:cells] = True
        got, r = painted(gpu, m.reshape(HG, WG), global_pm=250)
        assert counts(r) == (status, 1 if status == 1 else 0, cells, cells, 1 if status == 1 else 0)
        assert int(got["counts"][0]["evaluated"]) == 1 and int(got["records"][0]["status"]) == status


def test_threshold_learn_and_the_ends_of_the_range(gpu):
    """grey steps of 6 and 7 at thr 96: |d| = 16 * 96 does not move, 16 * 112 does; one pixel of a cell one grey level down is
    d = -16: learn 8 moves the background by -1 (the floor), learn 0 to 16 t; black to white and back at thr 4079 and 4080"""
    base = mv.grey(48, 64, 100)
    for delta, moving in ((6, 0), (7, 1), (-6, 0), (-7, 1)):
        rig = Rig(gpu, **dict(OPEN, thr=96))
        rig.step(base)
        pic = base.copy()
        pic[16:20, 16:20] = 100 + delta
        _, r = rig.step(pic)
        assert r["moving"] == moving and int(r["bg"][4, 4]) == 1600 * 16 + delta * 16 and int(r["bg"][0, 0]) == 25600
    for learn, bg in ((8, 25599), (0, 25584), (4, 25599)):
        rig = Rig(gpu, **dict(OPEN, learn=learn))
        rig.step(base)
        pic = base.copy()
        pic[17, 18] = 99
        got, r = rig.step(pic)
        assert int(r["thumb"][4, 4]) == 1599 and int(got["bg"][0, 4 * WG + 4]) == bg and r["moving"] == 0
    for first, second in ((0, 255), (255, 0)):
        for thr, moving in ((4079, 192), (4080, 0)):
            rig = Rig(gpu, **dict(OPEN, thr=thr, learn=0))
            _, a = rig.step(mv.grey(48, 64, first))
            got, r = rig.step(mv.grey(48, 64, second))
            assert (a["bg"] == 16 * 16 * first).all() and (got["bg"][0, :192] == 16 * 16 * second).all() and r["moving"] == moving


def test_clean_up(gpu):
    m = mv.place(mv.parse(["##", "##"]), HG, WG, 5, 5) | mv.place(mv.parse(["#"]), HG, WG, 9, 12)
    got, r = painted(gpu, m, min_nb=4)
    assert counts(r) == (1, 1, 5, 4, 1) and boxes(r) == [((20, 20, 8, 8), 4, 85)]
    assert got["mask"][0, 9 * WG + 12] == 1 and got["mask"][0, 5 * WG + 5] == 2
    _, r = painted(gpu, mv.place(mv.parse(["##", "#."]), HG, WG, 0, 0), min_nb=4)       # cells beyond the border do not count
    assert counts(r) == (1, 0, 3, 0, 0)
    _, r = painted(gpu, mv.place(mv.parse([".#", "##"]), HG, WG, HG - 2, WG - 2), min_nb=3)
    assert counts(r) == (1, 1, 3, 3, 1) and boxes(r) == [((56, 40, 8, 8), 3, 175)]
    _, r = painted(gpu, np.ones((HG, WG), bool), min_nb=9)
    assert r["kept"] == (HG - 2) * (WG - 2) and boxes(r) == [((4, 4, 56, 40), 140, 17)]


def test_three_chained_passes_own_box_and_still(gpu):
    """the background of a pass is the output of the pass before; the stream's own box lies beside the blob: still counts"""
    blob = mv.place(mv.parse(["###", "###", "###"]), HG, WG, 2, 2)
    rig = Rig(gpu, box=(40.0, 0.0, 8.0, 8.0), learn=4)
    recs = [rig.step(mv.paint(m, C, 60, 90))[1] for m in (np.zeros((HG, WG), bool), blob, blob, blob)]
    assert [r["status"] for r in recs] == [5, 1, 1, 1] and [int(r["bg"][3, 3]) for r in recs] == [15360, 15840, 16290, 16711]
    assert [(r["own_cells"], r["own_kept"], r["still"], r["kept"]) for r in recs[1:]] == [(4, 0, 1, 9), (4, 0, 2, 9), (4, 0, 3, 9)]
    assert (rig.model.evaluated, rig.model.listed) == (3, 3)
    rig = Rig(gpu, box=(9.5, 6.0, 5.0, 9.5), **OPEN)               # cells 2..3 x 1..3: floor(2.375), ceil(3.625); floor(1.5), ceil(3.875)
    rig.step(mv.paint(np.zeros((HG, WG), bool), C))
    _, r = rig.step(mv.paint(blob, C))
    assert (r["own_cells"], r["own_kept"], r["still"]) == (6, 4, 0)
    for box, own in (((-30.0, -4.0, 20.0, 10.0), 0), ((0.0, 0.0, 1000.0, 1000.0), 192), ((63.9, 47.9, 0.05, 0.05), 1)):
        rig = Rig(gpu, box=box, **OPEN)
        rig.step(mv.paint(np.zeros((HG, WG), bool), C))
        assert rig.step(mv.paint(blob, C))[1]["own_cells"] == own


# ---- grids, formats, slots ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("grid", [(8, 8), (17, 16), (33, 9), (64, 64)])
def test_cell_grids_on_a_textured_picture(gpu, grid):
    """8 x 8: a quarter of a workgroup; 17 x 16: a ragged second one, rows that straddle it; 33 x 9: neither side a multiple
    of anything; 64 x 64 at max_cells 4096: an exact fit, sixteen workgroups. Pixel sizes are no multiples of the cell. The
    second picture is the first shifted: a mask with hundreds of ragged components"""
    wg, hg = grid
    w, h = wg * C + (3 if wg != 64 else 0), hg * C + 2
    rig = Rig(gpu, thr=350, min_nb=2, min_area=2, global_pm=1000, max_n=8)
    _, a = rig.step(CANVAS[:h, :w])
    _, b = rig.step(CANVAS[5:5 + h, 7:7 + w])
    _, c = rig.step(CANVAS[5:5 + h, 7:7 + w])
    assert [r["status"] for r in (a, b, c)] == [5, 1, 1] and (a["Wg"], a["Hg"]) == grid
    assert b["components"] > 1 and b["n"] >= 1 and c["moving"] <= b["moving"]


def test_the_automatic_cell_and_one_cell_too_many(gpu):
    """320 x 240 at max_cells 4096: c = 8, 40 x 30 cells; 65 x 64 cells of 4 px: status 2 with the cell fixed"""
    rig = Rig(gpu, cell=0, thr=350, min_nb=2, global_pm=1000)
    _, a = rig.step(CANVAS[:240, :320])
    _, b = rig.step(CANVAS[9:249, 11:331])
    assert (a["status"], a["c"], a["Wg"], a["Hg"]) == (5, 8, 40, 30) and b["status"] == 1 and b["components"] > 1
    for k in range(b["n"]):
        x, y, w, h = b["boxes"][k]["box"]
        assert x % 8 == 0 and y % 8 == 0 and w % 8 == 0 and h % 8 == 0
    before = rig.carry
    got, r = rig.step(CANVAS[:256, :260], cell=4)
    assert (r["status"], r["c"], r["Wg"], r["Hg"]) == (2, 4, 65, 64) and int(got["records"][0]["has_bg"]) == 0
    assert got["bg"].tobytes() == before["bg"].tobytes() and got["mask"].tobytes() == before["mask"].tobytes()
    assert rig.step(CANVAS[:240, :320])[1]["status"] == 5


def test_a_full_store_of_one_serpentine(gpu):
    """64 x 64 cells at max_cells 4096, one path through every other row: 2079 cells under one label, whatever the order
    the sixteen workgroups meet in"""
    m = mv.serpentine(64, 64)
    got, r = painted(gpu, m)
    assert counts(r) == (1, 1, 2079, 2079, 1) and boxes(r) == [((0, 0, 256, 252), 2079, 0)]
    assert set(np.unique(got["labels"][0])) == {-1, 0}


@pytest.mark.parametrize("fmt", mv.FORMATS)
def test_formats(gpu, fmt):
    rig = Rig(gpu, fmt, thr=350, min_nb=2, global_pm=1000)
    rig.step(CANVAS[:68, :132])
    _, r = rig.step(CANVAS[30:98, 20:152])
    assert r["status"] == 1 and (r["Wg"], r["Hg"]) == (33, 17) and r["moving"] > 0


def test_nv12_with_colour_bits_is_its_rgb8_sibling(gpu):
    import colorimetry_util as col
    from test_gpu_planar_formats import _device
    w, h = 128, 96
    st = _states(gpu, 1, w, h)
    nv12 = [col.random_nv12(w, h, seed=80 + k) for k in range(2)]
    out = {}
    for name in ("coloured", "sibling"):
        frames = []
        for k in range(2):
            if name == "coloured":
                f, keep = _device(gpu, "nv12", col.format_bytes("nv12", nv12[k], w, h), w, h)
                f.format = col.word(gpu, "nv12", 2)
            else:
                f, keep = _device(gpu, "rgb8", col.sibling_of("nv12", nv12[k], w, h, 2), w, h)
            frames.append((f, keep))
        pol = dict(cell=4, max_cells=CELLS, thr=20, min_nb=2, global_pm=1000)
        one = gpu.op_movers([frames[0][0]], st, **pol)
        two = gpu.op_movers([frames[1][0]], st, **pol, **carry_of(one))
        out[name] = {k: np.asarray(v).tobytes() for k, v in two.items() if isinstance(v, np.ndarray)}
        assert int(two["records"][0]["status"]) == 1 and int(two["records"][0]["moving"]) > 0
    assert out["coloured"].keys() == out["sibling"].keys()
    for k in out["coloured"]:
        assert out["coloured"][k] == out["sibling"][k], k


def test_every_status(gpu):
    pic = CANVAS[:100, :160]
    rig = Rig(gpu)
    assert rig.step(pic, on=0)[1]["status"] == 0
    assert rig.step(pic)[1]["status"] == 5
    assert rig.step(pic)[1]["status"] == 1
    assert rig.step(pic, device_frames=False)[1]["status"] == 4        # devflag 0
    assert rig.step(pic)[1]["status"] == 5
    assert rig.step(pic)[1]["status"] == 1
    assert rig.step(CANVAS[:28, :160])[1]["status"] == 2               # Hg = 7
    assert rig.step(CANVAS[:32, :160])[1]["status"] == 5               # Hg = 8
    assert rig.step(CANVAS[:32, :160], cell=8)[1]["status"] == 2       # another cell: Hg = 4
    dev = mv.DevFrame(gpu, "rgb8", mv.from_rgb("rgb8", CANVAS[:32, :160]), 160, 32)
    win = gpu.CFrame(dev.frame.plane0, None, 320, 64, dev.frame.stride0, 0, gpu.PIX_RGB8, 0, 0, 1, 160, 32)
    got, r = rig.step(CANVAS[:32, :160], frame=win)                     # the planes hold a window of the frame only
    assert r["status"] == 4 and int(got["records"][0]["has_bg"]) == 0
    assert (rig.model.evaluated, rig.model.listed) == (2, 0)


def test_uninitialised_stream_and_period(gpu):
    pic = CANVAS[:100, :160]
    dev = mv.DevFrame(gpu, "rgb8", mv.from_rgb("rgb8", pic), 160, 100)
    st = _states(gpu, 1, 160, 100, initialised=0)
    got = gpu.op_movers([dev.frame], st, cell=C, max_cells=CELLS)
    assert int(got["heads"][0]["status"]) == 0 and not got["records"].tobytes().strip(b"\0")
    assert (got["bg"] == 0xFFFF).all() and (got["mask"] == 0xFF).all() and (got["accs"] == -1).all() and (got["labels"] == -1).all()
    rig = Rig(gpu, period=2)
    assert [rig.step(pic)[1]["status"] for _ in range(5)] == [5, 0, 1, 0, 1] and rig.model.evaluated == 2


def test_slots_streams_and_the_mirror(gpu):
    """a slot map that is not the identity; a stream named by two slots is worked once, by its first slot; a stream no slot
    names and one that is not initialised keep every byte; the pinned mirror takes the records of the worked streams only"""
    w, h = 160, 100
    pa, pb, po = CANVAS[:h, :w], CANVAS[30:30 + h, 30:30 + w], CANVAS[10:10 + h, 90:90 + w]
    fa, fb, fo = (mv.DevFrame(gpu, "rgb8", mv.from_rgb("rgb8", x), w, h) for x in (pa, pb, po))
    st = _states(gpu, 4, w, h)
    st["initialized"][3] = 0
    rng = np.random.default_rng(5)
    before = dict(bg=rng.integers(0, 65281, (4, CELLS)).astype(np.uint16), mask=rng.integers(0, 3, (4, CELLS)).astype(np.uint8),
                  records=np.frombuffer(rng.integers(0, 256, 4 * 256).astype(np.uint8).tobytes(), gpu.MOVERS_REC_DTYPE).copy(),
                  counts=np.frombuffer(rng.integers(0, 100, 16).astype(np.int32).tobytes(), gpu.MOVERS_COUNT_DTYPE).copy())
    before["records"]["has_bg"] = 0
    before["records"]["still"] = 0
    smap = [2, 2, 0, 3]
    pol = dict(cell=C, max_cells=CELLS, slot_stream=smap, thr=350, min_nb=2, global_pm=1000)
    mpol = {k: v for k, v in pol.items() if k != "slot_stream"}
    mirror = np.frombuffer(b"\xa5" * (4 * 256), gpu.MOVERS_REC_DTYPE).copy()
    one = gpu.op_movers([fa.frame, fo.frame, fb.frame, fa.frame], st, host_records=mirror, **pol, **before)
    two = gpu.op_movers([fb.frame, fo.frame, fa.frame, fa.frame], st, host_records=one["host_records"], **pol, **carry_of(one))
    assert one["heads"]["status"].tolist() == [5, -1, 5, 0] and two["heads"]["status"].tolist() == [1, -1, 1, 0]
    assert one["heads"]["stream"].tolist() == smap
    for s, pics in ((2, (fa, fb)), (0, (fb, fa))):
        m = mv.Stream()
        m.evaluated, m.listed = int(before["counts"][s]["evaluated"]), int(before["counts"][s]["listed"])
        mv.check_stream(one, s, m.step(pics[0].rgb, box=(10.0, 10.0, 20.0, 20.0), frames_done=3, **mpol), m, before)
        want = m.step(pics[1].rgb, box=(10.0, 10.0, 20.0, 20.0), frames_done=3, **mpol)
        mv.check_stream(two, s, want, m, carry_of(one))
        assert want["status"] == 1 and want["moving"] > 0
        assert two["host_records"][s].tobytes() == two["records"][s].tobytes()
    for got in (one, two):      # stream 1: in no slot; stream 3: not initialised
        for s in (1, 3):
            for k in before:
                assert got[k][s].tobytes() == before[k][s].tobytes(), (s, k)
            assert got["host_records"][s].tobytes() == mirror[s].tobytes() and (got["accs"][s] == -1).all()
            assert (got["labels"][s] == -1).all() and (got["thumbs"][s] == 0xFFFF).all()
        assert got["states"].tobytes() == st.tobytes()


def test_the_largest_store_one_path_through_it(gpu):
    """2048 x 2048 GRAY8 at cell 4: 262,144 cells, the most a store holds, and one serpentine of 131,327 cells through them: the
    longest path a labelling can meet. Expected values in closed form"""
    import torch
    side, g, n = 2048, 512, 262144
    st = _states(gpu, 1, side, side)
    m = torch.from_numpy(mv.serpentine(g, g)).cuda()
    flat = torch.full((side, side), 60, dtype=torch.uint8, device="cuda")
    snake = torch.where(m.repeat_interleave(4, 0).repeat_interleave(4, 1), torch.tensor(200, dtype=torch.uint8, device="cuda"), flat)
    frames = [gpu.CFrame(t.data_ptr(), None, side, side, side, 0, gpu.PIX_GRAY8, 0, 0, 0, 0, 0) for t in (flat, snake)]
    pol = dict(cell=4, max_cells=n, **OPEN)
    one = gpu.op_movers([frames[0]], st, **pol)
    two = gpu.op_movers([frames[1]], st, **pol, **carry_of(one))
    cells = 256 * g + 255
    r = two["records"][0]
    assert (int(r["status"]), int(r["n"]), int(r["moving"]), int(r["kept"]), int(r["components"])) == (1, 1, cells, cells, 1)
    e = r["box"][0]
    assert (int(e["x"]), int(e["y"]), int(e["w"]), int(e["h"]), int(e["area"]), int(e["label"])) == (0, 0, side, side - 4, cells, 0)
    lab = two["labels"][0].reshape(g, g)
    assert np.array_equal(lab, np.where(m.cpu().numpy(), 0, -1))
    assert (two["thumbs"][0].reshape(g, g) == np.where(m.cpu().numpy(), 3200, 960)).all()


def test_refusals(gpu):
    dev = mv.DevFrame(gpu, "rgb8", mv.from_rgb("rgb8", CANVAS[:100, :160]), 160, 100)
    st = _states(gpu, 1, 160, 100)
    for bad in (dict(cell=5), dict(cell=64), dict(period=0), dict(thr=4081), dict(min_area=0), dict(global_pm=1001), dict(learn=9),
                dict(min_nb=0), dict(min_nb=10), dict(max_n=0), dict(max_n=9), dict(on=2), dict(max_cells=4095), dict(max_cells=262145),
                dict(shape=-1), dict(shape=4 | 3 << 4 | 4 << 8 | 1 << 12), dict(slot_stream=[1])):
        with pytest.raises(gpu.VtError):
            gpu.op_movers([dev.frame], st, **dict(dict(cell=C, max_cells=CELLS), **bad))
