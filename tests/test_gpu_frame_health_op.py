"""Frame health, operator level (vt_op_frame_health: the four launches of csrc/k_health.hip alone), on the MI355X.

Every comparison is np.array_equal against the NumPy model of tests/frame_health_util.py: thumbnails, accumulators,
histograms, headers, records, counters and states, value for value. The hook keeps every array a launch may write between
guard bands (a changed guard byte is an error of the call); accumulators start as 0xff bytes, and so do the thumbnails and
histograms of a first call: what a launch must leave alone has to come back as it went in. Cell 4 unless stated."""
import importlib

import numpy as np
import pytest

import frame_health_util as fh

pytestmark = pytest.mark.gpu

C, CELLS = 4, 4096
CANVAS = fh.texture(300, 300, seed=31)


def _states(gpu, n, w, h, frames_done=3, initialised=1):
    st = np.zeros(n, importlib.import_module(gpu.__name__ + ".snapshot").STATE)
    st["box"] = (10.0, 10.0, 20.0, 20.0)
    st["frame_w"], st["frame_h"], st["frames_done"], st["initialized"] = w, h, frames_done, initialised
    return st


def picture(w, h, x=0, y=0):
    return CANVAS[y:y + h, x:x + w]


def carry_of(got):
    return {k: got[k] for k in ("thumbs", "hist", "records", "counts")}


def empty_store(gpu, n, max_cells):
    """no previous thumbnail; thumbnails and histograms as 0xff bytes: a cell or bin no launch stores shows"""
    return dict(thumbs=np.full((n, 2, max_cells), 0xFFFF, np.uint16), hist=np.full((n, 2, 32), -1, np.int32),
                records=np.zeros(n, gpu.HEALTH_REC_DTYPE), counts=np.zeros(n, gpu.HEALTH_COUNT_DTYPE))


class Rig:
    """one stream through successive calls of the hook over one store, its model beside it"""

    def __init__(self, gpu, fmt="rgb8", **pol):
        self.gpu, self.fmt = gpu, fmt
        self.pol = dict(cell=C, max_cells=CELLS)
        self.pol.update(pol)
        self.model = fh.Stream()
        self.carry = empty_store(gpu, 1, self.pol["max_cells"])
        self.frames_done = 0

    def step(self, rgb, device_frames=True, frame=None, **pol):
        p = dict(self.pol, **pol)
        h, w, _ = rgb.shape
        dev = fh.DevFrame(self.gpu, self.fmt, fh.from_rgb(self.fmt, rgb), w, h)
        st = _states(self.gpu, 1, w, h, self.frames_done)
        got = self.gpu.op_frame_health([frame or dev.frame], st, device_frames=device_frames, **p, **self.carry)
        want = self.model.step(dev.rgb, device=device_frames, whole=frame is None, frames_done=self.frames_done,
                               **{k: v for k, v in p.items() if k != "gate"})
        fh.check_stream(got, 0, want, self.model, self.carry)
        head = got["heads"][0]
        assert (int(head["status"]), int(head["stream"]), int(head["frames_done"])) == (want["status"], 0, self.frames_done)
        if want["status"] in fh.MEASURED:
            assert tuple(int(head[k]) for k in ("c", "Wg", "Hg", "cur")) == (want["c"], want["Wg"], want["Hg"], self.model.cur)
        assert got["states"].tobytes() == st.tobytes()
        self.carry = carry_of(got)
        self.frames_done += 1
        return got, want


@pytest.mark.parametrize("grid", [(8, 8), (16, 16), (17, 16), (33, 9), (64, 64)])
def test_cell_grids(gpu, grid):
    """8 x 8: a quarter of a workgroup; 16 x 16: one full workgroup; 17 x 16: a ragged second one; 33 x 9: rows that straddle
    workgroups; 64 x 64 at max_cells 4096: an exact fit, sixteen workgroups. Pixel sizes are no multiples of the cell"""
    wg, hg = grid
    w, h = wg * C + (3 if wg != 64 else 0), hg * C + 2
    rig = Rig(gpu)
    _, a = rig.step(picture(w, h))
    _, b = rig.step(picture(w, h, 7, 5))
    _, c = rig.step(picture(w, h, 7, 5))
    assert [r["status"] for r in (a, b, c)] == [5, 1, 1] and (a["Wg"], a["Hg"]) == grid
    assert b["D"] > 0 and b["G"] > 0 and c["D"] == 0 and c["still"] == 1


def test_one_cell_too_many_and_the_automatic_cell(gpu):
    """65 x 64 cells of 4 px at max_cells 4096: status 2 with the cell fixed, c = 8 with the automatic cell"""
    pic = picture(260, 256)
    rig = Rig(gpu)
    rig.step(picture(256, 256))
    before = rig.carry
    got, r = rig.step(pic)
    assert (r["status"], r["c"], r["Wg"], r["Hg"]) == (2, 4, 65, 64) and int(got["records"][0]["has_prev"]) == 0
    assert got["thumbs"].tobytes() == before["thumbs"].tobytes() and got["hist"].tobytes() == before["hist"].tobytes()
    rig = Rig(gpu, cell=0)
    _, r = rig.step(pic)
    assert (r["status"], r["c"], r["Wg"], r["Hg"]) == (5, 8, 32, 32)
    assert rig.step(pic)[1]["status"] == 1


@pytest.mark.parametrize("fmt", fh.FORMATS)
def test_formats(gpu, fmt):
    rig = Rig(gpu, fmt)
    rig.step(picture(132, 68))
    _, r = rig.step(picture(132, 68, 20, 30))
    assert r["status"] == 1 and (r["Wg"], r["Hg"]) == (33, 17) and r["D"] > 0


def test_the_largest_sums(gpu):
    """2048 x 2048 GRAY8 at cell 4: 262,144 cells, the most a store holds. A white-out: S2 = n * 4080^2 > 2^32 and n * S2
    = S1 * S1 = 0.99 * 2^60; then half black, half white: a standard deviation of exactly 2040, flat at flat_q 2040 and not at
    2039. Expected values in closed form"""
    import torch
    side, n = 2048, 262144
    st = _states(gpu, 1, side, side)
    white = torch.full((side * side,), 255, dtype=torch.uint8, device="cuda")
    half = white.clone().reshape(side, side)
    half[:, :side // 2] = 0
    frames = [gpu.CFrame(t.data_ptr(), None, side, side, side, 0, gpu.PIX_GRAY8, 0, 0, 0, 0, 0) for t in (white, half)]
    got = gpu.op_frame_health([frames[0]], st, cell=4, max_cells=n, flat_q=0)
    r = got["records"][0]
    S1, S2 = n * 4080, n * 4080 * 4080
    assert S2 > 1 << 32 and 1 << 59 < n * S2 == S1 * S1 < 1 << 60
    assert (int(r["status"]), int(r["S1"]), int(r["S2"]), int(r["G"]), int(r["flags"])) == (5, S1, S2, 0, fh.FLAT)
    assert (got["thumbs"][0, 0] == 4080).all() and got["hist"][0, 0].tolist() == [0] * 31 + [n]
    for q, flags in ((2040, fh.FLAT | fh.CUT), (2039, fh.CUT)):
        two = gpu.op_frame_health([frames[1]], st, cell=4, max_cells=n, flat_q=q, **carry_of(got))
        r = two["records"][0]
        assert (int(r["status"]), int(r["S1"]), int(r["S2"]), int(r["flags"])) == (1, S1 // 2, S2 // 2, flags), r
        assert (int(r["G"]), int(r["D"]), int(r["HD"]), int(r["G_ref"])) == (512 * 4080, S1 // 2, n, 512 * 4080)
        assert two["accs"][0].tolist() == [S1 // 2, S2 // 2, 512 * 4080, S1 // 2]
        assert two["hist"][0, 1].tolist() == [n // 2] + [0] * 30 + [n // 2]


def test_every_status(gpu):
    pic = picture(160, 100)
    rig = Rig(gpu, still_run=2)
    assert rig.step(pic, on=0)[1]["status"] == 0
    assert rig.step(pic)[1]["status"] == 5
    assert rig.step(pic)[1]["status"] == 1
    _, r = rig.step(pic)
    assert (r["status"], r["still"], r["flags"]) == (1, 2, fh.FROZEN)
    assert rig.step(pic, device_frames=False)[1]["status"] == 4
    assert rig.step(pic)[1]["status"] == 5
    assert rig.step(pic, max_cells=4096, cell=4)[1]["status"] == 1
    assert rig.step(picture(160, 28))[1]["status"] == 2        # Hg = 7
    assert rig.step(picture(160, 32))[1]["status"] == 5        # Hg = 8
    dev = fh.DevFrame(gpu, "rgb8", fh.from_rgb("rgb8", picture(160, 32)), 160, 32)
    win = gpu.CFrame(dev.frame.plane0, None, 320, 64, dev.frame.stride0, 0, gpu.PIX_RGB8, 0, 0, 1, 160, 32)
    got, r = rig.step(picture(160, 32), frame=win)             # the planes hold a window of the frame only
    assert r["status"] == 4 and int(got["records"][0]["has_prev"]) == 0
    assert (rig.model.evaluated, rig.model.flagged) == (6, 1)      # statuses 5, 1, 1, 5, 1, 5


def test_uninitialised_stream_and_period(gpu):
    pic = picture(160, 100)
    dev = fh.DevFrame(gpu, "rgb8", fh.from_rgb("rgb8", pic), 160, 100)
    st = _states(gpu, 1, 160, 100, initialised=0)
    got = gpu.op_frame_health([dev.frame], st, cell=C, max_cells=CELLS)
    assert int(got["heads"][0]["status"]) == 0 and not got["records"].tobytes().strip(b"\0")
    assert (got["thumbs"] == 0xFFFF).all() and (got["hist"] == -1).all() and (got["accs"] == -1).all()
    rig = Rig(gpu, period=2, still_run=1)
    statuses = [rig.step(pic)[1]["status"] for _ in range(5)]          # frames_done 0..4
    assert statuses == [5, 0, 1, 0, 1] and rig.model.rec["flags"] == fh.FROZEN and rig.model.evaluated == 3


def test_three_pass_sequences_over_one_store(gpu):
    a, b = picture(160, 100), picture(160, 100, 40, 60)
    grey = fh.grey(100, 160, 90)
    # frozen, then changed
    rig = Rig(gpu, still_run=1)
    flags = [rig.step(p)[1]["flags"] for p in (a, a, b)]
    assert flags[:2] == [0, fh.FROZEN] and not flags[2] & fh.FROZEN
    # cut to a constant picture and back: CUT and FLAT, G_ref follows the cuts
    rig = Rig(gpu)
    recs = [rig.step(p)[1] for p in (a, grey, a)]
    assert [r["flags"] for r in recs] == [0, fh.CUT | fh.FLAT, fh.CUT] and [r["G_ref"] for r in recs] == [recs[0]["G"], 0, recs[0]["G"]]
    # a geometry change in the middle
    rig = Rig(gpu)
    assert [rig.step(p)[1]["status"] for p in (a, a[:, :128], a[:, :128])] == [5, 5, 1]
    rig = Rig(gpu)
    assert [rig.step(a, cell=c)[1]["status"] for c in (4, 8, 8)] == [5, 5, 1]
    # period 2
    rig = Rig(gpu, period=2)
    assert [rig.step(p)[1]["status"] for p in (a, b, a)] == [5, 0, 1] and rig.model.rec["D"] == 0


def test_slots_streams_and_the_mirror(gpu):
    """a stream named by two slots is worked once, by its first slot; a stream no slot names keeps every byte; the pinned
    mirror takes the records of the worked streams and nothing else"""
    w, h = 160, 100
    pa, pb, po = picture(w, h), picture(w, h, 30, 30), picture(w, h, 90, 10)
    fa, fb, fo = (fh.DevFrame(gpu, "rgb8", fh.from_rgb("rgb8", x), w, h) for x in (pa, pb, po))
    st = _states(gpu, 4, w, h)
    st["initialized"][3] = 0
    rng = np.random.default_rng(5)
    before = dict(thumbs=rng.integers(0, 4081, (4, 2, CELLS)).astype(np.uint16),
                  hist=rng.integers(0, 99, (4, 2, 32)).astype(np.int32),
                  records=np.frombuffer(rng.integers(0, 256, 4 * 104).astype(np.uint8).tobytes(), gpu.HEALTH_REC_DTYPE).copy(),
                  counts=np.frombuffer(rng.integers(0, 100, 16).astype(np.int32).tobytes(), gpu.HEALTH_COUNT_DTYPE).copy())
    before["records"]["has_prev"] = 0
    before["records"]["still"] = 0
    smap = [2, 2, 0, 3]
    pol = dict(cell=C, max_cells=CELLS, slot_stream=smap, still_run=1)
    mirror = np.frombuffer(b"\xa5" * (4 * 104), gpu.HEALTH_REC_DTYPE).copy()
    one = gpu.op_frame_health([fa.frame, fo.frame, fb.frame, fa.frame], st, host_records=mirror, **pol, **before)
    two = gpu.op_frame_health([fa.frame, fo.frame, fa.frame, fa.frame], st, host_records=one["host_records"], **pol, **carry_of(one))
    assert one["heads"]["status"].tolist() == [5, -1, 5, 0] and two["heads"]["status"].tolist() == [1, -1, 1, 0]
    assert one["heads"]["stream"].tolist() == smap
    for s, pics in ((2, (fa, fa)), (0, (fb, fa))):
        m = fh.Stream()
        m.evaluated, m.flagged = int(before["counts"][s]["evaluated"]), int(before["counts"][s]["flagged"])
        fh.check_stream(one, s, m.step(pics[0].rgb, cell=C, max_cells=CELLS, still_run=1, frames_done=3), m, before)
        fh.check_stream(two, s, m.step(pics[1].rgb, cell=C, max_cells=CELLS, still_run=1, frames_done=3), m, carry_of(one))
        assert int(two["counts"][s]["gated"]) == int(before["counts"][s]["gated"])
        assert two["host_records"][s].tobytes() == two["records"][s].tobytes()
    assert int(two["records"][2]["flags"]) == fh.FROZEN and int(two["records"][0]["flags"]) == 0
    for got in (one, two):      # stream 1: in no slot; stream 3: not initialised
        for s in (1, 3):
            for k in before:
                assert got[k][s].tobytes() == before[k][s].tobytes(), (s, k)
            assert got["host_records"][s].tobytes() == mirror[s].tobytes() and (got["accs"][s] == -1).all()
        assert got["states"].tobytes() == st.tobytes()


def test_six_hundred_slots(gpu):
    """the prepare launch looks through the slots ahead of its own with 256 threads: a first slot at index 520, found from
    slot 599 in the third round of the scan; streams 0..2 named 199 or 200 times each, stream 4 by nobody"""
    w, h = 36, 34
    dev = fh.DevFrame(gpu, "rgb8", fh.from_rgb("rgb8", picture(w, h, 50, 50)), w, h)
    smap = [j % 3 for j in range(600)]
    smap[520] = smap[599] = 3
    st = _states(gpu, 5, w, h)
    before = empty_store(gpu, 5, CELLS)
    got = gpu.op_frame_health([dev.frame] * 600, st, cell=C, max_cells=CELLS, slot_stream=smap, **before)
    want = [5 if j in (0, 1, 2, 520) else -1 for j in range(600)]
    assert got["heads"]["status"].tolist() == want and got["heads"]["stream"].tolist() == smap
    for s in range(4):
        m = fh.Stream()
        fh.check_stream(got, s, m.step(dev.rgb, cell=C, max_cells=CELLS, frames_done=3), m, before)
    for k in before:
        assert got[k][4].tobytes() == before[k][4].tobytes(), k
    assert (got["accs"][4] == -1).all() and got["states"].tobytes() == st.tobytes()


def test_refusals(gpu):
    dev = fh.DevFrame(gpu, "rgb8", fh.from_rgb("rgb8", picture(160, 100)), 160, 100)
    st = _states(gpu, 1, 160, 100)
    for bad in (dict(cell=5), dict(cell=64), dict(period=0), dict(still_run=0), dict(still_run=1001), dict(flat_q=4081),
                dict(cut_pm=1001), dict(on=2), dict(gate=2), dict(max_cells=4095), dict(max_cells=262145), dict(slot_stream=[1])):
        with pytest.raises(gpu.VtError):
            gpu.op_frame_health([dev.frame], st, **dict(dict(cell=C, max_cells=CELLS), **bad))
