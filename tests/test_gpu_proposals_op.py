"""Reacquire proposals, operator level (vt_op_proposals: the four launches of csrc/k_proposals.hip alone), on the MI355X.

Every comparison is np.array_equal against the NumPy model of tests/proposals_util.py: pattern, thumbnail, similarity map
and records, bit for bit. The hook puts its outputs between guard bands and fills them with 0xff first: what a launch must
leave alone has to come back as 0xff. Frames are about 160x96, the target 32x32 (cells of 4x4 px at T = 64)."""
import numpy as np
import pytest

import proposals_util as pu
from test_proposals_cases import H, KPAD, M, NA, NB, PATCH, T, W, blocks, plant

pytestmark = pytest.mark.gpu

NORM = NA + NB
CELLS = 4096


def _states(gpu, boxes, frames_done=3, tpl_gen=0):
    import importlib
    st = np.zeros(len(boxes), importlib.import_module(gpu.__name__ + ".snapshot").STATE)
    for i, b in enumerate(boxes):
        st[i]["box"] = b
        st[i]["frames_done"] = frames_done
        st[i]["tpl_gen"] = tpl_gen
        st[i]["initialized"] = 1
    return st


def _results(gpu, success):
    r = np.zeros(len(success), gpu.RESULT_DTYPE)
    r["success"] = success
    return r


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(7)
    src = blocks(rng, T, T)
    tpl = src.astype(np.float32) * np.asarray(NA, np.float32) + np.asarray(NB, np.float32)
    noise = rng.normal(0, 0.02, tpl.shape).astype(np.float32)       # bf16 roundings that differ from pixel to pixel
    return dict(bg=blocks(rng, H, W), src=src, rows=pu.rows_from_template(tpl + noise, PATCH, KPAD))


def _one(gpu, scene, fmt, rgb, box=(5.0, 5.0, 32.0, 32.0), rows=None, T_=T, patch=PATCH, norm=NORM, **pol):
    h, w, _ = rgb.shape
    dev = pu.DevFrame(gpu, fmt, pu.from_rgb(fmt, rgb), w, h)
    rows = scene["rows"] if rows is None else rows
    pol.setdefault("max_cells", CELLS)
    got = gpu.op_proposals([dev.frame], _states(gpu, [box]), _results(gpu, [0]), rows[None, None], T_, patch, norm, **pol)
    want = pu.evaluate(dev.rgb, box, rows, T_, patch, norm[:3], norm[3:], max_cells=pol["max_cells"], max_n=pol.get("max_n", 4),
                       min_sim_pm=pol.get("min_sim_pm", 500))
    pu.check_slot(got, 0, 0, want, pol["max_cells"])
    assert got["evaluated"][0] == (1 if want["status"] in (1, 3) else 0)
    return got, want


@pytest.mark.parametrize("fmt", pu.FORMATS)
@pytest.mark.parametrize("size", [(W, H), (157, 93)])
def test_formats(gpu, scene, fmt, size):
    w, h = size
    if fmt == "yuy2":
        w &= ~1                      # packed pixel pairs: the one format that needs an even width
    rgb = plant(scene["bg"], scene["src"], 60, 28)[:h, :w]
    got, want = _one(gpu, scene, fmt, rgb, min_sim_pm=300)
    assert want["status"] == 1 and len(want["proposals"]) >= 1


@pytest.mark.parametrize("w", [152, 156, 160, 32])
def test_grid_widths_around_the_match_tile(gpu, scene, w):
    """Wg - M + 1 = 31, 32, 33 positions in a row (the tile is 32 wide), and Wg == M: a single column of positions"""
    rgb = plant(scene["bg"], scene["src"], 60, 28)[:, :w] if w > 32 else scene["src"][16:48, 16:48]
    got, want = _one(gpu, scene, "rgb8", rgb, min_sim_pm=0)
    assert want["Wg"] - M + 1 == {152: 31, 156: 32, 160: 33, 32: 1}[w]
    if w == 32:
        assert want["map"].shape == (1, 1)


def test_vitl14_template(gpu, scene):
    rng = np.random.default_rng(3)
    tpl = rng.normal(0, 1, (196, 196, 3)).astype(np.float32) + np.kron(rng.normal(0, 1, (14, 14, 3)), np.ones((14, 14, 1))).astype(np.float32)
    rows = pu.rows_from_template(tpl, 14, 640)
    got, want = _one(gpu, scene, "nv12", scene["bg"], box=(40.0, 20.0, 30.0, 34.0), rows=rows, T_=196, patch=14, min_sim_pm=0)
    assert want["M"] == 14 and want["status"] == 1 and want["c"] != np.float32(4)


def test_tie_and_suppression_boundary(gpu, scene):
    f = plant(plant(scene["bg"], scene["src"], 92, 16), scene["src"], 16, 20)
    got, want = _one(gpu, scene, "rgb8", f)
    assert want["proposals"]["sim"][0].tobytes() == want["proposals"]["sim"][1].tobytes()
    for dist in (M // 2, M // 2 + 1):
        f = plant(plant(scene["bg"], scene["src"], 32, 32), scene["src"], 32 + 4 * dist, 32)
        _one(gpu, scene, "rgb8", f, min_sim_pm=0, max_n=8)


def test_saturation_flat_and_max_cells(gpu, scene):
    f = scene["bg"].copy()
    f[:48] = 255
    f[48:] = 0
    hot = pu.rows_from_template(np.where(np.arange(T)[:, None, None] < 32, 1e30, -1e30) * np.ones((T, T, 3)), PATCH, KPAD)
    got, want = _one(gpu, scene, "rgb8", f, rows=hot, norm=(1e6, 1e6, 1e6, -1e8, -1e8, -1e8), min_sim_pm=0)
    assert set(np.unique(want["thumb"])) == {pu.OUTSIDE, -32767, 32767}
    got, want = _one(gpu, scene, "rgb8", np.full((H, W, 3), 77, np.uint8))
    assert want["status"] == 1 and len(want["proposals"]) == 0
    flat = pu.rows_from_template(np.full((T, T, 3), 0.25, np.float32), PATCH, KPAD)
    got, want = _one(gpu, scene, "rgb8", scene["bg"], rows=flat)
    assert want["status"] == 3
    cells = (W // 4 + 8) * (H // 4 + 8)
    assert _one(gpu, scene, "rgb8", scene["bg"], max_cells=cells)[1]["status"] == 1
    assert _one(gpu, scene, "rgb8", scene["bg"], max_cells=cells - 1)[1]["status"] == 2
    assert _one(gpu, scene, "rgb8", scene["bg"], box=(0.0, 0.0, 400.0, 400.0))[1]["status"] == 2
    assert _one(gpu, scene, "rgb8", scene["bg"], box=(0.0, 0.0, 0.0, 10.0))[1]["status"] == 2


@pytest.mark.parametrize("n", [1, 3, 30])
def test_slots_with_only_some_due(gpu, scene, n):
    """mode 1: the slots whose update succeeded are not due; a subset map; two template buffers chosen by tpl_gen; a
    windowed frame and a stream outside the pass"""
    rng = np.random.default_rng(n)
    ns = n + 1                                              # the last stream is in no slot
    fmts = ["rgb8", "nv12", "i420"]
    pics = [plant(scene["bg"], scene["src"], 20 + 24 * k, 12 + 16 * k) for k in range(3)]
    devs = [pu.DevFrame(gpu, fmts[k], pu.from_rgb(fmts[k], pics[k]), W, H) for k in range(3)]
    slot_stream = rng.permutation(n).astype(np.int32)
    success = (np.arange(n) % 3 == 1).astype(np.int32)
    boxes = [(5.0, 5.0, 32.0, 32.0 if s % 2 == 0 else 30.0) for s in range(ns)]
    st = _states(gpu, boxes)
    st["tpl_gen"] = np.arange(ns) % 3
    other = pu.rows_from_template(pu.template_from_rows(scene["rows"], T, PATCH)[::-1].astype(np.float32), PATCH, KPAD)
    tpl = np.stack([np.stack([scene["rows"], other]) for _ in range(ns)])
    frames = [devs[i % 3].frame for i in range(n)]
    windowed = n - 1 if n > 1 else None
    if windowed is not None:                                # the same planes, declared a window of the frame
        f = devs[windowed % 3].frame
        frames[windowed] = gpu.CFrame(f.plane0, f.plane1, f.width, f.height, f.stride0, f.stride1, f.format, 0, 0, 1, W - 2, H - 2)
    got = gpu.op_proposals(frames, st, _results(gpu, success), tpl, T, PATCH, NORM, mode=1, min_sim_pm=300, max_cells=CELLS,
                           slot_stream=slot_stream, tpl_bufs=2)
    for i in range(n):
        s = int(slot_stream[i])
        rows = tpl[s, int(st[s]["tpl_gen"]) & 1]
        if success[i]:
            want = dict(status=0, M=M, pattern=None, thumb=None, map=None, proposals=np.zeros(0, pu.REC_DTYPE))
        elif i == windowed:
            want = dict(status=4, M=M, pattern=None, thumb=None, map=None, proposals=np.zeros(0, pu.REC_DTYPE))
        else:
            want = pu.evaluate(devs[i % 3].rgb, boxes[s], rows, T, PATCH, NA, NB, max_cells=CELLS, min_sim_pm=300)
            assert want["status"] == 1
        pu.check_slot(got, i, s, want, CELLS)
        assert got["records"][s]["frames_done"] == 3
        assert got["evaluated"][s] == (1 if want["status"] == 1 else 0)
    assert (np.frombuffer(got["records"][ns - 1].tobytes(), np.uint8) == 0xff).all() and got["evaluated"][ns - 1] == 0


def test_host_pass_and_candidate_losers(gpu, scene):
    dev = pu.DevFrame(gpu, "rgb8", pu.from_rgb("rgb8", scene["bg"]), W, H)
    st = _states(gpu, [(5.0, 5.0, 32.0, 32.0)] * 2)
    tpl = np.stack([scene["rows"][None]] * 2)
    none = dict(M=M, pattern=None, thumb=None, map=None, proposals=np.zeros(0, pu.REC_DTYPE))
    got = gpu.op_proposals([dev.frame] * 2, st, _results(gpu, [0, 0]), tpl, T, PATCH, NORM, max_cells=CELLS, device_frames=False)
    for i in range(2):
        pu.check_slot(got, i, i, dict(status=4, **none), CELLS)
    # a candidate pass: three slots of stream 1, slot 2 wins - the record is the winner's, the losers run nothing
    got = gpu.op_proposals([dev.frame] * 3, st, _results(gpu, [0, 0, 0]), tpl, T, PATCH, NORM, max_cells=CELLS,
                           slot_stream=[1, 1, 1], winner=[2, 2, 2], min_sim_pm=0)
    want = pu.evaluate(dev.rgb, (5.0, 5.0, 32.0, 32.0), scene["rows"], T, PATCH, NA, NB, max_cells=CELLS, min_sim_pm=0)
    pu.check_slot(got, 2, 1, want, CELLS)
    for i in (0, 1):
        assert (got["pattern"][i] == -1).all() and (got["thumb"][i] == -1).all()
    assert (np.frombuffer(got["records"][0].tobytes(), np.uint8) == 0xff).all()
    # the period: frames_done 3 is not due at period 2
    got = gpu.op_proposals([dev.frame], st[:1], _results(gpu, [0]), tpl[:1], T, PATCH, NORM, max_cells=CELLS, period=2)
    pu.check_slot(got, 0, 0, dict(status=0, **none), CELLS)
