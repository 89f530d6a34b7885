"""Peak arbitration, operator level (vt_op_arbitrate: the four launches of csrc/k_arbitrate.hip alone), on the MI355X.

Every comparison is bit for bit, each launch against the existing piece it restates:
  * the lists against vt_op_response_peaks on the same operands;
  * the probe rows against the "template" tensor of a helper engine after vt_group_init_device at the peak's integer box;
  * the similarities against vt_op_appearance_score on those rows;
  * the record, the counters, the rewritten result and state and the three pinned mirrors against the NumPy rule of
    tests/arbitrate_util.py fed with those lists and similarities.
What no launch may touch comes back as the 0xff bytes the hook starts from; the hook itself reports a changed guard byte or a
ticket left non-zero as an error. The scene is arbitrate_util's planted one (320 x 240, the tiny model's shapes), whose planned
statuses tests/test_arbitrate_cases.py derives from the oracle alone."""
import importlib

import numpy as np
import pytest

import arbitrate_util as ar
import proposals_util as pu
from arbitrate_util import F
from test_gpu_planar_formats import _device

pytestmark = pytest.mark.gpu

B = len(ar.PLAN)
SLOTS = {"one": [0], "two of five": [3, 0], "five": None, "five shuffled": [4, 2, 0, 1, 3]}
FILL = 0xA5


@pytest.fixture(scope="module")
def model(gpu, oracle, weights_tiny):
    hdr = oracle.Model(weights_tiny).hdr
    assert (hdr["patch"], hdr["template"], hdr["search"], hdr["kpad"]) == (ar.PATCH, ar.T, ar.S, ar.KPAD)
    geo = oracle.crop_geometry(np.array(ar.PREV_BOX, F), 4.0, ar.S)
    helper = gpu.Group(weights_tiny, n_streams=1)
    yield dict(norm=list(hdr["norm_a"]) + list(hdr["norm_b"]), geo=geo, helper=helper, scene=ar.scene(geo), hann=ar.window())
    helper.close()


def _rows(g):
    return (g.read_tensor("template", 0).view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(ar.T // ar.PATCH * (ar.T // ar.PATCH), ar.KPAD)


def _cut(gpu, model, frame, ibox):
    """the template rows vt_group_init_device writes at the integer box"""
    model["helper"].init_device(0, frame, gpu.BBox.new(*(int(v) for v in ibox)))
    return _rows(model["helper"])


def _frames(gpu, model, fmt, window=None):
    out = []
    for s in range(B):
        out.append(_device(gpu, fmt, pu.from_rgb(fmt, model["scene"]["pictures"][s]), ar.W, ar.H, window=window))
    return out


def _states(gpu, model, oracle_lists):
    """the states and results a decode of the scene's logits leaves: peak 0 committed"""
    STATE = importlib.import_module(gpu.__name__ + ".snapshot").STATE
    st = np.zeros(B, STATE)
    res = np.zeros(B, gpu.RESULT_DTYPE)
    for s in range(B):
        ib = ar.int_box(oracle_lists["fbox"][s, 0])
        st[s]["box"], st[s]["geo"], st[s]["frame_w"], st[s]["frame_h"], st[s]["initialized"] = ib, model["geo"], ar.W, ar.H, 1
        st[s]["frames_done"], st[s]["success_count"], st[s]["window_miss"] = 5 + s, 4, 2
        st[s]["last_fbox"], st[s]["last_score"], st[s]["last_idx"] = oracle_lists["fbox"][s, 0], oracle_lists["score"][s, 0], oracle_lists["cell"][s, 0]
        st[s]["tpl_gen"], st[s]["tpl_frame"] = 1, 3
        res[s]["success"], res[s]["score"], res[s]["bbox"] = 1, oracle_lists["score"][s, 0], ib.astype(np.int32)
    return st, res


def _filled(n, dtype):
    return np.frombuffer(bytes([FILL]) * (n * dtype.itemsize), dtype).copy()


def _run_and_check(gpu, model, fmt, streams, K, *, window=None, winner=None, on=1, edit=None, low_pm=300, high_pm=500, tier=0):
    """one call of the hook on the slots `streams` (None: all, the identity map) and every comparison of the module's
    docstring -> the records by stream"""
    pol = dict(on=on, max_peaks=K, radius=1, min_resp_pm=50, low_pm=low_pm, high_pm=high_pm)
    slots = list(range(B)) if streams is None else streams
    n = len(slots)
    frames = _frames(gpu, model, fmt, window)
    ns = ar.GRID * ar.GRID
    ho = np.zeros((n * ns, 8), np.float32)
    ho[:, :5] = model["scene"]["logits"][slots].reshape(-1, 5)
    geo = np.tile(model["geo"], (B, 1))
    ora = ar.lists(model["scene"]["logits"], model["hann"], ar.GRID, geo, [ar.W] * B, [ar.H] * B, 1, 1, 50)
    st, res = _states(gpu, model, ora)
    if edit:
        edit(st, res)
    slot_res = res[slots].copy()
    anchor_frame = _device(gpu, fmt, pu.from_rgb(fmt, model["scene"]["anchor_picture"]), ar.W, ar.H)
    anchor = np.stack([_cut(gpu, model, anchor_frame[0], ar.ANCHOR_BOX)] * B)
    smap = None if streams is None else np.array(slots, np.int32)
    win = None if winner is None else np.array(winner, np.int32)
    cnt0 = np.zeros(B, gpu.ARBITRATE_COUNT_DTYPE)
    cnt0["evaluated"], cnt0["switched"] = 10 + np.arange(B), 3
    hres, hst, hrec = _filled(n, gpu.RESULT_DTYPE), _filled(B, st.dtype), _filled(B, gpu.ARBITRATE_REC_DTYPE)
    got = gpu.op_arbitrate(ho, model["hann"], [frames[s][0] for s in slots], st, slot_res, anchor, ar.GRID, ar.T, ar.S, ar.PATCH,
                           model["norm"], ar.SUCCESS_THRESHOLD, slot_stream=smap, winner=win, counts=cnt0, tier=tier,
                           host_results=hres, host_states=hst, host_records=hrec, **pol)
    # ---- 1. the lists: the response-peaks launch on the same operands ----
    peaks = gpu.op_response_peaks(ho, model["hann"], st, (K, 1, float(ar.threshold(50))), n, ar.GRID, slot_stream=smap)["records"]
    lst = ar.lists_of_records(peaks, K)
    want_st, want_res, want_cnt = st.copy(), slot_res.copy(), cnt0.copy()
    want_hst, want_hres = hst.copy(), hres.copy()
    ff = np.frombuffer(bytes([0xff]) * gpu.ARBITRATE_REC_DTYPE.itemsize, gpu.ARBITRATE_REC_DTYPE)[0]
    statuses = {}
    for i, s in enumerate(slots):
        rec = got["records"][s]
        if winner is not None and winner[i] != i:
            continue                                    # a candidate pass's losing slot writes nothing
        cut = {}

        def sims_of(k, ibox):
            cut[k] = _cut(gpu, model, frames[s][0], ibox)
            one = gpu.op_appearance_score(anchor[s][None], cut[k][None], ar.COLS)
            return int(one["status"][0]), one["similarity"][0]
        d = ar.decide(lst, i, sims_of, state=st[s], success=int(slot_res[i]["success"]), frame_wh=(ar.W, ar.H), T=ar.T, S=ar.S,
                      success_threshold=ar.SUCCESS_THRESHOLD, policy=pol, window=window, candidate=winner is not None)
        statuses[s] = (d["status"], d["chosen"])
        # ---- 4. the record against the rule ----
        assert (rec["status"], rec["frames_done"], rec["n"], rec["chosen"]) == (d["status"], st[s]["frames_done"], d["n"], d["chosen"]), (s, rec, d)
        for k in range(ar.KMAX):
            p = rec["peak"][k]
            if k >= d["n"]:
                assert not np.frombuffer(p.tobytes(), np.uint8).any(), (s, k)
                continue
            q = peaks[i]["peak"][k]
            assert (p["cell"], p["score"].tobytes(), p["resp"].tobytes(), p["box"].tobytes()) == \
                   (q["cell"], q["score"].tobytes(), q["resp"].tobytes(), q["box"].tobytes()), (s, k, p, q)
            assert p["status"] == d["peak_status"][k] and p["reserved"] == 0, (s, k, p, d)
            # ---- 3. the similarity: the appearance score's bits ----
            assert p["similarity"].tobytes() == F(d["sim"][k]).tobytes(), (s, k, p["similarity"], d["sim"][k])
            # ---- 2. the probe rows: vt_group_init_device at that box ----
            if k in cut:
                assert np.array_equal(got["probe"][s, k], cut[k]), (s, k)
            else:
                assert (got["probe"][s, k] == 0xffff).all(), (s, k)
        assert (got["probe"][s, d["n"]:] == 0xffff).all()
        if d["status"] in (ar.KEPT, ar.SWITCHED):
            want_cnt[s]["evaluated"] += 1
            want_cnt[s]["switched"] += d["status"] == ar.SWITCHED
        if d["status"] == ar.SWITCHED:
            ar.apply(want_st[s], want_res[i], lst, i, d["chosen"])
            want_hres[i] = want_res[i]
            for name in ("box", "last_fbox", "last_score", "last_idx"):
                want_hst[s][name] = want_st[s][name]
        if d["mark"]:
            want_st[s]["window_miss"] = want_hst[s]["window_miss"] = st[s]["frames_done"]
        assert got["host_records"][s].tobytes() == rec.tobytes(), s                     # every record ends final and mirrored
    for s in range(B):
        if s not in statuses:                           # a stream no working slot names: record and rows untouched
            assert got["records"][s].tobytes() == ff.tobytes() and (got["probe"][s] == 0xffff).all(), s
            assert got["host_records"][s].tobytes() == bytes([FILL]) * gpu.ARBITRATE_REC_DTYPE.itemsize, s
    assert got["states"].tobytes() == want_st.tobytes() and got["results"].tobytes() == want_res.tobytes()
    assert got["host_states"].tobytes() == want_hst.tobytes() and got["host_results"].tobytes() == want_hres.tobytes()
    assert got["counts"].tobytes() == want_cnt.tobytes()
    return statuses


@pytest.mark.parametrize("fmt", ["rgb8", "nv12", "i420"])
@pytest.mark.parametrize("slots", list(SLOTS))
def test_every_launch_against_the_piece_it_restates(gpu, model, fmt, slots):
    seen = set()
    for K in (2, 4):
        st = _run_and_check(gpu, model, fmt, SLOTS[slots], K)
        seen |= {v[0] for v in st.values()}
        want = {0: (2, 1), 1: (1, 0), 2: (0, 0), 3: (4, 0), 4: (0, 0) if K == 2 else (2, 2)}
        assert st == {s: want[s] for s in st}, (K, st)        # the plan test_arbitrate_cases.py derives from the oracle
    if SLOTS[slots] is None or len(SLOTS[slots]) == B:
        assert seen == {0, 1, 2, 4}


def test_three_peaks_and_the_other_crop_tiers(gpu, model):
    for tier in (1, 2):
        st = _run_and_check(gpu, model, "nv12", None, 3, tier=tier)
        assert st[4] == (2, 2) and st[0] == (2, 1)


def test_a_candidate_pass_leaves_status_3_and_nothing_else(gpu, model):
    st = _run_and_check(gpu, model, "nv12", [0, 0, 1], 4, winner=[1, 1, 2])
    assert st == {0: (3, 0), 1: (3, 0)}
    st = _run_and_check(gpu, model, "nv12", [0, 0, 1], 4, winner=[1, 1, 2], on=0)
    assert st == {0: (0, 0), 1: (0, 0)}


def test_a_window_miss_is_marked_and_nothing_is_cut(gpu, model):
    """a stored window that ends at x = 219 cuts the template taps of stream 0's runner-up (cell (5, 4): taps to x = 228)
    and leaves stream 1's peaks whole; one that ends at x = 189 cuts stream 1's peak 0 (cell (4, 3): taps to x = 204). Rule 7
    there: status 5, the mark in the state and its mirror, nothing cut"""
    st = _run_and_check(gpu, model, "nv12", None, 4, window=(40, 10, 180, 220))
    assert st[0] == (5, 0) and st[1] == (1, 0) and st[3] == (4, 0), st
    st = _run_and_check(gpu, model, "rgb8", [1], 2, window=(40, 10, 150, 220))        # peak 0 itself
    assert st == {1: (5, 0)}


def test_not_due_slots_and_the_policy_off(gpu, model):
    def fail_and_miss(st, res):
        res[0]["success"] = 0                           # a failed update
        st[1]["window_miss"] = st[1]["frames_done"]     # this pass missed its window: the redo arbitrates
    st = _run_and_check(gpu, model, "rgb8", None, 4, edit=fail_and_miss)
    assert st[0] == (0, 0) and st[1] == (0, 0) and st[4] == (2, 2)
    assert set(_run_and_check(gpu, model, "rgb8", None, 4, on=0).values()) == {(0, 0)}


def test_thresholds_move_the_decision(gpu, model):
    """low 0: no similarity is below it - every due slot keeps peak 0; low and high 1000: stream 1's matching peak 0 is
    challenged too, and no runner-up reaches 1"""
    st = _run_and_check(gpu, model, "nv12", None, 4, low_pm=0)
    assert st[0] == (1, 0) and st[4] == (1, 0)
    st = _run_and_check(gpu, model, "nv12", None, 4, low_pm=1000, high_pm=1000)
    assert st[0] == (1, 0) and st[1] == (1, 0)
    st = _run_and_check(gpu, model, "nv12", None, 4, low_pm=1000, high_pm=0)            # whoever scores highest among the runner-ups
    assert st[0] == (2, 1)


def test_bad_arguments(gpu, model):
    with pytest.raises(gpu.VtError) as ei:
        _run_and_check(gpu, model, "rgb8", [0], 5)
    assert ei.value.code == -1 and "arbitrate_max" in str(ei.value)
    with pytest.raises(gpu.VtError) as ei:
        _run_and_check(gpu, model, "rgb8", [0], 1)
    assert ei.value.code == -1 and "arbitrate_max" in str(ei.value)
    with pytest.raises(gpu.VtError) as ei:
        _run_and_check(gpu, model, "rgb8", [2, 0, 2], 2)
    assert ei.value.code == -1 and "named by two slots" in str(ei.value)
