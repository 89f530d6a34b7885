"""The peak arbitration's rule (tests/arbitrate_util.py; the text: include/vittrack_hip_ops.h above vt_op_arbitrate) on
planted cases, on the CPU: every record status, every peak status, the tie on the chosen peak, a similarity exactly at `low`
and exactly at `high`, and the planted scene of the operator tests decided through the oracle's lists and the oracle's crops -
the statuses tests/test_gpu_arbitrate_op.py plans for are the ones the rule gives."""
import numpy as np
import pytest

import arbitrate_util as ar
import decode_util as du
from arbitrate_util import F

POL = dict(ar.DEFAULTS, on=1, radius=1)


def _lst(scores, boxes, cells=None):
    """a one-case list in iterate_oracle's layout"""
    n = len(scores)
    out = dict(n=np.array([n]), cell=np.full((1, ar.KMAX), -1, np.int64), score=np.zeros((1, ar.KMAX), F),
               resp=np.zeros((1, ar.KMAX), F), fbox=np.zeros((1, ar.KMAX, 4), F))
    out["score"][0, :n], out["fbox"][0, :n] = scores, boxes
    out["cell"][0, :n] = cells if cells is not None else np.arange(n)
    out["resp"][0, :n] = np.asarray(scores, F) * F(0.5)
    return out


@pytest.fixture(scope="module")
def geo(oracle):
    return oracle.crop_geometry(np.array(ar.PREV_BOX, F), 4.0, ar.S)


def _box(ix, iy, geo, dx=0.25, dy=-0.25):
    x, y = ar.cell_box(ix, iy, geo)
    return (x + dx, y + dy, 48.0, 48.0)


def _examine(lst, geo, **kw):
    a = dict(on=1, success=1, frames_done=7, window_miss=3, geo=geo, frame_wh=(ar.W, ar.H), T=ar.T, S=ar.S,
             success_threshold=ar.SUCCESS_THRESHOLD)
    a.update(kw)
    return ar.examine(lst, 0, **a)


def test_thresholds_are_one_binary32_divide():
    assert ar.threshold(300) == F(300) / F(1000) and ar.threshold(500) == F(0.5) and ar.threshold(0) == 0 and ar.threshold(1000) == 1
    assert ar.threshold(300) != np.float64(0.3) and float(ar.threshold(50)) == float(np.float32(0.05))


def test_integer_box_rounds_as_the_decode():
    assert list(ar.int_box([10.5, 10.49, 47.5, 48.5])) == [11.0, 10.0, 48.0, 49.0]
    assert list(ar.int_box([0.0, -0.0, 10.0, 319.999])) == [0.0, 0.0, 10.0, 320.0]


def test_not_due_and_candidate(oracle, geo):
    lst = _lst([0.9, 0.8], [_box(3, 3, geo), _box(5, 4, geo)])
    assert _examine(lst, geo)["status"] == ar.KEPT                      # the base case is due
    for kw in (dict(on=0), dict(success=0), dict(window_miss=7), dict(on=0, candidate=True)):
        ex = _examine(lst, geo, **kw)
        assert ex["status"] == ar.NOT_DUE and ex["n"] == 0 and ex["peak_status"] == [0] * 4 and not ex["mark"], kw
    ex = _examine(lst, geo, candidate=True)
    assert ex["status"] == ar.CANDIDATE and ex["n"] == 0 and not ex["mark"]
    # no runner-up at all, a runner-up below the threshold (exactly at it: eligible), a NaN score
    assert _examine(_lst([0.9], [_box(3, 3, geo)]), geo)["status"] == ar.NOT_DUE
    below = float(np.nextafter(F(ar.SUCCESS_THRESHOLD), F(0)))
    ex = _examine(_lst([0.9, below], [_box(3, 3, geo), _box(5, 4, geo)]), geo)
    assert ex["status"] == ar.NOT_DUE and ex["n"] == 2 and ex["peak_status"] == [0] * 4
    assert _examine(_lst([0.9, ar.SUCCESS_THRESHOLD], [_box(3, 3, geo), _box(5, 4, geo)]), geo)["status"] == ar.KEPT
    assert _examine(_lst([0.9, np.nan], [_box(3, 3, geo), _box(5, 4, geo)]), geo)["status"] == ar.NOT_DUE
    # peak 0 needs no score of its own: result.success decided
    assert _examine(_lst([0.1, 0.8], [_box(3, 3, geo), _box(5, 4, geo)]), geo)["status"] == ar.KEPT


def test_rule_6_at_peak_0_and_at_a_runner_up(oracle, geo):
    for cell in ((1, 3), (6, 3), (3, 1), (3, 6)):       # a 48-px box centred there leaves the search crop's taps
        assert ar.taps_rule(ar.int_box(_box(*cell, geo)), geo, ar.T, ar.S, (ar.W, ar.H)) == 6, cell
    for cell in ((2, 2), (5, 5), (2, 5), (5, 2)):
        assert ar.taps_rule(ar.int_box(_box(*cell, geo)), geo, ar.T, ar.S, (ar.W, ar.H)) == 0, cell
    ex = _examine(_lst([0.9, 0.8], [_box(1, 3, geo), _box(4, 4, geo)]), geo)
    assert ex["status"] == ar.RULE6 and ex["n"] == 2 and ex["peak_status"] == [0] * 4 and not ex["mark"]
    ex = _examine(_lst([0.9, 0.8, 0.7], [_box(3, 3, geo), _box(6, 4, geo), _box(5, 5, geo)]), geo)
    assert ex["status"] == ar.KEPT and ex["peak_status"] == [1, 2, 1, 0]
    ex = _examine(_lst([0.9, 0.8], [_box(3, 3, geo), _box(6, 4, geo)]), geo)           # the only runner-up fails rule 6
    assert ex["status"] == ar.NOT_DUE and ex["peak_status"] == [0, 2, 0, 0]


def test_rule_7_marks_a_window_miss_and_ends_the_examination(oracle, geo):
    window = (60, 30, 160, 170)
    inside, outside = _box(3, 3, geo), _box(5, 5, geo)
    assert ar.taps_rule(ar.int_box(inside), geo, ar.T, ar.S, (ar.W, ar.H), window) == 0
    assert ar.taps_rule(ar.int_box(outside), geo, ar.T, ar.S, (ar.W, ar.H), window) == 7
    ex = _examine(_lst([0.9, 0.8], [inside, outside]), geo, window=window)
    assert ex["status"] == ar.WINDOW_MISS and ex["mark"] and ex["peak_status"] == [0] * 4
    ex = _examine(_lst([0.9, 0.8], [outside, inside]), geo, window=window)              # at peak 0
    assert ex["status"] == ar.WINDOW_MISS and ex["mark"]
    ex = _examine(_lst([0.9, 0.3], [inside, outside]), geo, window=window)              # a runner-up that is not examined
    assert ex["status"] == ar.NOT_DUE and not ex["mark"]
    ex = _examine(_lst([0.9, 0.8, 0.7], [inside, _box(6, 4, geo), outside]), geo, window=window)     # rule 6 first, then on
    assert ex["status"] == ar.WINDOW_MISS
    # the in-frame part only: a crop that hangs over the frame's edge is no miss of the whole frame
    assert ar.taps_rule(np.array([0, 0, 48, 48], F), (-47.5, -47.5, 1.5, 192.0), ar.T, ar.S, (ar.W, ar.H)) == 0


def _commit(sims, ps=(1, 1, 1, 1), low=300, high=500):
    n = len(sims)
    return ar.commit(list(ps)[:n] + [0] * (ar.KMAX - n), {k: (1, F(v)) for k, v in enumerate(sims)}, n, low, high)[:2]


def test_switch_rule():
    assert _commit([0.1, 0.9]) == (ar.SWITCHED, 1)
    assert _commit([0.4, 0.9]) == (ar.KEPT, 0)                          # peak 0 is not challenged
    assert _commit([0.1, 0.4]) == (ar.KEPT, 0)                          # nobody reaches high
    assert _commit([0.1, 0.6, 0.9, 0.7]) == (ar.SWITCHED, 2)            # the largest similarity
    assert _commit([-1.0, 0.6, 0.5]) == (ar.SWITCHED, 1)
    assert _commit([0.1, 0.9], ps=(1, 2)) == (ar.KEPT, 0)               # rule 6 failed there: never scored, never chosen
    assert _commit([0.1, 0.2, 0.9], ps=(1, 1, 0)) == (ar.KEPT, 0)


def test_tie_takes_the_lowest_peak():
    assert _commit([0.1, 0.75, 0.75, 0.75]) == (ar.SWITCHED, 1)
    assert _commit([0.1, 0.5, 0.75, 0.75]) == (ar.SWITCHED, 2)
    assert _commit([0.1, 0.75, 0.5, 0.75]) == (ar.SWITCHED, 1)


def test_exactly_at_low_and_exactly_at_high():
    low, high = ar.threshold(300), ar.threshold(500)
    assert _commit([low, 0.9]) == (ar.KEPT, 0)                          # sim[0] < low is strict
    assert _commit([np.nextafter(low, F(0)), 0.9]) == (ar.SWITCHED, 1)
    assert _commit([0.1, high]) == (ar.SWITCHED, 1)                     # sim[k] >= high
    assert _commit([0.1, np.nextafter(high, F(0))]) == (ar.KEPT, 0)
    assert _commit([0.0, 0.0], low=0, high=0) == (ar.KEPT, 0)           # low 0 challenges nobody: the option is inert,
    assert _commit([-0.5, 0.9], low=0, high=0) == (ar.KEPT, 0)          # a negative similarity included
    assert _commit([-0.5, 0.0], low=1, high=0) == (ar.SWITCHED, 1)      # one per mille does
    assert _commit([0.999, 1.0], low=1000, high=1000) == (ar.SWITCHED, 1)


def test_a_flat_crop_has_no_similarity():
    """score status 3 (a variance is not positive): at peak 0 nothing is challenged, at a runner-up it is never chosen"""
    st, chosen, ps, sim = ar.commit([1, 1, 0, 0], {0: (3, F(0)), 1: (1, F(0.9))}, 2, 300, 500)
    assert (st, chosen, ps[:2]) == (ar.KEPT, 0, [3, 1])
    st, chosen, ps, sim = ar.commit([1, 1, 1, 0], {0: (1, F(0.1)), 1: (3, F(0)), 2: (1, F(0.6))}, 3, 300, 500)
    assert (st, chosen, ps[:3]) == (ar.SWITCHED, 2, [1, 3, 1]) and sim[1] == 0
    st, chosen, _, _ = ar.commit([1, 1, 0, 0], {0: (1, F(-0.2)), 1: (3, F(0))}, 2, 300, 0)       # high 0 is still not met by "no score"
    assert (st, chosen) == (ar.KEPT, 0)


def test_apply_rewrites_what_the_decode_writes(vt):
    import importlib
    STATE = importlib.import_module(vt.__name__ + ".snapshot").STATE
    st = du.make_states(np.array([[47.5, 17.5, 1.5, 192.0]], F), [ar.W], [ar.H], 5)
    before = st.copy()
    res = np.zeros(1, vt.RESULT_DTYPE)
    lst = _lst([0.9, 0.8125], [(100.25, 50.75, 48.5, 47.4), (160.5, 90.49, 47.5, 48.5)], cells=[19, 37])
    ar.apply(st[0], res[0], lst, 0, 1)
    assert res[0]["success"] == 1 and res[0]["score"] == F(0.8125) and list(res[0]["bbox"]) == [161, 90, 48, 49]
    assert list(st[0]["box"]) == [161.0, 90.0, 48.0, 49.0] and list(st[0]["last_fbox"]) == [F(160.5), F(90.49), F(47.5), F(48.5)]
    assert st[0]["last_score"] == F(0.8125) and st[0]["last_idx"] == 37
    for name in STATE.names:
        if name not in ("box", "last_fbox", "last_score", "last_idx"):
            assert np.array_equal(st[0][name], before[0][name]), name       # frames_done and success_count among them


# ---- the planted scene, through the oracle -----------------------------------------------------------------------------------

WANT = {    # K -> the record status of streams 0..4, (chosen)
    2: [(2, 1), (1, 0), (0, 0), (4, 0), (0, 0)],
    3: [(2, 1), (1, 0), (0, 0), (4, 0), (2, 2)],
    4: [(2, 1), (1, 0), (0, 0), (4, 0), (2, 2)],
}


@pytest.fixture(scope="module")
def planted(oracle, weights_tiny, geo):
    hdr = oracle.Model(weights_tiny).hdr
    assert (hdr["patch"], hdr["template"], hdr["search"], hdr["kpad"]) == (ar.PATCH, ar.T, ar.S, ar.KPAD)
    sc = ar.scene(geo)
    crop = lambda pic, box: oracle.preproc(oracle.Frame.rgb8(pic), np.asarray(box, F), 2.0, ar.T, ar.PATCH, ar.KPAD, hdr["norm_a"],
                                           hdr["norm_b"])
    return dict(sc, anchor=crop(sc["anchor_picture"], ar.ANCHOR_BOX), crop=crop, hann=ar.window())


@pytest.mark.parametrize("K", [2, 3, 4])
def test_the_planted_scene_gives_the_planned_statuses(planted, geo, K):
    B = len(ar.PLAN)
    pol = dict(POL, max_peaks=K)
    lst = ar.lists(planted["logits"], planted["hann"], ar.GRID, np.tile(geo, (B, 1)), [ar.W] * B, [ar.H] * B, K, pol["radius"],
                   pol["min_resp_pm"])
    for s in range(B):
        cells = [iy * ar.GRID + ix for ix, iy, _, _ in ar.PLAN[s]][:K]
        assert list(lst["cell"][s, :lst["n"][s]]) == cells, (s, lst["cell"][s])       # listed in the plan's order, nothing else
        state = dict(frames_done=5, window_miss=0, geo=geo)
        seen = {}

        def sims_of(k, ibox):
            seen[k] = ar.similarity(planted["anchor"], planted["crop"](planted["pictures"][s], ibox), ar.COLS)
            return seen[k]
        d = ar.decide(lst, s, sims_of, state=state, success=1, frame_wh=(ar.W, ar.H), T=ar.T, S=ar.S,
                      success_threshold=ar.SUCCESS_THRESHOLD, policy=pol)
        assert (d["status"], d["chosen"]) == WANT[K][s], (s, K, d, seen)
        low, high = float(ar.threshold(pol["low_pm"])), float(ar.threshold(pol["high_pm"]))
        for k, (st, v) in seen.items():     # no compared similarity near a threshold: the device's crops may differ in the last bit
            assert st == 1 and min(abs(float(v) - low), abs(float(v) - high)) >= 0.05, (s, k, v)
    with np.errstate(over="ignore"):
        lead, thr = __import__("peaks_util").margins(planted["logits"], planted["hann"], ar.GRID, K, pol["radius"],
                                                      float(ar.threshold(pol["min_resp_pm"])))
    assert lead.min() >= 1e-2 and thr.min() >= 1e-2, (lead, thr)


# ---- the committed clip (tests/golden/make_arbitrate.py -> arbitrate_tiny.npz) ------------------------------------------------

@pytest.fixture(scope="module")
def mk():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_make_arbitrate", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                                                  "make_arbitrate.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def clip(mk):
    return dict(np.load(mk.OUT))


def test_the_committed_clip_meets_the_generators_conditions(mk, clip, weights_tiny):
    mk.check(clip)
    assert str(clip["weights_sha256"]) == mk.sha256_file(weights_tiny), "the fixture was made with another weight blob"
    assert {k: int(clip[k]) for k in mk.POLICY} == mk.POLICY and tuple(clip["lookalike"]) == mk.LOOKALIKE and tuple(clip["hide"]) == mk.HIDE
    # the scene parameters only: the frames come from them
    assert not any(v.ndim >= 2 and v.shape[-1] == 3 and v.dtype == np.uint8 for v in clip.values())
    f = mk.frame(50, clip)
    assert f.shape == (mk.H, mk.W, 3) and np.array_equal(f, mk.frame(50))


def test_the_committed_records_follow_the_rule(clip):
    """every due update's status and chosen peak from its recorded peak statuses and similarities; one switch, and the
    arbitrated run is on the target again five updates ahead of the plain run"""
    st = clip["arb_status"]
    for t in np.flatnonzero((st == ar.KEPT) | (st == ar.SWITCHED)):
        n = int(clip["arb_n"][t])
        ps = [ar.P_SCORED if s in (ar.P_SCORED, ar.P_FLAT) else int(s) for s in clip["arb_peak_status"][t]]
        sims = {k: (1 if clip["arb_peak_status"][t, k] == ar.P_SCORED else 3, clip["arb_sim"][t, k]) for k in range(n)}
        got = ar.commit(ps, sims, n, int(clip["low_pm"]), int(clip["high_pm"]))
        assert got[:2] == (int(st[t]), int(clip["arb_chosen"][t])), (t, got)
    switches = np.flatnonzero(st == ar.SWITCHED)
    assert len(switches) == 1 and int(clip["first_arb"]) == switches[0] and int(clip["first_plain"]) - int(clip["first_arb"]) == 5
    t = int(switches[0])
    k = int(clip["arb_chosen"][t])
    assert tuple(clip["arb_bbox"][t]) == tuple(int(v) for v in ar.int_box(clip["arb_fbox"][t, k])) and clip["arb_success"][t] == 1
    assert clip["arb_score"][t] == clip["arb_peak_score"][t, k]
    assert np.array_equal(clip["plain_bbox"][:t], clip["arb_bbox"][:t])         # identical until the switch


def test_the_generator_reproduces_the_committed_file(mk, clip, tmp_path, capsys):
    out = str(tmp_path / "again.npz")
    mk.run(out)
    capsys.readouterr()
    again = dict(np.load(out))
    assert sorted(again) == sorted(clip)
    for k in clip:
        assert np.array_equal(again[k], clip[k]), k
