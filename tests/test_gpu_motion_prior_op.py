"""The two launches of the motion prior alone (vt_op_motion_prior: k_motion.hip's place and settle on the caller's operands),
on the MI355X, against the NumPy-float32 model of tests/motion_prior_util.py: the known-answer cases of
tests/test_motion_prior_cases.py, a subset list whose slots are not their streams, the candidate form with a losing slot and an
uninitialised listed stream, and 1024 slots. States, records and the pinned mirrors are compared byte for byte; every word
the rule does not name - other streams' states and records, the state's other 18 words - must come back as it went in."""
import numpy as np
import pytest

import motion_prior_util as mu

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 640, 480


def _states(vt, boxes, init=None, seed=0):
    """STATE records with recognisable junk in every word the rule must not touch"""
    from gstreamer_vit_tracker_amd.snapshot import STATE
    rng = np.random.default_rng(seed)
    st = np.frombuffer(rng.integers(1, 2 ** 30, len(boxes) * 22, dtype=np.int32).tobytes(), STATE).copy()
    for i, b in enumerate(boxes):
        st[i]["box"] = b
        st[i]["frame_w"], st[i]["frame_h"] = W, H
        st[i]["initialized"] = 1 if init is None else init[i]
    return st


def _recs(vt, recs):
    out = np.zeros(len(recs), vt.MOTION_REC_DTYPE)
    out.view(np.uint32).reshape(len(recs), mu.REC_WORDS)[:] = [r.words() for r in recs]
    return out


def _results(vt, success, scores=None):
    r = np.zeros(len(success), vt.RESULT_DTYPE)
    r["success"] = success
    r["score"] = 0.5 if scores is None else scores
    r["bbox"] = 7
    return r


def _model(pol, states, recs, results, stages, slot_stream=None, cands=None, winner=None, after_boxes=None):
    """what the launches must leave: (states, records, host box words by stream or None where untouched)"""
    st, rc = states.copy(), [r.copy() for r in recs]
    n = len(results)
    smap = list(range(n)) if slot_stream is None and cands is None else [int(c["stream"]) for c in cands] if cands is not None else list(slot_stream)
    touched = {}
    if stages & 1:
        for s in dict.fromkeys(smap):
            if st[s]["initialized"]:
                st[s]["box"] = mu.place(pol, rc[s], st[s]["box"], int(st[s]["frame_w"]), int(st[s]["frame_h"]))
    if after_boxes is not None:         # what a decode between the two launches would have written
        for s, b in after_boxes.items():
            st[s]["box"] = b
    if stages & 2:
        for i, s in enumerate(smap):
            if winner is not None and winner[i] != i:
                continue
            if not st[s]["initialized"]:
                continue
            hb = bool(cands[i]["has_box"]) if cands is not None else False
            st[s]["box"] = mu.settle(pol, rc[s], st[s]["box"], bool(results[i]["success"]), hb)
            touched[s] = True
    return st, rc, touched


def _run_and_compare(vt, pol, states, recs, results, stages=3, **kw):
    from gstreamer_vit_tracker_amd.snapshot import STATE
    n_s = len(states)
    fill_s = np.frombuffer(b"\xa5" * (n_s * 88), STATE).copy()
    fill_r = np.frombuffer(b"\x5a" * (n_s * 48), vt.MOTION_REC_DTYPE).copy()
    out = vt.op_motion_prior(states, _recs(vt, recs), results, *pol.tuple(), stages=stages, host_states=fill_s, host_records=fill_r, **kw)
    want_s, want_r, touched = _model(pol, states, recs, results, stages, kw.get("slot_stream"), kw.get("cands"), kw.get("winner"))
    assert out["states"].tobytes() == want_s.tobytes(), "device states differ from the model"
    assert out["records"].tobytes() == _recs(vt, want_r).tobytes(), "device records differ from the model"
    # the mirrors: the final box and the record of every stream that settled, nothing else
    hs, hr = fill_s.copy(), fill_r.copy()
    for s in touched:
        hs[s]["box"] = want_s[s]["box"]
        hr[s] = _recs(vt, want_r)[s]
    assert out["host_states"].tobytes() == hs.tobytes(), "the pinned state mirror holds a word the rule does not write"
    assert out["host_records"].tobytes() == hr.tobytes(), "the pinned record mirror differs"
    return out, want_s, want_r


def test_known_answer_cases_in_one_launch_each(gpu):
    """one stream per case, both launches in one call (nothing sits between them, so settle sees the placed box as the
    decode's): EMA with gain 33, the clamp on both signs, the in-frame test on its four sides and just inside, live counting
    down, the restore, a failed (NaN-scored) update, the flag off"""
    cases = [   # (box, record before, success)
        ((100, 50, 20, 30), mu.Record(v=(3.3000002, -0.99), live=5), 1),
        ((100, 50, 20, 30), mu.Record(), 1),
        ((100, 100, 16, 25), mu.Record(v=(300, -300), live=1), 1),
        ((100, 100, 16, 25), mu.Record(v=(-300, 300), prior=(900, 900, 16, 25), live=1), 1),
        ((10, 100, 20, 20), mu.Record(v=(-30, 0), live=4, n_shift=7), 1),
        ((100, 5, 20, 20), mu.Record(v=(0, -25), live=4), 0),
        ((605, 100, 20, 20), mu.Record(v=(25, 0), live=4), 1),
        ((100, 458, 20, 20), mu.Record(v=(0, 12), live=4), 0),
        ((10, 100, 20, 20), mu.Record(v=(-20, 0), live=4), 1),
        ((605, 100, 20, 20), mu.Record(v=(24.5, 0), live=4), 0),
        ((108, 96, 20, 20), mu.Record(v=(8, -4), live=2, n_coast=3), 0),
        ((108, 96, 20, 20), mu.Record(v=(8, -4), live=0, n_shift=2), 0),
        ((50, 50, 20, 20), mu.Record(v=(0, 0), live=0), 0),
        ((77.5, 33.25, 21, 19), mu.Record(v=(1.3, 2.7), live=60), 1),
    ]
    n = len(cases)
    st = _states(gpu, [c[0] for c in cases])
    recs = [c[1] for c in cases]
    scores = np.array([0.9 if c[2] else np.nan for c in cases], F)
    res = _results(gpu, [c[2] for c in cases], scores)
    for pol in (mu.Policy(1, 33, 5, 200), mu.Policy(1, 100, 2, 50), mu.Policy(1, 50, 0, 100), mu.Policy(1, 1, 60, 0), mu.Policy(0, 50, 5, 100)):
        for stages in (1, 2, 3):
            _run_and_compare(gpu, pol, st, recs, res, stages=stages)
    # the cases are not vacuous under the first policy: boxes moved, velocities dropped, a box restored, counters advanced
    out, ws, wr = _run_and_compare(gpu, mu.Policy(1, 33, 5, 200), st, recs, res)
    assert sum(r.n_shift for r in wr) - sum(r.n_shift for r in recs) == 6
    assert wr[4].v.tolist() == [0, 0] and wr[4].live == 5 and wr[5].live == 0
    assert ws[11]["box"].tolist() == [108, 96, 20, 20] and wr[11].v.tolist() == [0, 0] and wr[10].n_coast == 4
    # settle alone: d is taken from the record's prior - far below and far above the box - and clamped on both signs
    out, ws, wr = _run_and_compare(gpu, mu.Policy(1, 100, 2, 50), st, recs, res, stages=2)
    assert wr[2].v.tolist() == [10, 10] and wr[3].v.tolist() == [-10, -10]
    assert n <= 1024


def test_a_settle_behind_a_moved_box_matches_the_ema(gpu):
    """place, then the box a decode would have left, then settle: the velocity is taken from the PRIOR's centre"""
    pol = mu.Policy(1, 33, 5, 200)
    st = _states(gpu, [(110, 47, 20, 30), (200, 200, 31, 17)])
    recs = [mu.Record(v=(3.3000002, -0.99), live=5), mu.Record(v=(-6.25, 9.125), live=1)]
    res = _results(gpu, [1, 1])
    placed = gpu.op_motion_prior(st, _recs(gpu, recs), res, *pol.tuple(), stages=1)
    ws, wr, _ = _model(pol, st, recs, res, 1)
    assert placed["states"].tobytes() == ws.tobytes() and placed["records"].tobytes() == _recs(gpu, wr).tobytes()
    after = placed["states"].copy()
    after[0]["box"], after[1]["box"] = (121, 44, 20, 30), (188, 215, 29, 19)
    out = gpu.op_motion_prior(after, placed["records"], res, *pol.tuple(), stages=2)
    ws2, wr2, _ = _model(pol, after, wr, res, 2)
    assert out["states"].tobytes() == ws2.tobytes() and out["records"].tobytes() == _recs(gpu, wr2).tobytes()
    assert [float(x) for x in wr2[0].v] == [5.841000556945801, -1.6533000469207764], "the model itself moved"


def test_a_subset_list_whose_slots_are_not_their_streams(gpu):
    n_s = 7
    boxes = [(40 + 30 * s, 60 + 20 * s, 20 + s, 24) for s in range(n_s)]
    st = _states(gpu, boxes, seed=3)
    recs = [mu.Record(v=(2.5 * (s - 3), -1.5 * s), live=s % 3) for s in range(n_s)]
    lst = [5, 0, 3]
    res = _results(gpu, [1, 0, 0])
    for stages in (1, 2, 3):
        out, ws, wr = _run_and_compare(gpu, mu.Policy(1, 70, 5, 200), st, recs, res, stages=stages, slot_stream=lst)
        for s in set(range(n_s)) - set(lst):
            assert out["states"][s].tobytes() == st[s].tobytes() and out["records"][s].tobytes() == _recs(gpu, recs)[s].tobytes()
    assert ws[5]["box"].tolist() != st[5]["box"].tolist()


def test_the_candidate_form_losers_placed_winners_and_an_uninitialised_stream(gpu):
    """slots: stream 2 three times (own box twice, a caller's box once), stream 0 once with a caller's box that wins, stream 4
    (uninitialised) once, stream 1 plain. Place works once per stream; only winners settle, with their own has_box"""
    n_s = 6
    boxes = [(40 + 30 * s, 60 + 20 * s, 20, 24) for s in range(n_s)]
    st = _states(gpu, boxes, init=[1, 1, 1, 1, 0, 1], seed=5)
    recs = [mu.Record(v=(4 + s, -3), live=2) for s in range(n_s)]
    cands = np.zeros(6, gpu.CANDIDATE_DTYPE)
    cands["stream"] = [2, 0, 2, 4, 2, 1]
    cands["has_box"] = [0, 1, 1, 0, 0, 0]
    cands["box"][1], cands["box"][2] = (300, 200, 22, 18), (10, 10, 20, 20)
    for winner, success in (([4, 1, 4, 3, 4, 5], [1, 1, 1, 1, 1, 0]),      # an own-box slot of stream 2 wins: its velocity learns
                            ([2, 1, 2, 3, 2, 5], [0, 1, 1, 0, 1, 1]),      # the placed slot of stream 2 wins: velocity reset
                            ([0, 1, 0, 3, 0, 5], [0, 0, 1, 1, 1, 1])):     # failing winners: coast
        res = _results(gpu, success)
        for stages in (1, 2, 3):
            out, ws, wr = _run_and_compare(gpu, mu.Policy(1, 70, 5, 200), st, recs, res, stages=stages, cands=cands, winner=winner)
            assert out["states"][4].tobytes() == st[4].tobytes(), "an uninitialised stream's state was written"
            assert out["records"][4].tobytes() == _recs(gpu, recs)[4].tobytes(), "an uninitialised stream's record was written"
            assert out["states"][3].tobytes() == st[3].tobytes() and out["states"][5].tobytes() == st[5].tobytes()
    assert wr[2].n_shift == 1, "place ran more than once for a stream named by three slots"


def test_1024_slots_in_reverse_order(gpu):
    n = 1024
    rng = np.random.default_rng(11)
    boxes = np.stack([rng.uniform(30, 560, n), rng.uniform(30, 400, n), rng.uniform(10, 40, n), rng.uniform(10, 40, n)], 1).astype(F)
    st = _states(gpu, boxes, seed=9)
    recs = [mu.Record(v=rng.uniform(-40, 40, 2).astype(F), live=int(rng.integers(0, 3))) for _ in range(n)]
    res = _results(gpu, rng.integers(0, 2, n))
    _run_and_compare(gpu, mu.Policy(1, 70, 1, 150), st, recs, res, slot_stream=list(range(n - 1, -1, -1)))
    _run_and_compare(gpu, mu.Policy(1, 70, 1, 150), st, recs, res)


def test_refused_operands(gpu):
    st = _states(gpu, [(10, 10, 20, 20)] * 2)
    recs = [mu.Record(), mu.Record()]
    res = _results(gpu, [1, 1])
    for bad in (dict(gain_pct=0), dict(gain_pct=101), dict(coast=61), dict(max_pct=201), dict(on=2), dict(slot_stream=[0, 2]),
                dict(stages=0), dict(stages=4)):
        with pytest.raises(gpu.VtError):
            gpu.op_motion_prior(st, _recs(gpu, recs), res, **bad)
    with pytest.raises(gpu.VtError):        # three slots, two streams, no map
        gpu.op_motion_prior(st, _recs(gpu, recs), _results(gpu, [1, 1, 1]))
