"""Motion prior, the rule (no GPU): hand-computed known answers for the NumPy-float32 model of tests/motion_prior_util.py -
the model the GPU tests compare the kernels with - and a replay of the committed behaviour fixture
(tests/golden/motion_prior_tiny.npz, made by tests/golden/make_motion_prior.py from the oracle alone)."""
import importlib.util
import os

import numpy as np

import motion_prior_util as mu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "motion_prior_tiny.npz")


def _maker():
    spec = importlib.util.spec_from_file_location("_make_motion_prior", os.path.join(HERE, "golden", "make_motion_prior.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_ema_with_a_gain_that_is_not_representable():
    pol, rec = mu.Policy(1, 33, 5, 200), mu.Record()
    assert mu.place(pol, rec, (100, 50, 20, 30), 640, 480).tolist() == [100, 50, 20, 30]     # v == 0: nothing moves
    assert rec.prior.tolist() == [100, 50, 20, 30] and rec.shift.tolist() == [0, 0] and rec.n_shift == 0
    # the decode left (110, 47, 20, 30): d = (10, -3); v = 0 + a * (d - 0), a = float32(33) / float32(100)
    a = F(33) / F(100)
    assert float(a) != 0.33 and float(a) == 0.33000001311302185
    out = mu.settle(pol, rec, (110, 47, 20, 30), True)
    assert out.tolist() == [110, 47, 20, 30]
    assert rec.v[0] == F(a * F(10)) and rec.v[1] == F(a * F(-3)) and rec.live == 5
    assert [float(x) for x in rec.v] == [3.3000001907348633, -0.9900000095367432]     # a * -3 is a tie: to even
    # second update: placed at (110 + vx, 47 + vy); the decode finds (121, 44): d from the PRIOR's centre = (11, -3)
    nb = mu.place(pol, rec, out, 640, 480)
    assert nb.tolist() == [float(F(110) + rec.v[0]), float(F(47) + rec.v[1]), 20, 30] and rec.n_shift == 1
    assert rec.shift.tolist() == rec.v.tolist() and rec.prior.tolist() == [110, 47, 20, 30]
    v0 = rec.v.copy()
    mu.settle(pol, rec, (121, 44, 20, 30), True)
    want = [F(v0[0] + F(a * F(F(11) - v0[0]))), F(v0[1] + F(a * F(F(-3) - v0[1])))]
    assert rec.v.tolist() == [float(w) for w in want]
    # worked in exact rational arithmetic, every operation rounded to binary32 on its own. vx tells a contracted
    # multiply-add apart: v + a * (d - v) with ONE rounding behind the product and the sum gives 5.841000080108643
    assert nb.tolist() == [113.30000305175781, 46.0099983215332, 20, 30]
    assert [float(x) for x in rec.v] == [5.841000556945801, -1.6533000469207764]


def test_the_clamp_on_both_signs():
    pol = mu.Policy(1, 100, 5, 50)     # lim = 0.5 * sqrt(16 * 25) = 10
    rec = mu.Record()
    mu.place(pol, rec, (100, 100, 16, 25), 640, 480)
    mu.settle(pol, rec, (140, 60, 16, 25), True)
    assert rec.v.tolist() == [10.0, -10.0]
    mu.place(pol, rec, (140, 60, 16, 25), 640, 480)
    mu.settle(pol, rec, (100, 100, 16, 25), True)       # d = (-40, 40) from the PRIOR (140, 60)
    assert rec.v.tolist() == [-10.0, 10.0]
    # the limit follows the NEW box: sqrt(9 * 9) * 2.0 = 18; and max_pct 0 pins the velocity at zero
    rec = mu.Record()
    mu.place(mu.Policy(1, 100, 5, 200), rec, (0, 0, 30, 30), 640, 480)
    mu.settle(mu.Policy(1, 100, 5, 200), rec, (40, 5, 9, 9), True)
    assert rec.v.tolist() == [18.0, -5.5]
    mu.settle(mu.Policy(1, 100, 5, 0), rec, (40, 5, 9, 9), True)
    assert rec.v.tolist() == [0.0, 0.0] or rec.v.tolist() == [-0.0, 0.0]


def test_the_in_frame_test_fails_on_each_side():
    pol = mu.Policy(1, 50, 5, 100)
    for v, box, why in (((-30, 0), (10, 100, 20, 20), "left: cx = -10"), ((0, -25), (100, 5, 20, 20), "top: cy = -10"),
                        ((25, 0), (605, 100, 20, 20), "right: cx = 640 is outside"), ((0, 12), (100, 458, 20, 20), "bottom: cy = 480")):
        rec = mu.Record(v=v, live=4, n_shift=7)
        out = mu.place(pol, rec, box, 640, 480)
        assert out.tolist() == list(box), why
        assert rec.v.tolist() == [0, 0] and rec.live == 0 and rec.shift.tolist() == [0, 0] and rec.n_shift == 7, why
        assert rec.prior.tolist() == list(box)
    # just inside on every side: cx = 0 / cy = 0 are inside, cx = W - 0.5 is
    for v, box in (((-20, 0), (10, 100, 20, 20)), ((0, -15), (100, 5, 20, 20)), ((24.5, 0), (605, 100, 20, 20)), ((0, 11.5), (100, 458, 20, 20))):
        rec = mu.Record(v=v, live=4)
        out = mu.place(pol, rec, box, 640, 480)
        assert out.tolist() == [box[0] + v[0], box[1] + v[1], 20, 20] and rec.live == 4 and rec.n_shift == 1
        assert rec.shift.tolist() == list(v)
    # the flag off: nothing moves and nothing is dropped
    rec = mu.Record(v=(5, 5), live=2)
    assert mu.place(mu.Policy(0), rec, (10, 10, 20, 20), 640, 480).tolist() == [10, 10, 20, 20] and rec.v.tolist() == [5, 5]


def test_live_counts_down_to_the_restore():
    pol, rec = mu.Policy(1, 100, 2, 200), mu.Record()
    box = mu.place(pol, rec, (100, 100, 20, 20), 640, 480)
    box = mu.settle(pol, rec, (108, 96, 20, 20), True)
    assert rec.v.tolist() == [8, -4] and rec.live == 2
    for k, live in ((1, 1), (2, 0)):        # two failures coast: the decode leaves the placed box, settle keeps it
        box = mu.place(pol, rec, box, 640, 480)
        assert box.tolist() == [108 + 8 * k, 96 - 4 * k, 20, 20]
        box = mu.settle(pol, rec, box, False)
        assert box.tolist() == [108 + 8 * k, 96 - 4 * k, 20, 20] and rec.live == live and rec.n_coast == k
        assert rec.v.tolist() == [8, -4]
    box = mu.place(pol, rec, box, 640, 480)     # the third failure restores the box this pass started from
    assert box.tolist() == [132, 84, 20, 20] and rec.n_shift == 3
    box = mu.settle(pol, rec, box, False)
    assert box.tolist() == [124, 88, 20, 20] and rec.v.tolist() == [0, 0] and rec.live == 0 and rec.n_coast == 2
    box = mu.place(pol, rec, box, 640, 480)     # from here on the plain tracker
    assert box.tolist() == [124, 88, 20, 20] and rec.n_shift == 3
    assert mu.settle(pol, rec, box, False).tolist() == [124, 88, 20, 20]
    # coast 0: the first failure restores
    pol, rec = mu.Policy(1, 100, 0, 200), mu.Record(v=(3, 3))
    box = mu.place(pol, rec, (50, 50, 20, 20), 640, 480)
    assert mu.settle(pol, rec, box, False).tolist() == [50, 50, 20, 20] and rec.n_coast == 0


def test_a_nan_score_fails_and_a_placed_winner_resets_the_velocity():
    # a NaN score: the decode's success is (score >= threshold) = 0, which is all the rule reads
    score = F("nan")
    success = bool(score >= F(0.2))
    pol, rec = mu.Policy(1, 50, 1, 100), mu.Record(v=(4, 0), live=1)
    box = mu.place(pol, rec, (10, 10, 20, 20), 640, 480)
    assert mu.settle(pol, rec, box, success).tolist() == [14, 10, 20, 20] and rec.live == 0 and rec.n_coast == 1
    # a has_box == 1 winner: the caller placed it, the jump is no motion
    rec = mu.Record(v=(4, -2), live=0)
    mu.place(pol, rec, (10, 10, 20, 20), 640, 480)
    out = mu.settle(pol, rec, (300, 200, 22, 18), True, has_box=True)
    assert out.tolist() == [300, 200, 22, 18] and rec.v.tolist() == [0, 0] and rec.live == 1
    # ... and a has_box winner that failed is a failure like any other
    rec = mu.Record(v=(4, -2), live=0)
    box = mu.place(pol, rec, (10, 10, 20, 20), 640, 480)
    assert mu.settle(pol, rec, box, False, has_box=True).tolist() == [10, 10, 20, 20] and rec.v.tolist() == [0, 0]


def test_record_words_and_read_out():
    rec = mu.Record(v=(1.5, -2), prior=(1, 2, 3, 4), shift=(1.5, -2), live=3, n_shift=9, n_coast=2)
    w = rec.words()
    assert w.dtype == np.uint32 and w.shape == (mu.REC_WORDS,) and w.nbytes == 48
    assert w[:8].view(F).tolist() == [1.5, -2, 1, 2, 3, 4, 1.5, -2] and w[8:].tolist() == [3, 9, 2, 0]
    assert rec.read_out(1).tolist() == [1, 1.5, -2, 3, 1.5, -2, 9, 2]


def test_the_committed_fixture_replays(vt, oracle):
    """the oracle driven by the model reproduces every recorded box, score, flag and record; the conditions that make the GPU
    tests meaningful hold on the committed file"""
    mk = _maker()
    fx = dict(np.load(FIXTURE))
    mk.check(fx)
    assert float(fx["min_iou"]) > 0.5
    weights = vt.weights.ensure_weights("tiny")
    assert mk.sha256_file(weights) == str(fx["weights_sha256"]), "the fixture was made with another weight blob"
    assert (int(fx["frame_w"]), int(fx["frame_h"]), int(fx["square"]), int(fx["step"]), int(fx["n"])) == (mk.W, mk.H, mk.SQ, mk.STEP, mk.N)
    sc, ts, frames = mk.clip()
    assert ts == fx["times"].tolist()
    res, recs, boxes = mu.drive(mu.OracleTracker(weights), frames, tuple(int(v) for v in fx["box0"]), mu.Policy(*fx["policy"]), mk.W, mk.H)
    assert np.array_equal(np.array([r.bbox for r in res], np.int32), fx["bbox"])
    assert np.array_equal(np.array([r.score for r in res], F).view(np.uint32), fx["score"].view(np.uint32))
    assert [int(r.success) for r in res] == fx["success"].tolist()
    assert np.array_equal(np.array([r.words() for r in recs]), fx["rec_words"])
    assert np.array_equal(np.array(boxes, F).view(np.uint32), fx["state_box"].view(np.uint32))
    pres, _, _ = mu.drive(mu.OracleTracker(weights), frames, tuple(int(v) for v in fx["box0"]), None, mk.W, mk.H)
    assert [int(r.success) for r in pres] == fx["plain_success"].tolist()
    assert np.array_equal(np.array([r.bbox for r in pres], np.int32), fx["plain_bbox"])
