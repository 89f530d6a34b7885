"""The rule of the stream conflicts on its NumPy model alone (tests/conflicts_util.py; the rule to the bit:
include/vittrack_hip.h above the "conflicts*" keys): what the GPU tests hold the kernel to must itself do what the rule says,
and the mutations a slip in the kernel would be must fail these cases. No GPU. CASES is shared with the operator test, which
runs every one of them through the kernel."""
import numpy as np
import pytest

import conflicts_util as cu

F = np.float32


def bits(v):
    return np.asarray(v, F).tobytes()


def fractional_boxes(seed=3, n=24):
    """overlapping boxes with sizes that are no short binary fractions: their areas round, and a fused sum differs"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(100.0, 130.0, (n, 2))
    wh = rng.uniform(30.0, 70.0, (n, 2)) / 3.0 * 3.1
    return np.concatenate([xy, wh], 1).astype(F)


# name -> keyword arguments of conflicts_util.check
CASES = {
    "identical": dict(boxes=[(10, 20, 30, 40), (10, 20, 30, 40)], success=[1, 1], scenes=[1, 1], pm=1000),
    "touching": dict(boxes=[(0, 0, 10, 10), (10, 0, 10, 10), (0, 10, 10, 10)], success=[1, 1, 1], scenes=[1, 1, 1], pm=1),
    "half_500": dict(boxes=[(0, 0, 2, 2), (0, 0, 2, 1)], success=[1, 1], scenes=[4, 4], pm=500),
    "half_501": dict(boxes=[(0, 0, 2, 2), (0, 0, 2, 1)], success=[1, 1], scenes=[4, 4], pm=501),
    "third_333": dict(boxes=[(0, 0, 2, 1), (1, 0, 2, 1)], success=[1, 1], scenes=[9, 9], pm=333),
    "third_334": dict(boxes=[(0, 0, 2, 1), (1, 0, 2, 1)], success=[1, 1], scenes=[9, 9], pm=334),
    # stream 0 against five partners: 1 and 4 tie at 0.5 (different boxes, same IoU), 2, 3, 5 smaller and distinct; the slots
    # list the streams in the order 0, 4, 3, 2, 1, 5, so slot order and stream order disagree on the tie
    "five_partners": dict(boxes=[(0, 0, 8, 8), (0, 0, 8, 4), (0, 0, 8, 3), (0, 0, 8, 2), (0, 4, 8, 4), (0, 0, 8, 1),
                                 (500, 500, 8, 8)],
                          success=[1] * 6, scenes=[2] * 7, pm=100, slot_stream=[0, 4, 3, 2, 1, 5]),
    "scene_zero": dict(boxes=[(0, 0, 8, 8)] * 3, success=[1, 1, 1], scenes=[1, 0, 1], pm=300),
    "other_scenes": dict(boxes=[(0, 0, 8, 8)] * 4, success=[1] * 4, scenes=[1, 2, 1, 65535], pm=300),
    "failed_stream": dict(boxes=[(0, 0, 8, 8)] * 3, success=[1, 0, 1], scenes=[1, 1, 1], pm=300),
    "window_miss": dict(boxes=[(0, 0, 8, 8)] * 3, success=[1, 1, 1], scenes=[1, 1, 1], pm=300, frames_done=[5, 7, 5],
                        window_miss=[0, 7, 4]),
    "uninitialised": dict(boxes=[(0, 0, 8, 8)] * 2, success=[1, 1], scenes=[1, 1], initialized=[1, 0], pm=300),
    "threshold_exact": dict(boxes=[(0, 0, 3, 1), (0, 0, 1, 1)], success=[1, 1], scenes=[1, 1], pm=333),
    "fractional": dict(boxes=fractional_boxes(), success=[1] * 24, scenes=[1] * 24, pm=300),
    "candidates": dict(boxes=[(0, 0, 8, 8), (0, 0, 8, 6), (100, 100, 8, 8)], success=[0, 1, 1, 0, 1, 1], scenes=[1, 1, 1], pm=300,
                       slot_stream=[0, 0, 1, 1, 2, 0], winner=[1, 1, 2, 2, 4, 1]),
    "off": dict(boxes=[(0, 0, 8, 8)] * 2, success=[1, 1], scenes=[1, 1], pm=300, on=0),
}


def same(a, b):
    return a.keys() == b.keys() and all(a[s].tobytes() == b[s].tobytes() for s in a)


def test_identical_boxes_have_iou_one():
    out = cu.check(**CASES["identical"])
    assert bits(cu.iou((10, 20, 30, 40), (10, 20, 30, 40))) == bits(1.0)
    for s, t in ((0, 1), (1, 0)):
        assert (out[s]["status"], out[s]["n_over"], out[s]["partner"].tolist()) == (2, 1, [t, -1, -1, -1])
        assert bits(out[s]["iou"]) == bits([1, 0, 0, 0])


def test_touching_boxes_are_not_listed():
    assert bits(cu.iou((0, 0, 10, 10), (10, 0, 10, 10))) == bits(0.0)       # ix == 0
    out = cu.check(**CASES["touching"])
    assert all((out[s]["status"], out[s]["n_over"]) == (1, 0) and out[s]["partner"].tolist() == [-1] * 4 for s in range(3))


def test_half_is_listed_at_500_and_not_at_501():
    assert bits(cu.iou((0, 0, 2, 2), (0, 0, 2, 1))) == bits(0.5)
    assert [cu.check(**CASES["half_500"])[s]["status"] for s in (0, 1)] == [2, 2]
    assert [cu.check(**CASES["half_501"])[s]["status"] for s in (0, 1)] == [1, 1]


def test_a_third_against_333_and_334():
    v = cu.iou((0, 0, 2, 1), (1, 0, 2, 1))
    assert bits(v) == bits(F(1.0) / F(3.0)) and cu.tau_of(333) < v < cu.tau_of(334)
    assert cu.check(**CASES["third_333"])[0]["status"] == 2 and cu.check(**CASES["third_334"])[0]["status"] == 1


def test_iou_equal_to_tau_is_over():
    assert bits(cu.iou((0, 0, 2, 2), (0, 0, 2, 1))) == bits(cu.tau_of(500))      # the same bits: equality counts
    assert cu.check(**CASES["half_500"])[0]["n_over"] == 1
    assert bits(cu.iou((0, 0, 3, 1), (0, 0, 1, 1))) == bits(F(1.0) / F(3.0))      # no per-mille tau: 333 lies below it
    assert cu.check(**CASES["threshold_exact"])[1]["partner"].tolist() == [0, -1, -1, -1]


def test_five_partners_of_which_two_tie():
    out = cu.check(**CASES["five_partners"])
    r = out[0]
    assert (r["status"], r["n_over"]) == (2, 5)
    assert r["partner"].tolist() == [1, 4, 2, 3]            # 0.5 (stream 1 before stream 4), 0.375, 0.25; 0.125 not listed
    assert bits(r["iou"]) == bits([0.5, 0.5, 0.375, 0.25])
    assert 6 not in out                                     # not in the pass: no record, and nobody's partner


@pytest.mark.parametrize("name,outsider", [("scene_zero", 1), ("failed_stream", 1), ("window_miss", 1), ("uninitialised", 1)])
def test_streams_that_are_not_eligible_have_status_3_and_are_nobodys_partner(name, outsider):
    kw = CASES[name]
    out = cu.check(**kw)
    fd = kw.get("frames_done", [1] * len(kw["scenes"]))[outsider]
    assert out[outsider].tobytes() == cu.record(3, fd).tobytes()
    for s, r in out.items():
        assert outsider not in r["partner"].tolist()
        if s != outsider and name != "uninitialised":
            assert r["status"] == 2 and r["n_over"] == 1       # the two others see each other


def test_different_scenes_do_not_meet():
    out = cu.check(**CASES["other_scenes"])
    assert out[0]["partner"].tolist() == [2, -1, -1, -1] and out[2]["partner"].tolist() == [0, -1, -1, -1]
    assert out[1]["status"] == 1 and out[3]["status"] == 1


def test_a_candidate_pass_works_at_the_winning_slot():
    out = cu.check(**CASES["candidates"])
    assert sorted(out) == [0, 1, 2]
    assert out[0]["status"] == 2 and out[0]["partner"][0] == 1      # slot 1 won for stream 0 and succeeded (slot 0 failed)
    assert out[2]["status"] == 1
    first = cu.check(**{**CASES["candidates"], "winner": None})     # without the marks the first slot of a stream works
    assert first[0]["status"] == 3 and first[1]["status"] == 1      # slot 0 failed: stream 0 is nobody's partner


def test_flag_zero_writes_nothing():
    assert cu.check(**CASES["off"]) == {}


def test_iou_is_symmetric_to_the_bit():
    b = fractional_boxes(seed=8, n=40)
    n = 0
    for s in range(len(b)):
        for t in range(s):
            assert bits(cu.iou(b[s], b[t])) == bits(cu.iou(b[t], b[s]))
            n += cu.iou(b[s], b[t]) > 0
    assert n > 300


def test_permuting_the_slots_changes_no_record():
    kw = CASES["fractional"]
    want = cu.check(**kw)
    assert sum(r["n_over"] > 4 for r in want.values()) > 0
    rng = np.random.default_rng(0)
    for _ in range(3):
        order = rng.permutation(len(kw["success"]))
        assert same(cu.check(**{**kw, "slot_stream": order}), want)
    kw = CASES["five_partners"]
    assert same(cu.check(**{**kw, "slot_stream": [5, 1, 2, 3, 4, 0]}), cu.check(**kw))


@pytest.mark.parametrize("mut,caught_by", [("gt", "half_500"), ("slot", "five_partners"), ("fused", "fractional"),
                                           ("failed", "failed_stream")])
def test_each_mutation_is_caught(mut, caught_by):
    assert not same(cu.check(**CASES[caught_by], mut=mut), cu.check(**CASES[caught_by]))
    assert same(cu.check(**CASES["third_333"], mut=mut), cu.check(**CASES["third_333"]))      # and is no blanket change


def test_rule_9_sits_ahead_of_the_geometry_and_counts():
    from types import SimpleNamespace as R
    ok = R(success=1, score=0.9, bbox=(100, 100, 40, 40))
    rule = cu.Rule(64, 128, period=2, conflicts_gate=True)
    box = np.array([100, 100, 40, 40], F)
    far = np.array([400, 300, 40, 40], F)       # a search crop elsewhere: rule 6 would skip
    assert rule.step(ok, pre_box=box, conflict=2) is None           # not yet due (rule 4)
    assert rule.step(ok, pre_box=far, conflict=2) == "conflict"     # due and conflicting: gated, no geometry skip
    assert rule.step(ok, pre_box=far, conflict=1) == "skip"         # still due, not conflicting: now rule 6 speaks
    assert rule.step(ok, pre_box=box, conflict=1) == "fire"
    assert (rule.conflict_gated, rule.skipped, rule.fired) == ([2], [3], [4])
    off = cu.Rule(64, 128, period=2, conflicts_gate=False)
    assert [off.step(ok, pre_box=box, conflict=2) for _ in range(2)] == [None, "fire"]
