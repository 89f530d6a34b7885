"""Which call zeroes which by-stream record of the keyed features ("The by-stream records and what resets
them"), and what an engine that has enabled nothing answers, on the MI355X, on the committed clip of
tests/golden/make_arbitrate.py. A characterisation of the behaviour as it is: whatever gathers the engine's scattered resets
into one place has to leave every cell below as it stands.

One group of two streams with all seven keyed features on (period 1 wherever there is one, proposals on every update, both
streams in one scene) runs two device passes, so that every record of stream 1 is filled; then ONE call from outside, and
every feature tensor of both streams is compared word by word with what it was: the record's fields all zero where the table
below says so and untouched where it does not, the policy and counter fields untouched, stream 0 untouched. The table is
written out here, cell by cell."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INVALID = -1

# the fields of each tensor that come from the stream's RECORD (the rest: the policy, the device counters, constant zeros)
RECORD = {
    "result_overlay": [],                                       # counters only
    "motion": list(range(1, 8)),
    "appearance": [1, 2, 3],
    "proposals": list(range(1, 7)) + list(range(12, 60)),
    "conflicts": list(range(1, 12)),
    "health": list(range(1, 13)),
    "health_words": list(range(52)),
    "arbitrate": list(range(1, 5)) + list(range(8, 48)),
}
FEATURE_OF = {"health_words": "health"}                         # a tensor's feature, where it is not its own name
# the events that zero a feature's record: an init (synchronous or queued), an import or being the destination of a copy,
# vt_group_set_state_box, the feature's own key set to 0
RESETS = {
    "result_overlay": set(),
    "motion": {"init", "import", "box", "off"},
    "appearance": {"init", "import"},
    "proposals": {"init"},                                      # not on import
    "conflicts": {"init", "import", "box"},
    "health": {"init", "import", "off"},
    "arbitrate": {"init", "import", "off"},
}
ON_KEY = {"result_overlay": "result_overlay", "motion": "motion_prior", "appearance": "appearance", "proposals": "proposals",
          "conflicts": "conflicts", "health": "health", "arbitrate": "arbitrate"}
ON_VALUE = {"result_overlay": 7, "proposals": 2}                # else 1


@pytest.fixture(scope="module")
def clip():
    spec = importlib.util.spec_from_file_location("_make_arbitrate", os.path.join(HERE, "golden", "make_arbitrate.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    fx = dict(np.load(mk.OUT))
    return dict(rgb=[mk.frame(t, fx) for t in range(4)], W=int(fx["frame_w"]), H=int(fx["frame_h"]),
                box0=tuple(int(v) for v in fx["box0"]),
                pol={k: int(fx[k]) for k in ("max_peaks", "radius", "min_resp_pm", "low_pm", "high_pm")})


class Rig:
    """a group of two streams with every keyed feature enabled, and its own device frames (the overlay draws into them)"""

    def __init__(self, gpu, weights, clip):
        import torch
        self.gpu, self.clip = gpu, clip
        self.keep = [torch.from_numpy(f.copy()).cuda() for f in clip["rgb"]]
        self.frames = [gpu.frame_rgb8(d.data_ptr(), clip["W"], clip["H"]) for d in self.keep]
        self.g = g = gpu.Group(weights, n_streams=2)
        self.init_all()
        p = clip["pol"]
        g.set_tuning("result_overlay", 7)
        g.set_motion_prior(True)
        g.set_appearance(True, period=1, gate=0.0)              # before the arbitration: the anchors are its store's
        g.set_proposals(2, period=1)
        g.set_conflicts(True)
        g.set_scene(None, 1)
        g.set_health(True, period=1)
        g.set_arbitration(True, max=p["max_peaks"], radius=p["radius"], min_resp_pm=p["min_resp_pm"], low_pm=p["low_pm"], high_pm=p["high_pm"])

    def box0(self):
        return self.gpu.BBox.new(*self.clip["box0"])

    def init_all(self):
        for s in range(2):
            self.g.init_device(s, self.frames[0], self.box0())

    def tensors(self, s):
        return {n: self.g.read_tensor(n, s).view(np.uint32).copy() for n in RECORD}

    def refill(self, expect):
        """every feature on again, both streams from frame 0, two device passes; then the precondition: each record that the
        coming event is expected to zero has a non-zero field for stream 1. Returns both streams' tensors."""
        for f, key in ON_KEY.items():
            self.g.set_tuning(key, ON_VALUE.get(f, 1))
        self.init_all()
        for t in (1, 2):
            self.g.update_device([self.frames[t]] * 2)
        before = [self.tensors(s) for s in range(2)]
        for n, idx in RECORD.items():
            if FEATURE_OF.get(n, n) in expect:
                assert np.any(before[1][n][idx] != 0), f"'{n}': stream 1's record is all zero before the event: {before[1][n]}"
        return before

    def check(self, before, expect, stream0=True, off=None):
        """after the event: stream 1's records zero exactly for the features in `expect`; off: the feature whose on-key the event
        set to 0 (its flag, field 0 of its tensor, is 0 now)"""
        after = [self.tensors(s) for s in range(2)]
        for n, idx in RECORD.items():
            was, now = before[1][n], after[1][n]
            rest = np.setdiff1d(np.arange(len(was)), idx)
            if FEATURE_OF.get(n, n) in expect:
                assert not np.any(now[idx]), f"'{n}': the record was not zeroed: {now.view(np.float32)}"
            else:
                assert np.array_equal(now[idx], was[idx]), f"'{n}': the record changed: {was} -> {now}"
            if off is not None and n == off:                    # "health_words" carries no flag
                assert now[0] == 0 and was[0] != 0
                rest = rest[rest != 0]
            assert np.array_equal(now[rest], was[rest]), f"'{n}': policy or counter fields changed: {was} -> {now}"
            if stream0:
                assert np.array_equal(after[0][n], before[0][n]), f"'{n}' of stream 0 changed: {before[0][n]} -> {after[0][n]}"
        return after

    def close(self):
        self.g.close()


def _on(event):
    return {f for f, ev in RESETS.items() if event in ev}


@pytest.fixture(scope="module")
def rig(gpu, weights_tiny, clip):
    r = Rig(gpu, weights_tiny, clip)
    yield r
    r.close()


def test_the_table_names_every_feature_and_every_event():
    assert set(RESETS) == set(ON_KEY) == {FEATURE_OF.get(n, n) for n in RECORD}
    assert _on("init") == set(RESETS) - {"result_overlay"} and _on("off") == {"motion", "health", "arbitrate"}
    assert _on("import") == _on("init") - {"proposals"} and _on("box") == {"motion", "conflicts"}


def test_init_device_zeroes_every_record_of_the_stream(rig):
    before = rig.refill(_on("init"))
    rig.g.init_device(1, rig.frames[0], rig.box0())
    rig.check(before, _on("init"))


def test_a_queued_init_zeroes_every_record_of_the_stream(rig):
    """vt_group_enqueue_init_host queues only behind an outstanding pass: a host pass over stream 0 alone, which is then
    collected - so stream 0 is named by that pass and not compared"""
    before = rig.refill(_on("init"))
    rgb = rig.clip["rgb"]
    rig.g.enqueue_host([rgb[3]], streams=[0])
    rig.g.enqueue_init_host(1, rgb[0], rig.box0())
    rig.g.wait_next()
    rig.check(before, _on("init"), stream0=False)
    assert rig.g.read_state(1)["frames_done"] == 0 and rig.g.read_state(0)["frames_done"] == 3


def test_set_state_box_zeroes_motion_and_conflicts(rig):
    before = rig.refill(_on("box"))
    box = rig.g.read_state(1)["box"]
    rig.g.set_state_box(1, [float(box[0]) + 3, float(box[1]) - 2, float(box[2]), float(box[3])])
    rig.check(before, _on("box"))


def test_import_zeroes_every_record_but_the_proposals(rig):
    before = rig.refill(_on("import"))
    rig.g.import_stream(1, rig.g.export_stream(1))
    rig.check(before, _on("import"))


def test_the_destination_of_a_copy_is_reset_like_an_import(rig, gpu, weights_tiny, clip):
    dst = Rig(gpu, weights_tiny, clip)          # a second, equally enabled group
    before = dst.refill(_on("import"))
    rig.refill(set())
    rig.g.copy_stream(0, dst.g, 1)
    dst.check(before, _on("import"))
    dst.close()


@pytest.mark.parametrize("feature", ["motion", "appearance", "proposals", "conflicts", "health", "arbitrate"])
def test_the_on_key_set_to_0_zeroes_every_streams_record_of_motion_health_and_arbitration_only(rig, feature):
    expect = {feature} & _on("off")
    before = rig.refill(expect)
    rig.g.set_tuning(ON_KEY[feature], 0)
    after = rig.check(before, expect, stream0=False, off=feature)
    for n, idx in RECORD.items():               # the key names every stream: stream 0's record as stream 1's
        if FEATURE_OF.get(n, n) in expect:
            assert not np.any(after[0][n][idx]), n


def test_set_scene_zeroes_the_conflict_records_of_the_streams_it_names(rig):
    before = rig.refill({"conflicts"})
    rig.g.set_scene(1, 1)                       # the scene it already shows: its scene field stays
    rig.check(before, {"conflicts"})
    before = rig.refill({"conflicts"})
    rig.g.set_scene(None, 1)                    # every stream
    after = rig.check(before, {"conflicts"}, stream0=False)
    assert not np.any(after[0]["conflicts"][RECORD["conflicts"]])


@pytest.fixture(scope="module")
def twins(gpu, weights_tiny, clip):
    """two rigs that only ever make the same calls (their overlays have drawn the same boxes into their frames)"""
    pair = [Rig(gpu, weights_tiny, clip) for _ in range(2)]
    yield pair
    for r in pair:
        r.close()


@pytest.mark.parametrize("feature", ["motion", "health", "arbitrate", "conflicts"])
def test_a_pass_directly_behind_a_reset_runs_behind_it(twins, feature):
    """The resets that fill on the engine's stream without waiting for it - an on-key set to 0, vt_group_set_scene - and then,
    with no read in between, one pass: stream 1's tensor equals, word for word, that of the twin, which made the same calls
    with a read (it synchronises the stream) between the reset and the pass. A consistency check of the order, no race
    detector."""
    got = []
    for r, read_between in zip(twins, (False, True)):
        r.refill({feature})
        if feature == "conflicts":
            r.g.set_scene(None, 1)
        else:
            r.g.set_tuning(ON_KEY[feature], 0)
        if read_between:
            r.g.read_tensor(feature, 1)
        r.g.update_device([r.frames[3]] * 2)
        got.append(r.tensors(1))
    for n in RECORD:
        if FEATURE_OF.get(n, n) == feature:
            assert np.array_equal(got[0][n], got[1][n]), f"'{n}': {got[0][n]} without a read, {got[1][n]} with one"


NOT_ENABLED = {
    "result_overlay": 'result overlay: not enabled on this engine (vt_group_set_tuning "result_overlay")',
    "motion": 'motion prior: not enabled on this engine (vt_group_set_tuning "motion_prior")',
    "appearance": 'appearance check: not enabled on this engine (vt_group_set_tuning "appearance")',
    "anchor": 'appearance check: not enabled on this engine (vt_group_set_tuning "appearance")',
    "probe": 'appearance check: not enabled on this engine (vt_group_set_tuning "appearance")',
    "proposals": 'reacquire proposals: not enabled on this engine (vt_group_set_tuning "proposals")',
    "proposals_pattern": 'reacquire proposals: not enabled on this engine (vt_group_set_tuning "proposals")',
    "proposals_map": 'reacquire proposals: not enabled on this engine (vt_group_set_tuning "proposals")',
    "conflicts": 'stream conflicts: not enabled on this engine (vt_group_set_tuning "conflicts")',
    "health": 'frame health: not enabled on this engine (vt_group_set_tuning "health")',
    "health_words": 'frame health: not enabled on this engine (vt_group_set_tuning "health")',
    "arbitrate": 'peak arbitration: not enabled on this engine (vt_group_set_tuning "arbitrate")',
}


def test_an_engine_that_enabled_nothing_names_the_key_that_enables(gpu, weights_tiny):
    g = gpu.Group(weights_tiny, n_streams=2)
    assert set(RECORD) <= set(NOT_ENABLED)
    for name, text in NOT_ENABLED.items():
        for s in range(2):
            with pytest.raises(gpu.VtError) as ei:
                g.read_tensor(name, s)
            assert ei.value.code == INVALID and str(ei.value) == f"vittrack_hip error {INVALID}: {text}", (name, str(ei.value))
    g.close()
