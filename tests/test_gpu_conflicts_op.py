"""Stream conflicts, operator level (vt_op_stream_conflicts: the one launch of csrc/k_conflicts.hip alone), on the MI355X.

Every comparison is np.array_equal against the NumPy model of tests/conflicts_util.py: every record, every counter and the
pinned mirror, byte for byte. The hook keeps records and counters between guard bands (a changed guard byte is an error of
the call); they start as 0xA5 bytes, so what the launch must leave alone - the streams no lane worked for, and with the flag
off everything - has to come back as it went in."""
import importlib

import numpy as np
import pytest

import conflicts_util as cu
from test_conflicts_cases import CASES

pytestmark = pytest.mark.gpu

F = np.float32
FILL = 0xA5


def _states(gpu, boxes, frames_done=None, initialized=None, window_miss=None):
    st = np.zeros(len(boxes), importlib.import_module(gpu.__name__ + ".snapshot").STATE)
    st["box"] = np.asarray(boxes, F).reshape(-1, 4)
    st["frame_w"], st["frame_h"] = 640, 480
    st["frames_done"] = 1 if frames_done is None else frames_done
    st["initialized"] = 1 if initialized is None else initialized
    st["window_miss"] = 0 if window_miss is None else window_miss
    return st


def _pattern(n, dtype):
    return np.frombuffer(bytes([FILL]) * (n * dtype.itemsize), dtype).copy()


def run(gpu, boxes, success, scenes, pm=300, frames_done=None, initialized=None, window_miss=None, slot_stream=None, winner=None,
        on=1, counts=None):
    """the hook and the model on the same operands; -> (got, model's {stream: record})"""
    st = _states(gpu, boxes, frames_done, initialized, window_miss)
    res = np.zeros(len(success), gpu.RESULT_DTYPE)
    res["success"] = success
    res["score"] = 0.5
    ns = len(st)
    got = gpu.op_stream_conflicts(st, res, scenes, on=on, iou_pm=pm, slot_stream=slot_stream, winner=winner, counts=counts,
                                  host_records=_pattern(ns, gpu.CONFLICT_REC_DTYPE), fill=FILL)
    want = cu.check_states(st, res, scenes, pm=pm, slot_stream=slot_stream, winner=winner, on=on)
    start_c = _pattern(ns, gpu.CONFLICT_COUNT_DTYPE) if counts is None else np.asarray(counts, gpu.CONFLICT_COUNT_DTYPE)
    rec, cnt = cu.apply(_pattern(ns, cu.REC), start_c.view(cu.COUNT), want)
    assert cu.REC == gpu.CONFLICT_REC_DTYPE and cu.COUNT == gpu.CONFLICT_COUNT_DTYPE
    assert np.array_equal(got["records"].view(np.uint8), rec.view(np.uint8)), _diff(got["records"], rec)
    assert np.array_equal(got["host_records"].view(np.uint8), rec.view(np.uint8)), "the pinned mirror"
    assert np.array_equal(got["counts"].view(np.uint8), cnt.view(np.uint8)), (got["counts"], cnt)
    return got, want


def _diff(a, b):
    bad = [s for s in range(len(a)) if a[s].tobytes() != b[s].tobytes()]
    return f"{len(bad)} records differ, first stream {bad[0]}: got {a[bad[0]]}, want {b[bad[0]]}" if bad else ""


def random_scene(n, n_scenes, seed, n_streams=None):
    """boxes on a 640 x 480 canvas, sides 20..120 with fractions: many pairs overlap; some streams fail, some sit in scene 0"""
    rng = np.random.default_rng(seed)
    ns = n if n_streams is None else n_streams
    wh = rng.uniform(20.0, 120.0, (ns, 2))
    xy = rng.uniform(0.0, 1.0, (ns, 2)) * (np.array([640.0, 480.0]) - wh)
    boxes = np.concatenate([xy, wh], 1).astype(F)
    scenes = rng.integers(0, n_scenes + 1, ns)      # 0: compared with nobody
    scenes[scenes > 0] += 1000 * (n_scenes > 3)     # large scene numbers too
    success = (rng.uniform(size=n) > 0.1).astype(np.int32)
    fd = rng.integers(1, 50, ns)
    miss = np.where(rng.uniform(size=ns) > 0.9, fd, 0)
    return dict(boxes=boxes, success=success, scenes=scenes, frames_done=fd, window_miss=miss)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1024])
@pytest.mark.parametrize("n_scenes", [1, 3, 64])
def test_random_boxes_equal_the_model(gpu, n, n_scenes):
    kw = random_scene(n, n_scenes, seed=1000 * n_scenes + n)
    _, want = run(gpu, pm=300, **kw)
    if n >= 63 and n_scenes <= 3:       # dense enough that every status occurs, and at 1024 more partners than a record lists
        assert {1, 2, 3} <= {int(r["status"]) for r in want.values()}
        assert max(int(r["n_over"]) for r in want.values()) > 4 or n < 1024


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cpu_cases_on_the_kernel(gpu, name):
    kw = dict(CASES[name])
    _, want = run(gpu, **kw)
    assert (want == {}) == (name == "off")


@pytest.mark.parametrize("n,n_streams", [(5, 9), (64, 200), (300, 1024)])
def test_subset_maps(gpu, n, n_streams):
    """slot != stream: the listed streams get records, every byte of the unlisted ones stays the pattern (run compares all)"""
    kw = random_scene(n, 2, seed=7 * n, n_streams=n_streams)
    rng = np.random.default_rng(n)
    order = rng.permutation(n_streams)[:n]
    _, want = run(gpu, slot_stream=order, pm=200, **kw)
    assert sorted(want) == sorted(int(s) for s in order)
    # the order of the list changes no record
    rev = order[::-1].copy()
    kw2 = dict(kw, success=kw["success"][::-1].copy())
    _, want2 = run(gpu, slot_stream=rev, pm=200, **kw2)
    assert all(want[s].tobytes() == want2[s].tobytes() for s in want)


def test_candidate_style_list(gpu):
    """several slots name one stream: the winning slot works for it, with its result; the losers leave no trace"""
    n_streams, per = 40, 3
    kw = random_scene(n_streams * per, 2, seed=99, n_streams=n_streams)
    rng = np.random.default_rng(5)
    smap = np.repeat(np.arange(n_streams), per)[rng.permutation(n_streams * per)]
    winner = np.empty(len(smap), np.int32)
    for s in range(n_streams):
        slots = np.flatnonzero(smap == s)
        winner[slots] = slots[rng.integers(0, per)]
    _, want = run(gpu, slot_stream=smap, winner=winner, **kw)
    assert len(want) == n_streams and {1, 2, 3} <= {int(r["status"]) for r in want.values()}
    run(gpu, slot_stream=smap, winner=None, **kw)       # without the marks: the first slot of each stream


def test_flag_zero_writes_nothing(gpu):
    kw = random_scene(200, 1, seed=4)
    got, want = run(gpu, on=0, **kw)
    assert want == {} and set(got["records"].view(np.uint8).tolist()) == {FILL}


def test_counters_advance_from_what_they_held(gpu):
    kw = CASES["failed_stream"]
    counts = np.zeros(3, gpu.CONFLICT_COUNT_DTYPE)
    counts["evaluated"], counts["conflicting"], counts["gated"], counts["reserved"] = [5, 6, 7], [1, 2, 3], 9, 11
    got, _ = run(gpu, counts=counts, **kw)
    assert got["counts"]["evaluated"].tolist() == [6, 6, 8] and got["counts"]["conflicting"].tolist() == [2, 2, 4]
    assert got["counts"]["gated"].tolist() == [9, 9, 9] and got["counts"]["reserved"].tolist() == [11, 11, 11]


def test_bad_operands_are_refused(gpu):
    kw = CASES["identical"]
    for bad in (dict(pm=0), dict(pm=1001), dict(on=2), dict(scenes=[1, 65536]), dict(scenes=[-1, 1]), dict(slot_stream=[0, 2]),
                dict(slot_stream=[0, 1], winner=[0, 2])):
        with pytest.raises(gpu.VtError):
            run(gpu, **{**kw, **bad})
