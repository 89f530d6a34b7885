"""Peak arbitration in the pass (the "arbitrate*" keys of vt_group_set_tuning; DESIGN.md section 3, "Peak arbitration"), on the
MI355X, on the committed clip of tests/golden/make_arbitrate.py (the frames are regenerated from the fixture's parameters).

Yardsticks: a PLAIN appearance-enabled engine (the option switched off, or inert at low 0, changes no bit); a HOST TWIN - a
plain engine whose host reads last_peaks behind every pass, cuts each peak's probe through a helper engine's init, scores it
with vt_op_appearance_score, applies the NumPy rule of tests/arbitrate_util.py and, on a switch, calls vt_group_set_state_box;
and the synchronous host passes for the pipelined ones."""
import importlib.util
import os

import numpy as np
import pytest

import arbitrate_util as ar
from arbitrate_util import F
from test_gpu_stream_subsets import _res

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = {"arbitrate_max": 3, "arbitrate_radius": 1, "arbitrate_min_resp_pm": 50, "arbitrate_low_pm": 300, "arbitrate_high_pm": 500, "arbitrate": 1}
INVALID = -1


@pytest.fixture(scope="module")
def clip():
    spec = importlib.util.spec_from_file_location("_make_arbitrate", os.path.join(HERE, "golden", "make_arbitrate.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    fx = dict(np.load(mk.OUT))
    n = int(fx["n_frames"])
    return dict(mk=mk, fx=fx, n=n, rgb=[mk.frame(t, fx) for t in range(n)], W=int(fx["frame_w"]), H=int(fx["frame_h"]),
                box0=tuple(int(v) for v in fx["box0"]), pol={k: int(fx[k]) for k in ("on", "max_peaks", "radius", "min_resp_pm", "low_pm", "high_pm")})


@pytest.fixture(scope="module")
def dev(gpu, clip):
    """the clip's frames in device memory: (CFrame, keep-alive tensor) per frame"""
    import torch
    keep = [torch.from_numpy(f).cuda() for f in clip["rgb"]]
    return [gpu.frame_rgb8(d.data_ptr(), clip["W"], clip["H"]) for d in keep], keep


def _state(g, s=0):
    return g.read_tensor("state", s).view(np.uint32).copy()


def _tpl(g, s=0):
    return g.read_tensor("template", s).view(np.uint32).copy()


def _bits(g, name, s=0):
    mi = g.model_info()
    return (g.read_tensor(name, s).view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(mi.tokens_template, mi.kpad)


def _engine(gpu, weights, clip, frame0, B=1, arbitrate=True, host=False, **kw):
    g = gpu.Group(weights, n_streams=B, **kw)
    for s in range(B):
        (g.init_host if host else g.init_device)(s, frame0, gpu.BBox.new(*clip["box0"]))
    g.set_appearance(True, period=1, gate=0.0)
    if arbitrate:
        p = clip["pol"]
        g.set_arbitration(True, max=p["max_peaks"], radius=p["radius"], min_resp_pm=p["min_resp_pm"], low_pm=p["low_pm"], high_pm=p["high_pm"])
    return g


def _on_target(clip, boxes):
    return clip["mk"].first_on_target(np.asarray(boxes), clip["fx"])


# ---- (a) the keys ---------------------------------------------------------------------------------------------------

def test_keys_are_accepted_and_the_enable_needs_the_appearance_store(gpu, weights_tiny, clip, dev):
    g = gpu.Group(weights_tiny, n_streams=1)
    g.init_device(0, dev[0][0], gpu.BBox.new(*clip["box0"]))
    for k, v in KEYS.items():
        if k != "arbitrate":
            g.set_tuning(k, v)                      # a field before the enable: accepted, nothing allocated
    with pytest.raises(gpu.VtError) as ei:
        g.set_tuning("arbitrate", 1)
    assert ei.value.code == INVALID and "appearance-capable" in str(ei.value)
    with pytest.raises(gpu.VtError) as ei:
        g.read_tensor("arbitrate", 0)
    assert ei.value.code == INVALID
    g.set_appearance(True)
    before = g.graph_captures()
    for k, v in KEYS.items():
        g.set_tuning(k, v)
    assert g.graph_captures() > before              # the passes were captured again with the four launches
    for k, v in (("arbitrate_max", 5), ("arbitrate_max", 1), ("arbitrate_radius", 0), ("arbitrate_low_pm", 1001), ("arbitrate", 2)):
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning(k, v)
        assert ei.value.code == INVALID and k in str(ei.value)
    with pytest.raises(gpu.VtError):
        g.set_tuning("arbitrate_tau", 1)
    a = g.arbitration(0)
    assert a["on"] == 1 and a["status"] == 0 and a["n"] == 0 and a["evaluated"] == 0
    r = g.update_device([dev[0][1]])
    a = g.arbitration(0)
    assert r[0].success and a["frames_done"] == 1 and a["status"] in (0, 1)
    names = {k["name"] for k in g.profile_device([dev[0][2]], iters=1)}
    assert {"arbitrate_list", "arbitrate_probe", "arbitrate_score", "arbitrate_commit"} <= names
    g.init_device(0, dev[0][0], gpu.BBox.new(*clip["box0"]))
    assert g.arbitration(0)["frames_done"] == 0     # init zeroes the record
    g.close()


# ---- (b) inert and switched off: the plain engine's bits ---------------------------------------------------------------------

def test_low_0_and_switched_off_equal_a_plain_engine(gpu, weights_tiny, clip, dev):
    frames = dev[0]
    main, plain = (_engine(gpu, weights_tiny, clip, frames[0], arbitrate=False) for _ in range(2))
    for g in (main, plain):
        g.set_template_refresh(2, 0.0)
        g.set_appearance(True, period=1, gate=0.3)
        g.enable_chips(32, gpu.CHIP_RGB8)
        g.set_chips(2.0)
        g.set_motion_prior(True)
        g.set_peaks(3, 1, 0.05)
    p = clip["pol"]
    main.set_arbitration(True, max=p["max_peaks"], radius=p["radius"], min_resp_pm=p["min_resp_pm"], low_pm=0, high_pm=p["high_pm"])
    due = 0
    for t in range(clip["n"]):
        if t == 92:
            main.set_arbitration(False)             # back to 0 for the rest of the clip
        rm, rp = main.update_device([frames[t]]), plain.update_device([frames[t]])
        assert [_res(r) for r in rm] == [_res(r) for r in rp], t
        assert np.array_equal(_state(main), _state(plain)) and np.array_equal(_tpl(main), _tpl(plain)), t
        assert main.appearance(0) == plain.appearance(0), t
        assert main.last_peaks().tobytes() == plain.last_peaks().tobytes(), t
        a = main.arbitration(0)
        assert a["status"] in (0, 1, 4) and a["switched"] == 0, (t, a)
        due += a["status"] == 1
    assert due >= 3, "the inert option never evaluated a slot: the identity shows nothing"
    assert main.arbitration(0)["status"] == 0 and main.arbitration(0)["n"] == 0
    main.close()
    plain.close()


# ---- (c) the host twin ---------------------------------------------------------------------------------------------------------

def test_twin_identity_with_a_host_that_applies_the_rule(gpu, weights_tiny, clip, dev):
    frames = dev[0]
    pol = clip["pol"]
    main = _engine(gpu, weights_tiny, clip, frames[0])
    twin = _engine(gpu, weights_tiny, clip, frames[0], arbitrate=False)
    helper = gpu.Group(weights_tiny, n_streams=1)
    for g in (main, twin):
        g.set_peaks(pol["max_peaks"], pol["radius"], float(ar.threshold(pol["min_resp_pm"])))
    mi = main.model_info()
    cols = 3 * mi.patch ** 2
    anchor = _bits(twin, "anchor")
    assert np.array_equal(anchor, _bits(main, "anchor"))
    thr = float(np.float32(0.2))            # the blob's success threshold
    switches, boxes_main, boxes_plain = [], [], []
    plain = _engine(gpu, weights_tiny, clip, frames[0], arbitrate=False)
    for t in range(clip["n"]):
        rm, rt = main.update_device([frames[t]]), twin.update_device([frames[t]])
        boxes_plain.append(plain.update_device([frames[t]])[0].bbox)
        st = twin.read_state(0)
        lst = ar.lists_of_records(twin.last_peaks(1), pol["max_peaks"])

        def sims_of(k, ibox):
            helper.init_device(0, frames[t], gpu.BBox.new(*(int(v) for v in ibox)))
            one = gpu.op_appearance_score(anchor[None], _bits(helper, "template")[None], cols)
            return int(one["status"][0]), one["similarity"][0]
        d = ar.decide(lst, 0, sims_of, state=st, success=int(rt[0].success), frame_wh=(clip["W"], clip["H"]), T=mi.template_size,
                      S=mi.search_size, success_threshold=thr, policy=pol)
        a = main.arbitration(0)
        assert (a["status"], a["n"], a["chosen"], a["frames_done"]) == (d["status"], d["n"], d["chosen"], st["frames_done"]), (t, a, d)
        for k in range(d["n"]):
            assert a["peaks"][k]["status"] == d["peak_status"][k] and a["peaks"][k]["similarity"].tobytes() == F(d["sim"][k]).tobytes(), (t, k, a, d)
            assert a["peaks"][k]["cell"] == lst["cell"][0, k] and a["peaks"][k]["box"].tobytes() == lst["fbox"][0, k].tobytes(), (t, k)
        if d["status"] == ar.SWITCHED:
            k = d["chosen"]
            ib = ar.int_box(lst["fbox"][0, k])
            twin.set_state_box(0, ib)
            switches.append(t)
            # the switched pass's result record against the peak's record
            assert rm[0].success and np.float32(rm[0].score).tobytes() == F(lst["score"][0, k]).tobytes(), (t, rm[0])
            assert tuple(rm[0].bbox) == tuple(int(v) for v in ib), (t, rm[0].bbox, ib)
            sm = main.read_state(0)
            assert sm["last_idx"] == lst["cell"][0, k] and sm["last_fbox"].tobytes() == lst["fbox"][0, k].tobytes()
            assert np.float32(sm["last_score"]).tobytes() == F(lst["score"][0, k]).tobytes()
            assert sm["box"].tobytes() == ib.tobytes() and (sm["frames_done"], sm["success_count"]) == (st["frames_done"], st["success_count"])
        else:
            assert _res(rm[0]) == _res(rt[0]), t                                   # every other result, before and after
            assert np.array_equal(_state(main), _state(twin)), t                     # and every state word
        boxes_main.append(rm[0].bbox)
    assert len(switches) >= 1, "no switch on the device"
    assert main.arbitration(0)["switched"] == len(switches)
    assert _on_target(clip, boxes_main) < _on_target(clip, boxes_plain), (switches, _on_target(clip, boxes_main), _on_target(clip, boxes_plain))
    for g in (main, twin, plain, helper):
        g.close()


# ---- (d) pipelined host passes ----------------------------------------------------------------------------------------------

def test_pipelined_host_passes_equal_synchronous_ones_across_the_switch(gpu, weights_tiny, clip, capsys):
    rgb = clip["rgb"]
    sync, pipe = (_engine(gpu, weights_tiny, clip, rgb[0], host=True) for _ in range(2))
    want, recs = [], []
    for t in range(clip["n"]):
        want.append(_res(sync.update_host([rgb[t]])[0]))
        recs.append(sync.arbitration(0))
    got, got_recs = [], []
    pipe.enqueue_host([rgb[0]])
    for t in range(1, clip["n"]):
        pipe.enqueue_host([rgb[t]])
        got.append(_res(pipe.wait_next()[0]))
        got_recs.append(pipe.arbitration(0))
    got.append(_res(pipe.wait_next()[0]))
    got_recs.append(pipe.arbitration(0))
    assert got == want
    # the by-stream mirrors of a pipelined run are compared where both runs have collected the same pass: at the end (between
    # two waits the engine's mirror may already hold the record of a redone pass's successor)
    a, b = got_recs[-1], recs[-1]
    assert (a["status"], a["chosen"], a["n"], a["frames_done"]) == (b["status"], b["chosen"], b["n"], b["frames_done"]), (a, b)
    assert [p["similarity"].tobytes() for p in a["peaks"]] == [p["similarity"].tobytes() for p in b["peaks"]]
    switched = [t for t, r in enumerate(recs) if r["status"] == 2]
    assert len(switched) >= 1, "no switch in the synchronous run"
    assert want[switched[0]][0] == tuple(int(v) for v in ar.int_box(recs[switched[0]]["peaks"][recs[switched[0]]["chosen"]]["box"]))
    assert pipe.arbitration(0)["switched"] >= len(switched)         # a redone pass may count twice
    assert np.array_equal(_state(sync), _state(pipe))
    with capsys.disabled():
        print(f"\n[arbitrate pipelined] redos {pipe.host_redos()}, switches at {[t for t, r in enumerate(recs) if r['status'] == 2]}")
    sync.close()
    pipe.close()


# ---- (e) candidate passes, (f) subset passes -----------------------------------------------------------------------------------

def test_a_candidate_pass_leaves_status_3_and_an_unchanged_result(gpu, weights_tiny, clip, dev):
    frames = dev[0]
    main = _engine(gpu, weights_tiny, clip, frames[0], B=2)
    plain = _engine(gpu, weights_tiny, clip, frames[0], B=2, arbitrate=False)
    for t in range(3):
        assert [_res(r) for r in main.update_device([frames[t]] * 2)] == [_res(r) for r in plain.update_device([frames[t]] * 2)]
    before = main.read_tensor("arbitrate", 1).tobytes()
    box = main.read_state(0)["box"]
    cands = [(0, None), (0, [float(box[0]) + 6, float(box[1]) - 4, float(box[2]), float(box[3])])]
    (rm, wm), (rp, wp) = main.update_device_candidates(cands, [frames[3]] * 2), plain.update_device_candidates(cands, [frames[3]] * 2)
    assert wm == wp and [_res(r) for r in rm] == [_res(r) for r in rp]
    a = main.arbitration(0)
    assert a["status"] == 3 and a["n"] == 0 and a["frames_done"] == main.read_state(0)["frames_done"]
    assert np.array_equal(_state(main), _state(plain))
    assert main.read_tensor("arbitrate", 1).tobytes() == before     # a stream the candidate pass does not name keeps its record
    main.close()
    plain.close()


def test_a_subset_pass_arbitrates_its_listed_streams_only(gpu, weights_tiny, clip, dev):
    """two streams on the same clip; stream 1 sits out the passes from the first due one on: its record stays the one of its
    last pass, stream 0's goes on to the switch"""
    frames = dev[0]
    g = _engine(gpu, weights_tiny, clip, frames[0], B=2)
    single = _engine(gpu, weights_tiny, clip, frames[0])
    first_due = int(np.flatnonzero(clip["fx"]["arb_status"] >= 1)[1])       # behind the occlusion's first frame
    frozen = None
    for t in range(clip["n"]):
        want = _res(single.update_device([frames[t]])[0])
        if t < first_due:
            r = g.update_device([frames[t], frames[t]])
            assert _res(r[0]) == want and _res(r[1]) == want, t
            frozen = g.arbitration(1)
        else:
            r = g.update_device([frames[t]], streams=[0])
            assert _res(r[0]) == want, t
            now = g.arbitration(1)
            assert (now["status"], now["frames_done"], now["n"], now["evaluated"]) == (frozen["status"], frozen["frames_done"], frozen["n"], frozen["evaluated"]), t
        a, b = g.arbitration(0), single.arbitration(0)
        assert (a["status"], a["chosen"], a["frames_done"]) == (b["status"], b["chosen"], b["frames_done"]), (t, a, b)
    assert g.arbitration(0)["switched"] >= 1 and g.arbitration(1)["switched"] == 0
    g.close()
    single.close()
