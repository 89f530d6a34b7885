"""The first enable of the seven optional in-the-pass features - template refresh, target chips, response peaks, result
overlay, motion prior, appearance check, reacquire proposals - as ONE behaviour, on the MI355X.

Tiny model, 3 streams on 640 x 480 MovingSquare NV12 clips. Three properties that hold whatever the host code behind the
enables looks like:
  * the order of the enables does not matter: two engines that enable the seven in opposite orders give the same bits on
    every kind of pass (full, subset, candidate, synchronous host, pipelined host);
  * nor does it matter whether the pipelined slots owned their sinks before an enable or got them afterwards;
  * a first enable captures every wanted graph set exactly once; a repeated enable, a later key and a pass capture nothing;
  * a call refused for its arguments leaves nothing behind: no capture, the feature still "not enabled", the next pass
    that of an untouched engine."""
import numpy as np
import pytest

from test_gpu_stream_subsets import H, INVALID, W, _clips, _frames_at, _init_all, _res

pytestmark = pytest.mark.gpu

B = 3
_cache = {}


def _scs(gpu):
    if "scs" not in _cache:
        _cache["scs"] = _clips(gpu, B)
    return _cache["scs"]


def _group(gpu, weights):
    """a group of B streams initialised on frame 0 of their clips"""
    g = gpu.Group(weights, n_streams=B)
    frames0, keep0 = _frames_at(gpu, _scs(gpu), 0)
    _init_all(gpu, g, frames0, _scs(gpu))
    return g


def _host_frames(gpu, t, streams=range(B)):
    return [gpu.NV12Frame(_scs(gpu)[s].frame_nv12(t), W, H) for s in streams]


ENABLES = {
    "refresh": lambda g, gpu: g.set_template_refresh(2, 0.0),
    "chips": lambda g, gpu: (g.enable_chips(32, gpu.CHIP_RGB8), g.set_chips(2.0)),
    "peaks": lambda g, gpu: g.set_peaks(3),
    "overlay": lambda g, gpu: g.set_tuning("result_overlay", 7),
    "motion": lambda g, gpu: g.set_tuning("motion_prior", 1),
    "appearance": lambda g, gpu: g.set_tuning("appearance", 1),
    "proposals": lambda g, gpu: g.set_tuning("proposals", 2),       # mode 2: every update evaluates
}
ORDER = ["refresh", "chips", "peaks", "overlay", "motion", "appearance", "proposals"]


def _observe(g):
    """everything the seven features and the tracker itself let the host see, as exact values"""
    chips, infos = g.read_chips()
    return dict(
        states=[g.read_tensor("state", s).tobytes() for s in range(B)],
        peaks=g.last_peaks().tobytes(),
        chips=chips.tobytes(), chip_infos=infos,
        motion=[g.motion(s) for s in range(B)],
        overlay=[g.result_overlay_stats(s) for s in range(B)],
        appearance=[g.appearance(s) for s in range(B)], anchors=[g.anchor(s).tobytes() for s in range(B)],
        proposals=[g.proposals(s) for s in range(B)],
        refresh=[g.template_refresh_stats(s) for s in range(B)])


def _same(a, b, results, what):
    ra, rb = results
    assert [_res(r) for r in ra] == [_res(r) for r in rb], f"{what}: results differ"
    oa, ob = _observe(a), _observe(b)
    for key in oa:
        assert oa[key] == ob[key], f"{what}: {key} differs between the two enable orders"


def test_enable_order_does_not_matter_bit_for_bit(gpu, weights_tiny, capsys):
    """engine a enables refresh, chips, peaks, overlay, motion, appearance, proposals; engine b the same in reverse; then two full device passes, a
    subset pass (slot != stream), a candidate pass, a synchronous host pass and two pipelined host passes two deep. Each
    engine has its own copies of the device frames: the overlay draws into them."""
    scs = _scs(gpu)
    a, b = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    for name in ORDER:
        ENABLES[name](a, gpu)
    for name in reversed(ORDER):
        ENABLES[name](b, gpu)
    caps = a.graph_captures()
    assert caps == b.graph_captures()
    t = 0

    def dev():
        fa, ka = _frames_at(gpu, scs, t)
        fb, kb = _frames_at(gpu, scs, t)
        return fa, fb, (ka, kb)

    for _ in range(2):
        t += 1
        fa, fb, keep = dev()
        _same(a, b, (a.update_device(fa), b.update_device(fb)), f"full device pass {t}")
    t += 1
    fa, fb, keep = dev()
    L = [2, 0]
    _same(a, b, (a.update_device([fa[s] for s in L], streams=L), b.update_device([fb[s] for s in L], streams=L)), "subset pass")
    t += 1
    fa, fb, keep = dev()
    box = a.read_state(1)["box"]
    assert box.tobytes() == b.read_state(1)["box"].tobytes()
    x, y, w, h = (float(v) for v in box)
    cands = [(1, (x + 6, y - 4, w, h)), (1, (x - 10, y + 8, w, h)), (2, None)]
    (ra, wa), (rb, wb) = (a.update_device_candidates(cands, [fa[1], fa[1], fa[2]]),
                          b.update_device_candidates(cands, [fb[1], fb[1], fb[2]]))
    assert wa == wb and wa[0] == wa[1] and wa[2] == 2
    _same(a, b, (ra, rb), "candidate pass")
    t += 1
    _same(a, b, (a.update_host(_host_frames(gpu, t)), b.update_host(_host_frames(gpu, t))), "synchronous host pass")
    for g in (a, b):
        g.enqueue_host(_host_frames(gpu, t + 1))
        g.enqueue_host(_host_frames(gpu, t + 2))
    ra, rb = a.wait_next(), b.wait_next()       # the second pass is still outstanding: what this one returned, no more
    assert [_res(r) for r in ra] == [_res(r) for r in rb], "pipelined host pass 1: results differ"
    assert a.last_peaks().tobytes() == b.last_peaks().tobytes(), "pipelined host pass 1: peaks differ"
    _same(a, b, (a.wait_next(), b.wait_next()), "pipelined host pass 2")
    did = dict(refreshes=sum(a.template_refresh_stats(s)["generation"] for s in range(B)),
               shifts=sum(a.motion(s)["n_shift"] for s in range(B)),
               drawn=sum(a.result_overlay_stats(s)["n_drawn"] for s in range(B)),
               peaks=int(a.last_peaks()["n"].sum()), chips=sum(i["status"] == 1 for i in a.read_chips()[1]),
               appearance=sum(a.appearance(s)["evaluated"] for s in range(B)),
               proposals=sum(a.proposals(s)["evaluated"] for s in range(B)))
    with capsys.disabled():
        print(f"\n[enable order] {did}")
    assert min(did.values()) >= 1, f"the run exercises little: a feature did nothing: {did}"
    assert a.graph_captures() == caps and b.graph_captures() == caps
    a.close()
    b.close()


def test_a_first_enable_captures_once_and_nothing_else_captures(gpu, weights_tiny):
    scs = _scs(gpu)
    g = gpu.Group(weights_tiny, n_streams=B)
    c0 = g.graph_captures()
    assert c0 > 0
    frames0, keep0 = _frames_at(gpu, scs, 0)
    _init_all(gpu, g, frames0, scs)
    assert g.graph_captures() == c0, "an init on NV12 captured"
    later = {
        "refresh": [lambda: g.set_template_refresh(3, 0.5, stream=1), lambda: g.set_template_refresh(0)],
        "chips": [lambda: g.set_chips(2.0), lambda: g.set_chips(1.5, 2, 1, stream=0)],
        "peaks": [lambda: g.set_peaks(5, 1, 0.25, stream=2), lambda: g.set_peaks(0)],
        "overlay": [lambda: g.set_tuning("result_overlay_luma", 200), lambda: g.set_tuning("result_overlay_style", 2 | 9 << 8 | 1 << 16),
                    lambda: g.set_tuning("result_overlay", 0), lambda: g.set_tuning("result_overlay", 7)],
        "motion": [lambda: g.set_tuning("motion_gain_pct", 70), lambda: g.set_tuning("motion_coast", 3),
                   lambda: g.set_tuning("motion_prior", 0), lambda: g.set_tuning("motion_prior", 1)],
        "appearance": [lambda: g.set_tuning("appearance_period", 2), lambda: g.set_tuning("appearance_gate_pm", 900),
                       lambda: g.set_tuning("appearance_anchor", 1)],
        "proposals": [lambda: g.set_tuning("proposals_period", 2), lambda: g.set_tuning("proposals_max", 3),
                      lambda: g.set_tuning("proposals_min_sim_pm", 250)],
    }
    caps = c0
    for name in ORDER:
        ENABLES[name](g, gpu)
        caps += c0
        assert g.graph_captures() == caps, f"{name}: the first enable did not capture every graph exactly once"
        ENABLES[name](g, gpu)
        assert g.graph_captures() == caps, f"{name}: the repeated enable captured"
        for call in later[name]:
            call()
            assert g.graph_captures() == caps, f"{name}: a later key captured"
    f1, keep1 = _frames_at(gpu, scs, 1)
    g.update_device(f1)
    g.update_device([f1[2], f1[0]], streams=[2, 0])
    g.update_device_candidates([(1, (300.0, 200.0, 50.0, 50.0)), (1, None), 0], [f1[1], f1[1], f1[0]])
    g.update_host(_host_frames(gpu, 2))
    g.update_host(_host_frames(gpu, 3, [1]), streams=[1])
    g.enqueue_host(_host_frames(gpu, 4))
    g.enqueue_host(_host_frames(gpu, 5, [2, 1]), streams=[2, 1])
    g.wait_next()
    g.wait_next()
    assert g.graph_captures() == caps, "a pass captured"
    g.close()


REFUSED = {
    "refresh": lambda g, gpu: g.set_template_refresh(1),
    "chips": lambda g, gpu: g.enable_chips(33, gpu.CHIP_RGB8),
    "peaks": lambda g, gpu: g.set_peaks(3, 9),
    "overlay": lambda g, gpu: g.set_tuning("result_overlay", 8),
    "motion": lambda g, gpu: g.set_tuning("motion_gain_pct", 0),
    "appearance": lambda g, gpu: g.set_tuning("appearance_period", 0),
    "proposals": lambda g, gpu: g.set_tuning("proposals_max", 0),
}


def _untouched_pass(gpu, weights):
    """the first full pass of an engine nobody configured: (its frames, results, state words) - made once"""
    if "plain" not in _cache:
        g = _group(gpu, weights)
        f1, keep1 = _frames_at(gpu, _scs(gpu), 1)
        res = [_res(r) for r in g.update_device(f1)]
        _cache["plain"] = (f1, keep1, res, [g.read_tensor("state", s).tobytes() for s in range(B)])
        g.close()
    return _cache["plain"]


@pytest.mark.parametrize("feature", ORDER)
def test_a_refused_enable_leaves_nothing_behind(gpu, weights_tiny, feature):
    f1, keep1, res, states = _untouched_pass(gpu, weights_tiny)
    g = _group(gpu, weights_tiny)
    caps = g.graph_captures()
    with pytest.raises(gpu.VtError) as ei:
        REFUSED[feature](g, gpu)
    assert ei.value.code == INVALID
    assert g.graph_captures() == caps
    for not_enabled in (g.last_peaks, g.read_chips, lambda: g.read_tensor("motion", 0), lambda: g.read_tensor("result_overlay", 0),
                        lambda: g.read_tensor("appearance", 0), lambda: g.read_tensor("anchor", 0), lambda: g.read_tensor("proposals", 0)):
        with pytest.raises(gpu.VtError) as ei:
            not_enabled()
        assert ei.value.code == INVALID
    assert all(g.template_refresh_stats(s)["period"] == 0 for s in range(B))
    assert [_res(r) for r in g.update_device(f1)] == res
    assert [g.read_tensor("state", s).tobytes() for s in range(B)] == states
    assert g.graph_captures() == caps
    g.close()


def test_slots_that_owned_sinks_before_the_enable_get_the_new_ones(gpu, weights_tiny):
    """engine a enables peaks, motion, appearance and proposals before any pass, so its pipelined slots get all their
    sinks at their first use. Engine b first runs and collects two pipelined host passes - both slots own their base
    sinks - and enables afterwards: the enable itself must give those slots the new members. a runs the same two passes
    before it is compared - capable, but with the three keyed policies switched off for them, or its motion record and
    its counters would be two passes ahead of b's by design; then two more pipelined passes two deep on both: the same
    bits everywhere."""
    a, b = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    sinks = ["peaks", "motion", "appearance", "proposals"]
    for name in sinks:
        ENABLES[name](a, gpu)
    for key in ("motion_prior", "appearance", "proposals"):
        a.set_tuning(key, 0)
    caps = a.graph_captures()
    before = []
    for g in (b, a):
        g.enqueue_host(_host_frames(gpu, 1))
        g.enqueue_host(_host_frames(gpu, 2))
        before.append([[_res(r) for r in g.wait_next()], [_res(r) for r in g.wait_next()]])
    assert before[0] == before[1], "the features changed the results of the two passes ahead of b's enables"
    for name in sinks:
        ENABLES[name](a, gpu)       # a is capable: the policies go on again, nothing is captured
        ENABLES[name](b, gpu)
    assert a.graph_captures() == caps
    for g in (a, b):
        g.enqueue_host(_host_frames(gpu, 3))
        g.enqueue_host(_host_frames(gpu, 4))

    def seen(g):
        return dict(states=[g.read_tensor("state", s).tobytes() for s in range(B)], peaks=g.last_peaks().tobytes(),
                    motion=[g.motion(s) for s in range(B)], appearance=[g.appearance(s) for s in range(B)],
                    proposals=[g.proposals(s) for s in range(B)])

    for k in (1, 2):
        ra, rb = a.wait_next(), b.wait_next()
        assert [_res(r) for r in ra] == [_res(r) for r in rb], f"pipelined pass {k} after the enables: results differ"
        assert a.last_peaks().tobytes() == b.last_peaks().tobytes(), f"pipelined pass {k} after the enables: peaks differ"
    sa, sb = seen(a), seen(b)
    for key in sa:
        assert sa[key] == sb[key], f"{key} differs between slots that had sinks before the enable and slots that had none"
    assert int(a.last_peaks()["n"].sum()) >= 1 and all(sb["appearance"][s]["status"] == 1 for s in range(B))
    a.close()
    b.close()
