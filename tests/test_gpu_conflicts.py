"""Stream conflicts, engine level ("conflicts*" keys of vt_group_set_tuning), on the MI355X.

Tiny model, four streams on 640 x 480 MovingSquare NV12 clips. Streams 0, 1 and 2 show the SAME clip (scene 1): 0 is started
on the target, 1 on a box shifted by SHIFT of its side - both land on the square -, 2 on a box far away; stream 3 shows
another clip (scene 2). After every collected pass each stream's record is compared with the NumPy model of
tests/conflicts_util.py run on that pass's final states and results."""
import importlib

import numpy as np
import pytest

import conflicts_util as cu
from test_gpu_stream_subsets import H, INVALID, W, _dev as _dev_buf, _res
from test_gpu_template_refresh import _tpl

pytestmark = pytest.mark.gpu

F = np.float32
B = 4
OOM = -8
SIDE = 64
SHIFT = 1.0 / 3.0       # of the side, along x and y: chosen on the GPU - both streams land on the square (IoU >= 0.3 every pass)
FAR = (40, 380, 64, 64)         # stream 2: a piece of background of the same picture
SCENES = [1, 1, 1, 2]
_cache = {}


def _scs(gpu):
    if "scs" not in _cache:
        a = gpu.synth.MovingSquare(W, H, SIDE, seed=3)
        _cache["scs"] = [a, a, a, gpu.synth.MovingSquare(W, H, SIDE, seed=4)]
    return _cache["scs"]


def _boxes0(gpu):
    x, y, w, h = _scs(gpu)[0].gt_box(0)
    d = int(round(SHIFT * w))
    return [(x, y, w, h), (x + d, y + d, w, h), FAR, _scs(gpu)[3].gt_box(0)]


def _frames(gpu, t, streams=range(B)):
    """device frames of clip time t, one copy per listed stream (the overlay draws into them) + the tensors that own them"""
    pairs = [_dev_buf(gpu, _scs(gpu)[s].frame_nv12(t)) for s in streams]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _host(gpu, t, streams=range(B)):
    return [gpu.NV12Frame(_scs(gpu)[s].frame_nv12(t), W, H) for s in streams]


def _group(gpu, weights, **kw):
    g = gpu.Group(weights, n_streams=B, **kw)
    f0, keep = _frames(gpu, 0)
    for s, b in enumerate(_boxes0(gpu)):
        g.init_device(s, f0[s], gpu.BBox.new(*b))
    return g


def _scenes(g, scenes=SCENES):
    for s, sc in enumerate(scenes):
        g.set_scene(s, sc)


def _states(gpu, g):
    STATE = importlib.import_module(gpu.__name__ + ".snapshot").STATE
    return np.concatenate([np.frombuffer(g.read_tensor("state", s).tobytes(), STATE) for s in range(B)])


def _rec(g, s):
    c = g.conflicts(s)
    r = cu.record(c["status"], c["frames_done"], c["n_over"])
    r["partner"], r["iou"] = c["partner"], c["iou"]
    return r


def _check_records(gpu, g, results, streams=None, winner=None, pm=300, scenes=SCENES):
    """the records of the pass's streams against the model on the pass's final states and results -> {stream: status}"""
    want = cu.check_states(_states(gpu, g), results, scenes, pm=pm, slot_stream=streams, winner=winner)
    for s, r in want.items():
        assert _rec(g, s).tobytes() == r.tobytes(), f"stream {s}: record {g.conflicts(s)}, model {r}"
    return {s: int(r["status"]) for s, r in want.items()}


OTHERS = [lambda g, gpu: g.set_template_refresh(2, 0.0), lambda g, gpu: (g.enable_chips(32, gpu.CHIP_RGB8), g.set_chips(2.0)),
          lambda g, gpu: g.set_peaks(3), lambda g, gpu: g.set_tuning("result_overlay", 7),
          lambda g, gpu: g.set_tuning("motion_prior", 1), lambda g, gpu: g.set_tuning("appearance", 1),
          lambda g, gpu: g.set_tuning("proposals", 2)]


def _observe(g):
    """everything the other seven features and the tracker itself let the host see, as exact values"""
    chips, infos = g.read_chips()
    return dict(states=[g.read_tensor("state", s).tobytes() for s in range(B)], templates=[_tpl(g, s).tobytes() for s in range(B)],
                peaks=g.last_peaks().tobytes(), chips=chips.tobytes(), chip_infos=infos, motion=[g.motion(s) for s in range(B)],
                overlay=[g.result_overlay_stats(s) for s in range(B)], appearance=[g.appearance(s) for s in range(B)],
                anchors=[g.anchor(s).tobytes() for s in range(B)], proposals=[g.proposals(s) for s in range(B)],
                refresh=[g.template_refresh_stats(s) for s in range(B)])


def _same(a, b, ra, rb, what, drawn=None):
    assert [_res(r) for r in ra] == [_res(r) for r in rb], f"{what}: results differ"
    oa, ob = _observe(a), _observe(b)
    for key in oa:
        assert oa[key] == ob[key], f"{what}: {key} differs between the enabled engine and the plain one"
    if drawn:
        assert all(bool((x == y).all()) for x, y in zip(*drawn)), f"{what}: the drawn frames differ"


# ---- 1. the read-only twin --------------------------------------------------------------------------------------------------

def test_read_only_twin_on_every_kind_of_pass(gpu, weights_tiny, capsys):
    """gate 0, the other seven features on in both engines: the enabled engine equals the plain one in every bit the host can
    see, over two full device passes, a subset pass, a candidate pass, a synchronous host pass and two pipelined host passes
    two deep; every collected pass's records equal the model"""
    main, plain = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    for g in (main, plain):
        for enable in OTHERS:
            enable(g, gpu)
    main.set_conflicts(True)
    _scenes(main)
    seen, t = [], 0
    for _ in range(2):
        t += 1
        (fa, ka), (fb, kb) = _frames(gpu, t), _frames(gpu, t)
        ra, rb = main.update_device(fa), plain.update_device(fb)
        _same(main, plain, ra, rb, f"full device pass {t}", (ka, kb))
        seen.append(_check_records(gpu, main, ra))
    t += 1
    L = [1, 3, 0]
    (fa, ka), (fb, kb) = _frames(gpu, t, L), _frames(gpu, t, L)
    kept = _rec(main, 2).tobytes()
    ra, rb = main.update_device(fa, streams=L), plain.update_device(fb, streams=L)
    _same(main, plain, ra, rb, "subset pass", (ka, kb))
    seen.append(_check_records(gpu, main, ra, streams=L))
    assert _rec(main, 2).tobytes() == kept, "a stream that was not in the pass lost its record"
    t += 1
    x, y, w, h = (float(v) for v in main.read_state(0)["box"])
    cands = [(0, (x + 5, y - 4, w, h)), (0, None), 1, (3, None)]
    slots = [0, 0, 1, 3]
    (fa, ka), (fb, kb) = _frames(gpu, t, slots), _frames(gpu, t, slots)
    (ra, wa), (rb, wb) = main.update_device_candidates(cands, fa), plain.update_device_candidates(cands, fb)
    assert wa == wb and wa[0] == wa[1]
    _same(main, plain, ra, rb, "candidate pass", (ka, kb))
    seen.append(_check_records(gpu, main, ra, streams=slots, winner=wa))
    t += 1
    ra, rb = main.update_host(_host(gpu, t)), plain.update_host(_host(gpu, t))
    _same(main, plain, ra, rb, "synchronous host pass")
    seen.append(_check_records(gpu, main, ra))
    for g in (main, plain):
        g.enqueue_host(_host(gpu, t + 1))
        g.enqueue_host(_host(gpu, t + 2))
    ra, rb = main.wait_next(), plain.wait_next()        # the second pass is still outstanding: the mirror shows this one
    assert [_res(r) for r in ra] == [_res(r) for r in rb], "pipelined host pass 1: results differ"
    first = [_rec(main, s) for s in range(B)]
    assert all(r["frames_done"] == first[0]["frames_done"] for r in first[:2]) and {int(r["status"]) for r in first} <= {1, 2, 3}
    ra, rb = main.wait_next(), plain.wait_next()
    _same(main, plain, ra, rb, "pipelined host pass 2")
    seen.append(_check_records(gpu, main, ra))
    assert all(int(_rec(main, s)["frames_done"]) == int(first[s]["frames_done"]) + 1 for s in (0, 1, 3))
    statuses = sorted({v for d in seen for v in d.values()})
    with capsys.disabled():
        print(f"\n[conflicts twin] statuses per pass {seen}; counters {[main.conflicts(s) for s in range(B)]}")
    assert statuses == [1, 2, 3], f"the run must show every status, it shows {statuses}"
    assert all(d[0] == 2 and d[1] == 2 for d in seen), "streams 0 and 1 sit on one square: both conflict in every pass"
    assert sum(main.template_refresh_stats(s)["generation"] for s in range(B)) >= 3 and main.conflicts(0)["gated"] == 0
    main.close()
    plain.close()


# ---- 2. the gate -------------------------------------------------------------------------------------------------------------

def test_gate_equals_a_host_twin_under_rule_9(gpu, weights_tiny, capsys):
    """main: refresh (period 2), conflicts and the gate; twin: refresh off, re-initialised by the host where the model's rules
    1-9 fire. After four updates stream 1 leaves the scene: stream 0 is alone from then on and refreshes again."""
    main, twin = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    mi = main.model_info()
    main.set_template_refresh(2, 0.0)
    main.set_conflicts(True, gate=True)
    scenes = list(SCENES)
    _scenes(main, scenes)
    rules = [cu.Rule(mi.template_size, mi.search_size, 2, 0.0, conflicts_gate=True) for _ in range(B)]
    for t in range(1, 11):
        if t == 5:
            scenes[1] = 0
            main.set_scene(1, 0)
        (fa, ka), (fb, kb) = _frames(gpu, t), _frames(gpu, t)
        rm, rt = main.update_device(fa), twin.update_device(fb)
        assert [_res(r) for r in rm] == [_res(r) for r in rt], f"update {t}"
        st = _states(gpu, twin)
        want = cu.check_states(_states(gpu, main), rm, scenes)      # the restatement decides for the twin (whose frames_done restart with every re-initialisation)
        for s in range(B):
            assert _rec(main, s).tobytes() == want[s].tobytes(), f"update {t}, stream {s}"
            act = rules[s].step(rt[s], geo=st[s]["geo"], window_miss=st[s]["window_miss"] == st[s]["frames_done"],
                                conflict=int(want[s]["status"]))
            if act == "fire":
                twin.init_device(s, fb[s], gpu.BBox.new(*rt[s].bbox))
            got = main.template_refresh_stats(s)
            assert (got["generation"], got["last_frame"]) == (rules[s].generation, rules[s].last_frame), f"update {t}, stream {s}: {got} vs {act}"
            assert np.array_equal(_tpl(main, s), _tpl(twin, s)), f"update {t}, stream {s}: template rows differ"
    fired, gated = sum(len(r.fired) for r in rules), sum(len(r.conflict_gated) for r in rules)
    with capsys.disabled():
        print(f"\n[conflicts gate] fired {[r.fired for r in rules]}, gated {[r.conflict_gated for r in rules]}, skipped {[r.skipped for r in rules]}")
    assert fired >= 3 and gated >= 3 and len(rules[0].fired) >= 1 and len(rules[0].conflict_gated) >= 1
    assert [main.conflicts(s)["gated"] for s in range(B)] == [len(r.conflict_gated) for r in rules]
    main.set_tuning("conflicts_gate", 0)            # the gate off: stream 1 (still recorded as scene 0) and the others refresh as ever
    main.close()
    twin.close()


def test_pipelined_host_run_equals_the_synchronous_run_with_the_gate_on(gpu, weights_tiny):
    sync, pipe = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    for g in (sync, pipe):
        g.set_template_refresh(2, 0.0)
        g.set_conflicts(True, gate=True)
        _scenes(g)
    N = 7
    rs = [sync.update_host(_host(gpu, t)) for t in range(1, N + 1)]
    pipe.enqueue_host(_host(gpu, 1))
    rp = []
    for t in range(2, N + 1):
        pipe.enqueue_host(_host(gpu, t))
        rp.append(pipe.wait_next())
    rp.append(pipe.wait_next())
    assert [[_res(r) for r in p] for p in rs] == [[_res(r) for r in p] for p in rp]
    for s in range(B):
        assert sync.read_tensor("state", s).tobytes() == pipe.read_tensor("state", s).tobytes(), f"stream {s}: state"
        assert np.array_equal(_tpl(sync, s), _tpl(pipe, s)), f"stream {s}: template"
        cs, cp = sync.conflicts(s), pipe.conflicts(s)
        assert _rec(sync, s).tobytes() == _rec(pipe, s).tobytes(), f"stream {s}: record"
        if pipe.host_redos() == 0:      # the counters are diagnostics that are never rewound: a redone pass counts twice
            assert {k: cs[k] for k in ("evaluated", "conflicting", "gated")} == {k: cp[k] for k in ("evaluated", "conflicting", "gated")}
    assert sync.conflicts(0)["gated"] >= 2 and sync.template_refresh_stats(3)["generation"] >= 2
    sync.close()
    pipe.close()


# ---- 3. the records' life ----------------------------------------------------------------------------------------------------

def test_records_are_zeroed_by_everything_that_gives_a_stream_a_new_state(gpu, weights_tiny):
    g, other = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    g.set_conflicts(True)
    other.set_conflicts(True)
    _scenes(g)
    _scenes(other, [5, 5, 5, 5])
    zero = cu.record(0, 0)
    zero["partner"] = 0
    f0, k0 = _frames(gpu, 0)

    def run(engine=g):
        f1, k1 = _frames(gpu, 1)
        engine.update_device(f1)
        assert all(_rec(engine, s)["status"] != 0 for s in range(B))

    assert all(_rec(g, s).tobytes() == zero.tobytes() for s in range(B)), "records start as zeros"
    run()
    g.init_device(0, f0[0], gpu.BBox.new(*_boxes0(gpu)[0]))
    assert _rec(g, 0).tobytes() == zero.tobytes() and _rec(g, 1)["status"] == 2, "init zeroes its stream's record, and no other"
    assert [g.conflicts(s)["scene"] for s in range(B)] == SCENES, "scenes survive init"
    run()
    g.set_state_box(1, g.read_state(1)["box"])
    assert _rec(g, 1).tobytes() == zero.tobytes() and _rec(g, 0)["status"] == 2
    run()
    g.import_stream(2, g.export_stream(3))
    assert _rec(g, 2).tobytes() == zero.tobytes() and g.conflicts(2)["scene"] == 1, "import zeroes the record and keeps the scene"
    run(other)
    g.copy_stream(0, other, 3)
    assert _rec(other, 3).tobytes() == zero.tobytes() and other.conflicts(3)["scene"] == 5 and _rec(g, 0)["status"] != 0
    run()
    g.set_scene(3, 7)
    assert _rec(g, 3).tobytes() == zero.tobytes() and _rec(g, 0)["status"] != 0 and g.conflicts(3)["scene"] == 7
    g.set_scene(None, 9)
    assert all(_rec(g, s).tobytes() == zero.tobytes() and g.conflicts(s)["scene"] == 9 for s in range(B))
    run()
    g.set_tuning("conflicts_scene", -1)
    assert all(_rec(g, s).tobytes() == zero.tobytes() and g.conflicts(s)["scene"] == 0 for s in range(B))
    f2, k2 = _frames(gpu, 2)
    g.update_device(f2)
    assert all(_rec(g, s)["status"] == 3 for s in range(B)), "scene 0: compared with nobody"
    ev, recs = [g.conflicts(s)["evaluated"] for s in range(B)], [_rec(g, s).tobytes() for s in range(B)]
    g.set_tuning("conflicts", 0)        # the flag off: the launch writes nothing
    g.update_device(f2)
    assert [g.conflicts(s)["evaluated"] for s in range(B)] == ev and [_rec(g, s).tobytes() for s in range(B)] == recs
    g.close()
    other.close()


# ---- 4. enable semantics -----------------------------------------------------------------------------------------------------

def test_keys_enable_and_refusals(gpu, weights_tiny):
    g = _group(gpu, weights_tiny)
    caps = g.graph_captures()
    for call in (lambda: g.read_tensor("conflicts", 0), lambda: g.set_tuning("conflicts_scene", 1 << 16)):
        with pytest.raises(gpu.VtError) as ei:
            call()
        assert ei.value.code == INVALID and "not enabled" in str(ei.value)
    g.set_tuning("conflicts_iou_pm", 450)       # remembered until the enable
    g.set_tuning("conflicts_gate", 1)
    g.set_tuning("conflicts", 0)
    for key, bad in (("conflicts", 2), ("conflicts_iou_pm", 0), ("conflicts_iou_pm", 1001), ("conflicts_gate", 2), ("conflicts_nope", 1)):
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning(key, bad)
        assert ei.value.code == INVALID, (key, bad)
    assert g.graph_captures() == caps, "a refused or remembered key captured"
    with pytest.raises(gpu.VtError):
        g.read_tensor("conflicts", 0)           # a refused key ("conflicts_iou_pm" 0) left nothing behind
    g.set_tuning("conflicts", 1)
    c0 = gpu.Group(weights_tiny, n_streams=B)
    per_set = c0.graph_captures()
    c0.close()
    assert g.graph_captures() == caps + per_set, "the first enable captures every graph set exactly once"
    c = g.conflicts(2)
    assert (c["on"], c["status"], c["evaluated"], c["gated"], c["scene"], c["partner"]) == (1, 0, 0, 0, 0, [0, 0, 0, 0])
    g.set_tuning("conflicts", 1)
    g.set_tuning("conflicts_iou_pm", -1)
    g.set_tuning("conflicts_gate", -1)
    _scenes(g)
    for bad in (-2, B, 0xFFFE, B | 3 << 16):
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning("conflicts_scene", bad)
        assert ei.value.code == INVALID and [g.conflicts(s)["scene"] for s in range(B)] == SCENES
    f1, k1 = _frames(gpu, 1)
    g.update_device(f1)
    g.update_device([f1[2], f1[0]], streams=[2, 0])
    g.update_host(_host(gpu, 2))
    g.enqueue_host(_host(gpu, 3))
    with pytest.raises(gpu.VtError) as ei:
        g.set_tuning("conflicts_scene", 0)      # no key while a pipelined pass is outstanding
    assert ei.value.code == INVALID
    g.wait_next()
    assert g.graph_captures() == caps + per_set, "a repeated enable, a later key or a pass captured"
    g.close()


def test_enable_under_a_memory_cap_is_refused_and_nothing_changes(gpu, weights_tiny):
    """The store of 4 streams is 384 bytes and vt_config.max_device_mib counts whole MiB, so the smallest cap that creates the
    engine may well leave room for it. The room is therefore filled first, to within 24 bytes, by the one store whose size the
    host chooses finely: the proposals' (6 bytes per cell and stream, "proposals_max_cells"). The enable of the conflicts must
    then return VT_ERR_OOM and change nothing."""
    n = 4

    def create(mib):
        try:
            return gpu.Group(weights_tiny, n_streams=n, max_device_mib=mib, use_graph=False)
        except gpu.VtError as e:
            assert e.code == OOM
            return None

    lo, hi = 0, 4096
    while hi - lo > 1:
        mid = (lo + hi) // 2
        g = create(mid)
        if g is None:
            lo = mid
        else:
            g.close()
            hi = mid
    cap = hi + 1        # 1 to 2 MiB of room: more than the smallest proposals store of 4 streams (0.4 MiB), less than the largest

    def with_proposals(cells, mib=cap):
        g = create(mib)
        g.set_tuning("proposals_max_cells", cells)
        try:
            g.set_tuning("proposals", 1)
        except gpu.VtError as e:
            assert e.code == OOM
            g.close()
            return None
        return g

    lo, hi = 16384, 4194304
    g = with_proposals(lo)
    assert g is not None and with_proposals(hi) is None
    g.close()
    while hi - lo > 1:
        mid = (lo + hi) // 2
        g = with_proposals(mid)
        if g is None:
            hi = mid
        else:
            g.close()
            lo = mid
    g = with_proposals(lo)          # one more cell does not fit: less than 24 bytes are left
    f0, k0 = _frames(gpu, 0)
    for s, b in enumerate(_boxes0(gpu)):
        g.init_device(s, f0[s], gpu.BBox.new(*b))
    g.set_tuning("conflicts_iou_pm", 450)
    with pytest.raises(gpu.VtError) as ei:
        g.set_tuning("conflicts", 1)
    assert ei.value.code == OOM
    with pytest.raises(gpu.VtError) as ei:
        g.read_tensor("conflicts", 0)
    assert ei.value.code == INVALID, "the refused enable left the engine capable"
    f1, k1 = _frames(gpu, 1)
    assert all(r.success for r in g.update_device(f1)[:2])
    g.close()
    roomy = with_proposals(lo, cap + 1)
    roomy.set_tuning("conflicts_iou_pm", 450)
    roomy.set_tuning("conflicts", 1)
    assert roomy.conflicts(3)["on"] == 1
    roomy.close()


def test_enabling_first_or_last_among_the_eight_gives_the_same_bits(gpu, weights_tiny):
    a, b = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    a.set_conflicts(True, gate=True)
    _scenes(a)
    for g in (a, b):
        for enable in OTHERS:
            enable(g, gpu)
    b.set_conflicts(True, gate=True)
    _scenes(b)
    assert a.graph_captures() == b.graph_captures()
    for t in (1, 2, 3):
        (fa, ka), (fb, kb) = _frames(gpu, t), _frames(gpu, t)
        ra, rb = a.update_device(fa), b.update_device(fb)
        _same(a, b, ra, rb, f"pass {t}", (ka, kb))
        assert [a.conflicts(s) | {"iou": a.conflicts(s)["iou"].tobytes()} for s in range(B)] == \
            [b.conflicts(s) | {"iou": b.conflicts(s)["iou"].tobytes()} for s in range(B)]
    assert a.conflicts(0)["gated"] >= 1
    a.close()
    b.close()


def test_one_launch_per_pass_on_enabled_engines_only(gpu, weights_tiny):
    g = _group(gpu, weights_tiny)
    g.set_motion_prior(True)
    g.set_appearance(True)
    f0, k0 = _frames(gpu, 0)
    plain = g.profile_device(f0, iters=2)
    assert not [k for k in plain if k["name"].startswith("conflicts")]
    g.set_conflicts(True)
    fams = {k["name"]: k["launches"] for k in g.profile_device(f0, iters=2)}
    assert {n: c for n, c in fams.items() if n.startswith("conflicts")} == {"conflicts_check": 1}
    assert sum(fams.values()) == sum(k["launches"] for k in plain) + 1
    order = [k["name"] for k in g.profile_device(f0, iters=1)]
    assert order.index("conflicts_check") == order.index("motion_settle") + 1 == order.index("appearance_probe") - 1
    g.close()
