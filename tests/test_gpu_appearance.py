"""The appearance check (the "appearance*" keys of vt_group_set_tuning; DESIGN.md section 3, "Appearance check"), on the
MI355X.

Yardsticks: a PLAIN engine that never enables the check (the read-only twin: results, state words and templates bit for
bit); the template rows a twin engine writes at init(frame, result.bbox) and the oracle's crop there (the probe's bits);
the NumPy float64 restatement of tests/appearance_util.py (the similarity, within its derived bound); and a refresh-off
HOST TWIN the test re-initialises exactly when the refresh rule extended by rule 8 fires (the gate), on the committed clip
tests/golden/appearance_tiny.npz."""
import importlib.util
import os
import re

import numpy as np
import pytest

import appearance_util as au
from template_refresh_util import inside, tap_rect, tap_rect_geo
from test_gpu_planar_formats import _device, _frames_of, _oracle_frame
from test_gpu_stream_subsets import _res
from test_gpu_template_refresh import _dev, _tpl
from test_gpu_trajectories import _clip, _fixture

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 640, 480
INVALID, OOM = -1, -8
PREMISE = 0.1           # va >= 0.1 Saa, vp >= 0.1 Spp: asserted wherever a tolerance is used


@pytest.fixture(scope="module")
def mk():
    spec = importlib.util.spec_from_file_location("_make_appearance", os.path.join(HERE, "golden", "make_appearance.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bits(g, name, s=0):
    """a bf16 tensor of read_tensor (widened to float32) as its bf16 bit patterns [nt, kpad]"""
    mi = g.model_info()
    return (g.read_tensor(name, s).view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(mi.tokens_template, mi.kpad)


def _state(g, s=0):
    return g.read_tensor("state", s).view(np.uint32).copy()


def _cols(g):
    return 3 * g.model_info().patch ** 2


def _check_similarity(g, s=0):
    """the stream's record against the restatement on the rows the engine holds"""
    ap = g.appearance(s)
    a, p = _bits(g, "anchor", s), _bits(g, "probe", s)
    cols = _cols(g)
    want = au.score(a, p, cols)
    assert ap["status"] == want["status"], (ap, want)
    if want["status"] == 1:
        f = au.premise(a, p, cols)
        assert f >= PREMISE, f"premise: va, vp are only {f} of Saa, Spp"
        tol = au.sim_tolerance(a.shape[0] * cols, PREMISE, want["similarity"])
        assert abs(ap["similarity"] - float(want["similarity"])) <= tol, (ap, want)
    return ap


# ---- 1. the read-only twin ------------------------------------------------------------------------------------------------

def _enable_all(gpu, g, appearance, motion=True):
    g.set_template_refresh(2, 0.0)
    g.enable_chips(32, gpu.CHIP_RGB8)
    g.set_chips(2.0)
    if motion:
        g.set_motion_prior(True)
    if appearance:
        g.set_appearance(True, period=1, gate=0.0)


def _same(main, plain, rm, rp, tag):
    assert [_res(r) for r in rm] == [_res(r) for r in rp], tag
    for s in range(main.streams):
        assert np.array_equal(_state(main, s), _state(plain, s)), f"{tag}: stream {s}: state words"
        assert np.array_equal(_tpl(main, s), _tpl(plain, s)), f"{tag}: stream {s}: template"


def test_read_only_twin_on_device_passes(gpu, weights_tiny):
    """full, subset and candidate passes with refresh, chips and the motion prior beside the check: gate 0 changes nothing"""
    B = 3
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    main, plain = gpu.Group(weights_tiny, n_streams=B), gpu.Group(weights_tiny, n_streams=B)
    keep = [_dev(gpu, sc, 0) for sc in scs]
    for g in (main, plain):
        for s in range(B):
            g.init_device(s, keep[s][0], gpu.BBox.new(*scs[s].gt_box(0)))
    _enable_all(gpu, main, True)
    _enable_all(gpu, plain, False)
    for p, L in enumerate([None, None, [2, 0], None, [1], None]):
        pairs = [_dev(gpu, sc, p) for sc in scs]
        streams = L if L is not None else list(range(B))
        frames = [pairs[s][0] for s in streams]
        rm, rp = main.update_device(frames, streams=L), plain.update_device(frames, streams=L)
        _same(main, plain, rm, rp, f"pass {p} {L}")
        for i, s in enumerate(streams):
            assert _check_similarity(main, s)["status"] == (1 if rm[i].success else 0)
    box = main.read_state(1)["box"]
    cands = [(1, [4.0, 4.0, 40.0, 40.0]), (1, None), (1, [float(box[0]) + 5, float(box[1]) - 3, float(box[2]), float(box[3])])]
    pairs = [_dev(gpu, sc, 6) for sc in scs]
    (rm, wm), (rp, wp) = main.update_device_candidates(cands, [pairs[1][0]] * 3), plain.update_device_candidates(cands, [pairs[1][0]] * 3)
    assert wm == wp
    _same(main, plain, rm, rp, "candidate pass")
    pairs = [_dev(gpu, sc, 7) for sc in scs]
    frames = [p[0] for p in pairs]
    _same(main, plain, main.update_device(frames), plain.update_device(frames), "full pass after the candidate pass")
    assert sum(main.template_refresh_stats(s)["generation"] for s in range(B)) >= 3, "no refresh ran beside the check"
    assert main.motion(0)["on"] == 1 and main.appearance(0)["gated"] == 0
    main.close()
    plain.close()


def test_read_only_twin_on_host_passes(gpu, weights_tiny):
    """synchronous and pipelined host passes with refresh and chips beside the check. Margin -1 and no motion prior (it
    plans the speculative windows ahead of a steady target): the speculative windows are the exact ones of the old box,
    every third clip frame, as in the similarity test below, so passes are redone"""
    B, N = 2, 12
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s + 1) for s in range(B)]
    frames = [[sc.frame_rgb8(3 * i) for sc in scs] for i in range(N)]
    main, plain = (gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1) for _ in range(2))
    for g in (main, plain):
        for s in range(B):
            g.init_host(s, frames[0][s], gpu.BBox.new(*scs[s].gt_box(0)))
    _enable_all(gpu, main, True, motion=False)
    _enable_all(gpu, plain, False, motion=False)
    for i in range(3):
        _same(main, plain, main.update_host(frames[i]), plain.update_host(frames[i]), f"synchronous host pass {i}")
    for g in (main, plain):
        g.enqueue_host(frames[3])
    for i in range(4, N):
        for g in (main, plain):
            g.enqueue_host(frames[i])
        assert [_res(r) for r in main.wait_next()] == [_res(r) for r in plain.wait_next()], f"pipelined pass {i - 1}"
    _same(main, plain, main.wait_next(), plain.wait_next(), "the last pipelined pass")
    assert main.host_redos() > 0, "no pass was redone: the redo path was not exercised"
    main.close()
    plain.close()


# ---- 2. the probe's bits ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["rgb8", "nv12", "i420", "nv12_window"])
def test_probe_is_the_template_crop_at_the_new_box(gpu, oracle, weights_tiny, case):
    fmt = case.split("_")[0]
    window = (200, 150, 400, 330) if case.endswith("window") else None
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    ref = oracle.VitTrackRef(weights_tiny)

    def frame(t):
        if fmt == "i420":
            sib, sdata, data = _frames_of(gpu, fmt, sc, t, W, H)
        else:
            sib, sdata = fmt, (sc.frame_nv12(t) if fmt == "nv12" else sc.frame_rgb8(t))
            data = sdata
        f, keep = _device(gpu, fmt, data, W, H, **({"window": window} if window else {}))
        return f, keep, _oracle_frame(oracle, sib, sdata, W, H)

    main, twin = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    f0, k0, _ = frame(0)
    main.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    main.set_appearance(True)
    for t in range(1, 4):
        f, k, of = frame(t)
        r = main.update_device([f])[0]
        ap = _check_similarity(main)
        assert r.success and ap["status"] == 1 and ap["frames_done"] == t and ap["similarity"] > 0.9
        probe = _bits(main, "probe")
        twin.init_device(0, f, gpu.BBox.new(*r.bbox))
        assert np.array_equal(probe, _bits(twin, "template")), f"update {t}: probe != the rows init writes at the new box"
        assert np.array_equal(probe, ref._pre(of, np.float32(r.bbox), 2.0, ref.m.T)), f"update {t}: probe != the oracle's crop"
    main.close()
    twin.close()


def test_probe_bits_cfg5_patch14(gpu, oracle):
    """patch 14: the crop's 2-pixel stores and 52 pad columns per row (588 of 640), which stay as the enable left them"""
    weights = gpu.weights.ensure_weights("cfg5")
    sc = _clip(gpu, _fixture("traj_cfg5_300.npz"))
    main, twin = gpu.Group(weights, n_streams=1), gpu.Group(weights, n_streams=1)
    mi = main.model_info()
    assert mi.patch == 14 and mi.kpad > 3 * 14 * 14
    f0, k0 = _dev(gpu, sc, 0)
    main.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    main.set_appearance(True)
    f, k = _dev(gpu, sc, 1)
    r = main.update_device([f])[0]
    ap = _check_similarity(main)
    assert r.success and ap["status"] == 1
    twin.init_device(0, f, gpu.BBox.new(*r.bbox))
    probe = _bits(main, "probe")
    assert np.array_equal(probe, _bits(twin, "template"))
    assert not probe[:, 588:].any() and probe[:, :588].any()
    ref = oracle.VitTrackRef(weights)
    assert np.array_equal(probe, ref._pre(oracle.Frame.nv12(sc.frame_nv12(1), sc.w, sc.h), np.float32(r.bbox), 2.0, ref.m.T))
    main.close()
    twin.close()


# ---- 3. the anchor -----------------------------------------------------------------------------------------------------------

def test_anchor_follows_init_import_copy_and_the_action_only(gpu, weights_tiny):
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(2)]
    a, b = gpu.Group(weights_tiny, n_streams=2), gpu.Group(weights_tiny, n_streams=2)
    keep = [_dev(gpu, sc, 0) for sc in scs]
    for s in range(2):
        a.init_device(s, keep[s][0], gpu.BBox.new(*scs[s].gt_box(0)))
    a.set_appearance(True)                              # the enable behind the inits fills the anchors
    for s in range(2):
        assert np.array_equal(_bits(a, "anchor", s), _bits(a, "template", s)) and _bits(a, "anchor", s).any()
    assert not np.array_equal(_bits(a, "anchor", 0), _bits(a, "anchor", 1))
    f1, k1 = _dev(gpu, scs[0], 5)
    a.init_device(0, f1, gpu.BBox.new(*scs[0].gt_box(5)))     # init
    init_rows = _bits(a, "anchor", 0)
    assert np.array_equal(init_rows, _bits(a, "template", 0))
    a.set_template_refresh(2, 0.0)                      # a refresh never writes it
    for t in range(5, 9):
        pairs = [_dev(gpu, sc, t) for sc in scs]
        a.update_device([p[0] for p in pairs])
    assert a.template_refresh_stats(0)["generation"] >= 1
    assert np.array_equal(_bits(a, "anchor", 0), init_rows) and not np.array_equal(_bits(a, "template", 0), init_rows)
    other = _bits(a, "anchor", 1)
    a.set_anchor(0)                                     # the action: the current (refreshed) template
    assert np.array_equal(_bits(a, "anchor", 0), _bits(a, "template", 0)) and np.array_equal(_bits(a, "anchor", 1), other)
    a.set_anchor(-1)
    assert np.array_equal(_bits(a, "anchor", 1), _bits(a, "template", 1))
    assert a.appearance(0)["status"] == 0, "the action did not reset the stream's record"
    for bad in (-2, 2):
        with pytest.raises(gpu.VtError) as ei:
            a.set_anchor(bad)
        assert ei.value.code == INVALID
    # import and copy: the imported rows (the source's CURRENT template)
    b.set_appearance(True)
    b.import_stream(1, a.export_stream(0))
    assert np.array_equal(_bits(b, "anchor", 1), _bits(a, "template", 0)) and np.array_equal(_bits(b, "anchor", 1), _bits(b, "template", 1))
    a.copy_stream(1, b, 0)
    assert np.array_equal(_bits(b, "anchor", 0), _bits(a, "template", 1)) and np.array_equal(_bits(b, "anchor", 0), _bits(b, "template", 0))
    # a queued init, behind an outstanding pass of the other stream
    fr = [sc.frame_rgb8(9) for sc in scs]
    b.update_host(fr)
    b.enqueue_host([scs[0].frame_rgb8(10)], streams=[0])
    b.enqueue_init_host(1, scs[1].frame_rgb8(10), gpu.BBox.new(*scs[1].gt_box(10)))
    b.wait_next()
    plain = gpu.Group(weights_tiny, n_streams=1)
    plain.init_host(0, scs[1].frame_rgb8(10), gpu.BBox.new(*scs[1].gt_box(10)))
    assert np.array_equal(_bits(b, "anchor", 1), _bits(plain, "template", 0)) and np.array_equal(_bits(b, "anchor", 1), _bits(b, "template", 1))
    # a single tracker: the same keys through vt_tracker_as_group
    trk = gpu.VitTrack(weights_tiny)
    trk.init(scs[0].frame_rgb8(0), gpu.BBox.new(*scs[0].gt_box(0)))
    trk.set_appearance(True)
    trk.update(scs[0].frame_rgb8(1))
    assert trk.appearance()["status"] == 1 and trk.anchor().any()
    trk.import_state(trk.export_state())
    assert trk.appearance()["status"] == 0
    trk.close()
    for g in (a, b, plain):
        g.close()


# ---- 4. the similarity; pipelined == synchronous ------------------------------------------------------------------------------

def test_similarity_within_the_bound_and_pipelined_bits_equal_synchronous(gpu, weights_tiny):
    """B 2, margin -1: every speculative window is the exact one of the OLD box, so a moving target's pass is redone. The
    records, the probes, the states and the results of the pipelined run equal the synchronous run's bit for bit wherever
    the pipeline is drained (every second pass)."""
    B, N = 2, 12
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s + 1) for s in range(B)]
    frames = [[sc.frame_rgb8(3 * i) for sc in scs] for i in range(N)]

    def make():
        g = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1)
        for s in range(B):
            g.init_host(s, frames[0][s], gpu.BBox.new(*scs[s].gt_box(0)))
        g.set_appearance(True)
        return g

    def snap(g):
        return [(g.read_tensor("appearance", s)[:4].view(np.uint32).tolist(), _bits(g, "probe", s).tobytes(), _state(g, s).tobytes())
                for s in range(B)]

    sync, want, recs = make(), [], []
    for i in range(N):
        want.append([_res(r) for r in sync.update_host(frames[i])])
        for s in range(B):
            ap = _check_similarity(sync, s)
            assert ap["status"] == 1 and ap["frames_done"] == i + 1 and 0.8 < ap["similarity"] <= 1.0, (i, s, ap)
        recs.append(snap(sync))
    assert sync.appearance(0)["evaluated"] == N and sync.host_redos() == 0
    pipe = make()
    for i in range(0, N, 2):
        pipe.enqueue_host(frames[i])
        pipe.enqueue_host(frames[i + 1])            # speculative: its streams are in the pass still running
        assert [_res(r) for r in pipe.wait_next()] == want[i], f"frame {i}"
        assert [_res(r) for r in pipe.wait_next()] == want[i + 1], f"frame {i + 1}"
        assert snap(pipe) == recs[i + 1], f"frame {i + 1}: record, probe or state differ from the synchronous run"
    assert pipe.host_redos() > 0, "no pass was redone: the redo path was not exercised"
    assert pipe.appearance(0)["evaluated"] >= N
    sync.close()
    pipe.close()


# ---- 5. statuses ----------------------------------------------------------------------------------------------------------------

def test_status_2_where_the_template_crop_leaves_the_sampled_search_crop(gpu, weights_tiny):
    """the fast clip of the refresh tests' geometry skip (every 20th clip frame): refresh rule 6, restated"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=3)
    g = gpu.Group(weights_tiny, n_streams=1)
    f0, k0 = _dev(gpu, sc, 0, "rgb8")
    g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    g.set_appearance(True)
    mi = g.model_info()
    seen = {1: 0, 2: 0}
    for t in range(0, 16 * 20, 20):
        f, k = _dev(gpu, sc, t, "rgb8")
        r = g.update_device([f])[0]
        ap, st = g.appearance(0), g.read_state(0)
        if not r.success:
            assert ap["status"] == 0
            continue
        ok = inside(tap_rect(np.float32(r.bbox), 2.0, mi.template_size), tap_rect_geo(st["geo"], mi.search_size))
        assert ap["status"] == (1 if ok else 2), (t, ap, r.bbox)
        assert ap["similarity"] == 0.0 or ok
        seen[ap["status"]] += 1
    assert seen[2] >= 1 and seen[1] >= 1, seen
    assert g.appearance(0)["evaluated"] == seen[1]
    g.close()


def test_status_0_on_a_failed_update_and_off_period(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0, hide=(3, 6))
    g = gpu.Group(weights_tiny, n_streams=1)
    f0, k0 = _dev(gpu, sc, 0, "rgb8")
    g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    g.set_appearance(True, period=3)
    failed = 0
    for t in range(12):
        f, k = _dev(gpu, sc, t, "rgb8")
        r = g.update_device([f])[0]
        ap = g.appearance(0)
        assert ap["frames_done"] == t + 1 and ap["period"] == 3
        want = 1 if r.success and (t + 1) % 3 == 0 else 0
        assert ap["status"] == want and (want == 1 or ap["similarity"] == 0.0), (t, r, ap)
        failed += not r.success
    assert failed >= 1, "the occlusion failed no update"
    g.set_appearance(False)
    f, k = _dev(gpu, sc, 12, "rgb8")
    assert g.update_device([f])[0].success and g.appearance(0)["status"] == 0 and g.appearance(0)["on"] == 0
    g.close()


def test_switching_the_check_off_switches_its_gate_off(gpu, weights_tiny):
    """ "appearance" 0 with a gate left at 999 per mille: records are no longer written, and no refresh waits for one"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = gpu.Group(weights_tiny, n_streams=1)
    f0, k0 = _dev(gpu, sc, 0, "rgb8")
    g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    g.set_template_refresh(2, 0.0)
    g.set_appearance(True, gate=0.999)
    for t in range(1, 5):
        f, k = _dev(gpu, sc, t, "rgb8")
        assert g.update_device([f])[0].success
    on = g.appearance(0)
    assert on["status"] == 1 and on["similarity"] < 0.999, "the moving target scores above the gate: the test shows nothing"
    assert g.template_refresh_stats(0)["generation"] == 0 and on["gated"] == 3      # due at updates 2, 3 and 4
    g.set_appearance(False)
    for t in range(5, 9):
        f, k = _dev(gpu, sc, t, "rgb8")
        assert g.update_device([f])[0].success
    off = g.appearance(0)
    assert g.template_refresh_stats(0)["generation"] == 2, "the gate of a check that is off held the refresh back"
    assert off["gated"] == on["gated"] and off["status"] == 0 and off["on"] == 0
    g.close()


def test_candidate_pass_evaluates_the_winning_slot_only(gpu, weights_tiny):
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(3)]
    g, twin = gpu.Group(weights_tiny, n_streams=3), gpu.Group(weights_tiny, n_streams=1)
    keep = [_dev(gpu, sc, 0) for sc in scs]
    for s in range(3):
        g.init_device(s, keep[s][0], gpu.BBox.new(*scs[s].gt_box(0)))
    g.set_appearance(True)
    g.update_device([k[0] for k in keep])
    before = [g.appearance(s) for s in range(3)]
    box = g.read_state(2)["box"]
    cands = [(2, [4.0, 4.0, 40.0, 40.0]), (2, None), (2, [float(box[0]) + 6, float(box[1]) - 4, float(box[2]), float(box[3])])]
    f, k = _dev(gpu, scs[2], 1)
    res, win = g.update_device_candidates(cands, [f] * 3)
    assert win[0] in (1, 2) and res[win[0]].success
    ap = _check_similarity(g, 2)
    assert ap["status"] == 1 and ap["evaluated"] == before[2]["evaluated"] + 1 and ap["frames_done"] == 2
    twin.init_device(0, f, gpu.BBox.new(*res[win[0]].bbox))
    assert np.array_equal(_bits(g, "probe", 2), _bits(twin, "template")), "the probe is not the crop at the committed slot's box"
    for s in (0, 1):
        assert g.appearance(s) == before[s], "a stream that was not in the pass got a new record"
    g.close()
    twin.close()


# ---- 6. the gate ------------------------------------------------------------------------------------------------------------------

def test_gate_equals_a_host_twin_under_the_extended_rule(gpu, weights_tiny, mk, capsys):
    fx = dict(np.load(os.path.join(HERE, "golden", "appearance_tiny.npz")))
    box0, frames = mk.gate_clip()
    tau = float(fx["gate_pm"]) / 1000.0
    main, twin = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    mi = main.model_info()
    rule = au.Rule(mi.template_size, mi.search_size, int(fx["period"]), 0.0, int(fx["gate_pm"]))
    cols = _cols(main)

    def dev(i):
        import torch
        d = torch.from_numpy(np.ascontiguousarray(frames[i])).cuda()
        return gpu.frame_rgb8(d.data_ptr(), frames[i].shape[1], frames[i].shape[0]), d

    f0, k0 = dev(0)
    for g in (main, twin):
        g.init_device(0, f0, gpu.BBox.new(*box0))
    main.set_template_refresh(int(fx["period"]), 0.0)
    main.set_appearance(True, period=1, gate=tau)
    assert main.appearance(0)["gate_pm"] == int(fx["gate_pm"])
    acts, sims, imp_ok = [], [], []
    for i in range(1, int(fx["n_updates"]) + 1):
        f, k = dev(i)
        rm, rt = main.update_device([f])[0], twin.update_device([f])[0]
        assert _res(rm) == _res(rt), f"update {i}: {rm} vs twin {rt}"
        ap = _check_similarity(main)
        assert ap["status"] == 1 and ap["frames_done"] == i
        sim = float(au.score(_bits(main, "anchor"), _bits(main, "probe"), cols)["similarity"])      # the restatement decides for the twin
        assert abs(sim - tau) > 0.01, f"update {i}: similarity {sim} within 0.01 of tau"
        st = twin.read_state(0)
        act = rule.step(rt, geo=st["geo"], window_miss=st["window_miss"] == st["frames_done"], record=(1, sim))
        if act == "fire":
            twin.init_device(0, f, gpu.BBox.new(*rt.bbox))
        acts.append(act)
        sims.append(sim)
        if mk.impostor_at(i):
            imp_ok.append(bool(rm.success))
        got = main.template_refresh_stats(0)
        assert (got["generation"], got["last_frame"]) == (rule.generation, rule.last_frame), f"update {i}: {got} vs {act}"
        assert np.array_equal(_tpl(main), _tpl(twin)), f"update {i}: template rows differ"
    with capsys.disabled():
        print(f"\n[appearance gate] fired {len(rule.fired)}, gated {len(rule.gated)}, similarities {min(sims):.3f} .. {max(sims):.3f}")
    assert len(rule.fired) >= 3 and len(rule.gated) >= 3, (rule.fired, rule.gated)
    assert all(imp_ok) and len(imp_ok) == 18, "the tracker fails on an impostor frame"
    assert all(not mk.impostor_at(i) for i in rule.fired) and all(mk.impostor_at(i) for i in rule.gated)
    assert main.appearance(0)["gated"] == len(rule.gated)
    assert [{None: 0, "fire": 1, "gate": 2, "skip": 3}[a] for a in acts] == list(fx["gate_action"]), "the oracle's run decided otherwise"
    main.close()
    twin.close()


# ---- 7. keys ------------------------------------------------------------------------------------------------------------------------

def test_keys_ranges_memory_and_refusal(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = gpu.Group(weights_tiny, n_streams=2)
    f0, k0 = _dev(gpu, sc, 0)
    for s in range(2):
        g.init_device(s, f0, gpu.BBox.new(*sc.gt_box(0)))
    for name in ("appearance", "anchor", "probe"):      # never enabled: no such tensor
        with pytest.raises(gpu.VtError) as ei:
            g.read_tensor(name, 0)
        assert ei.value.code == INVALID
    with pytest.raises(gpu.VtError) as ei:
        g.set_tuning("appearance_anchor", 0)
    assert ei.value.code == INVALID
    caps = g.graph_captures()
    g.set_tuning("appearance_period", 5)                # remembered until the enable
    g.set_tuning("appearance_gate_pm", 250)
    g.set_tuning("appearance", 0)
    assert g.graph_captures() == caps
    for key, bad in (("appearance", 2), ("appearance_period", 0), ("appearance_period", 1000001), ("appearance_gate_pm", 1001),
                     ("appearance_nope", 1)):
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning(key, bad)
        assert ei.value.code == INVALID, (key, bad)
    assert g.graph_captures() == caps
    g.set_tuning("appearance", 1)
    caps_on = g.graph_captures()
    assert caps_on > caps
    ap = g.appearance(1)
    assert (ap["on"], ap["period"], ap["gate_pm"], ap["status"], ap["evaluated"], ap["gated"]) == (1, 5, 250, 0, 0, 0)
    for key, bad in (("appearance", 2), ("appearance_period", 0), ("appearance_gate_pm", 1001), ("appearance_anchor", -2),
                     ("appearance_anchor", 2)):
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning(key, bad)
        assert ei.value.code == INVALID, (key, bad)
        assert g.appearance(1) == ap
    g.set_tuning("appearance_period", -1)               # negative: the default
    g.set_tuning("appearance_gate_pm", -1)
    ap = g.appearance(0)
    assert (ap["period"], ap["gate_pm"]) == (1, 0) and g.graph_captures() == caps_on
    g.set_tuning("appearance_period", 1000000)
    g.set_tuning("appearance_gate_pm", 1000)
    assert (g.appearance(0)["period"], g.appearance(0)["gate_pm"]) == (1000000, 1000)
    # refused while a pipelined pass is outstanding
    h = gpu.Group(weights_tiny, n_streams=1)
    fr = sc.frame_rgb8(0)
    h.init_host(0, fr, gpu.BBox.new(*sc.gt_box(0)))
    h.set_tuning("appearance", 1)                       # enabled: each call below is valid but for the outstanding pass
    h.set_tuning("appearance_anchor", 0)
    h.enqueue_host([fr])
    for key, value in (("appearance", 0), ("appearance_period", 2), ("appearance_gate_pm", 500), ("appearance_anchor", 0)):
        with pytest.raises(gpu.VtError) as ei:
            h.set_tuning(key, value)
        assert ei.value.code == INVALID, key
    assert h.wait_next()[0].success
    ap = h.appearance(0)
    assert (ap["on"], ap["period"], ap["gate_pm"], ap["status"]) == (1, 1, 0, 1), "a refused key changed the policy"
    for key, value in (("appearance_period", 2), ("appearance_gate_pm", 500), ("appearance_anchor", 0), ("appearance", 0)):
        h.set_tuning(key, value)
    g.close()
    h.close()


def test_enable_under_a_memory_cap_is_refused_and_nothing_changes(gpu, weights_tiny):
    """64 tiny streams: anchors and probes are 64 x 2 x 24 KiB = 3 MiB. Under the smallest max_device_mib that still creates
    the engine less than 1 MiB is left: the enable must return VT_ERR_OOM and change nothing."""
    B = 64

    def create(mib):
        try:
            return gpu.Group(weights_tiny, n_streams=B, max_device_mib=mib, use_graph=False)
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
    g = create(hi)
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    f0, k0 = _dev(gpu, sc, 0)
    for s in range(B):
        g.init_device(s, f0, gpu.BBox.new(*sc.gt_box(0)))
    g.set_tuning("appearance_period", 7)
    with pytest.raises(gpu.VtError) as ei:
        g.set_tuning("appearance", 1)
    assert ei.value.code == OOM
    with pytest.raises(gpu.VtError) as ei:
        g.read_tensor("appearance", 5)
    assert ei.value.code == INVALID, "the refused enable left the engine capable"
    f1, k1 = _dev(gpu, sc, 1)
    assert all(r.success for r in g.update_device([f1] * B))
    g.close()
    roomy = gpu.Group(weights_tiny, n_streams=B, max_device_mib=hi + 4, use_graph=False)
    roomy.set_tuning("appearance_period", 7)
    roomy.set_tuning("appearance", 1)
    assert roomy.appearance(63)["period"] == 7
    roomy.close()


# ---- 8. exports and launches -------------------------------------------------------------------------------------------------------

def test_no_new_export(gpu):
    assert len(gpu.EXPORTS) == 91 and "vt_op_appearance_score" in gpu.OPS_EXPORTS
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(HERE, "..", "include", "vittrack_hip.h")).read(), flags=re.S)
    assert len(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", txt))) == 91


def test_two_launches_per_pass_on_enabled_engines_only(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = gpu.Group(weights_tiny, n_streams=2)
    f0, k0 = _dev(gpu, sc, 0)
    for s in range(2):
        g.init_device(s, f0, gpu.BBox.new(*sc.gt_box(0)))
    plain = g.profile_device([f0, f0], iters=2)
    assert not [k for k in plain if k["name"].startswith("appearance")]
    g.set_appearance(True)
    fams = {k["name"]: k["launches"] for k in g.profile_device([f0, f0], iters=2)}
    assert {n: c for n, c in fams.items() if n.startswith("appearance")} == {"appearance_probe": 1, "appearance_score": 1}
    assert sum(fams.values()) == sum(k["launches"] for k in plain) + 2
    order = [k["name"] for k in g.profile_device([f0, f0], iters=1)]
    assert order.index("appearance_score") == order.index("appearance_probe") + 1
    g.close()
