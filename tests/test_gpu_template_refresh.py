"""Device-side template refresh (vt_group_set_template_refresh; DESIGN.md section 3, "Template refresh"), on the MI355X.

The yardstick of the bit-exact tests is a HOST TWIN: a second engine that never enables refresh. After each update the
test applies the restated rule (tests/template_refresh_util.py) to the twin's own state and result and calls
init_device(stream, whole frame, result.bbox) when it fires. "Equal" means: success, score and bbox bit-identical on
every frame, the "template" tensor bit-identical after every update, generation == the twin's re-init count.
tests/test_template_refresh_abi.py pins, on the oracle, that the clips used here fire, skip and fail where needed."""
import numpy as np
import pytest

from conftest import iou
from template_refresh_util import OracleTracker, Rule, clip_frames, drive, tap_rect
from test_gpu_stream_subsets import _res
from test_gpu_trajectories import _clip, _fixture

pytestmark = pytest.mark.gpu

W, H = 640, 480
INVALID, OOM = -1, -8


def _dev(gpu, sc, t, fmt="nv12"):
    """(device frame of clip time t in the given format, keep-alive tensor)"""
    import torch
    w, h = sc.w, sc.h
    if fmt == "nv12":
        d = torch.from_numpy(sc.frame_nv12(t)).cuda()
        return gpu.frame_nv12(d.data_ptr(), d.data_ptr() + w * h, w, h), d
    rgb = sc.frame_rgb8(t)
    if fmt == "rgb8":
        d = torch.from_numpy(np.ascontiguousarray(rgb)).cuda()
        return gpu.frame_rgb8(d.data_ptr(), w, h), d
    assert fmt == "bgrx"
    a = np.full((h, w, 4), 255, np.uint8)
    a[..., 0], a[..., 1], a[..., 2] = rgb[..., 2], rgb[..., 1], rgb[..., 0]
    d = torch.from_numpy(a).cuda()
    return gpu.frame_bgrx(d.data_ptr(), w, h), d


def _tpl(g, s=0):
    return g.read_tensor("template", s).view(np.uint32).copy()


class Twin:
    """a group with refresh off + one Rule per stream: after_pass() re-initialises the streams whose rule fires"""

    def __init__(self, gpu, weights, B, period, min_score=0.0, **kw):
        self.gpu, self.g = gpu, gpu.Group(weights, n_streams=B, **kw)
        mi = self.g.model_info()
        self.rules = [Rule(mi.template_size, mi.search_size, period, min_score) for _ in range(B)]

    def after_pass(self, streams, frames, results, winners=None):
        """streams[i] / frames[i] / results[i]: slot i's stream, whole frame and result; winners: of a candidate pass"""
        acts = {}
        for i, s in enumerate(streams):
            if winners is not None and winners[i] != i:
                continue                                    # one step per stream: at its committed slot
            st = self.g.read_state(s)
            act = self.rules[s].step(results[i], geo=st["geo"], window_miss=st["window_miss"] == st["frames_done"])
            if act == "fire":
                self.g.init_device(s, frames[i], self.gpu.BBox.new(*results[i].bbox))
            acts[s] = act
        return acts

    def close(self):
        self.g.close()


def _assert_equal(main, twin, res_m, res_t, tag):
    assert len(res_m) == len(res_t)
    for i, (a, b) in enumerate(zip(res_m, res_t)):
        assert _res(a) == _res(b), f"{tag}: slot {i}: {a} vs twin {b}"
    for s, rule in enumerate(twin.rules):
        st = main.template_refresh_stats(s)
        assert st["generation"] == rule.generation, f"{tag}: stream {s}: generation {st['generation']}, twin re-inits {rule.generation}"
        assert st["last_frame"] == rule.last_frame, f"{tag}: stream {s}: last_frame"
        assert np.array_equal(_tpl(main, s), _tpl(twin.g, s)), f"{tag}: stream {s}: template rows differ"


def _pair(gpu, weights, scs, fmts, period, min_score=0.0, t0=0, **kw):
    """(main group with the policy on every stream, twin), both initialised on clip time t0"""
    B = len(scs)
    main, twin = gpu.Group(weights, n_streams=B, **kw), Twin(gpu, weights, B, period, min_score, **kw)
    keep = []
    for s, (sc, fmt) in enumerate(zip(scs, fmts)):
        f, k = _dev(gpu, sc, t0, fmt)
        keep.append(k)
        for g in (main, twin.g):
            g.init_device(s, f, gpu.BBox.new(*sc.gt_box(t0)))
    main.set_template_refresh(period, min_score)
    return main, twin


def _run_full(gpu, weights, scs, fmts, ts, period, min_score=0.0, twin_on=True, **kw):
    """full passes at clip times ts against the twin -> per update (result bits per stream, template words per stream)"""
    B = len(scs)
    if twin_on:
        main, twin = _pair(gpu, weights, scs, fmts, period, min_score, t0=ts[0], **kw)
    else:
        main, twin = gpu.Group(weights, n_streams=B, **kw), None
        for s in range(B):
            f, k = _dev(gpu, scs[s], ts[0], fmts[s])
            main.init_device(s, f, gpu.BBox.new(*scs[s].gt_box(ts[0])))
        main.set_template_refresh(period, min_score)
    caps = main.graph_captures()
    rec = []
    for i, t in enumerate(ts):
        pairs = [_dev(gpu, scs[s], t, fmts[s]) for s in range(B)]
        frames = [p[0] for p in pairs]
        rm = main.update_device(frames)
        if twin:
            rt = twin.g.update_device(frames)
            twin.after_pass(list(range(B)), frames, rt)
            _assert_equal(main, twin, rm, rt, f"update {i + 1}")
        rec.append(([_res(r) for r in rm], [_tpl(main, s) for s in range(B)]))
    assert main.graph_captures() == caps, "a graph was captured after the enable"
    stats = [main.template_refresh_stats(s) for s in range(B)]
    rules = twin.rules if twin else None
    main.close()
    if twin:
        twin.close()
    return rec, stats, rules


# ---- 1. full passes ------------------------------------------------------------------------------------------------------

def test_full_passes_equal_the_twin_in_three_formats(gpu, weights_tiny):
    """B 3, NV12 / RGB8 / BGRX (a pass with BGRX runs the crop kernels that read any layout; every other test here runs
    the RGB8 / NV12 ones), clip (a)'s motion, 24 updates, period 4"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    scs, fmts, ts = [sc] * 3, ["nv12", "rgb8", "bgrx"], list(range(24))
    rec, stats, rules = _run_full(gpu, weights_tiny, scs, fmts, ts, 4)
    for s in range(3):
        assert stats[s]["generation"] >= 5 and stats[s]["period"] == 4 and stats[s]["min_score"] == 0.0
        first = rules[s].fired[0]
        assert not np.array_equal(rec[first - 1][1][s], rec[first - 2][1][s]), "the first refresh left the init template"
    # eager launches give the same bits as the captured graphs
    rec0, stats0, _ = _run_full(gpu, weights_tiny, scs, fmts, ts, 4, twin_on=False, use_graph=False)
    for i, (a, b) in enumerate(zip(rec, rec0)):
        assert a[0] == b[0], f"update {i + 1}: use_graph=0 results differ"
        assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])), f"update {i + 1}: use_graph=0 template differs"
    assert [s["generation"] for s in stats0] == [s["generation"] for s in stats]


# ---- 2. the gate: scores and occlusion -----------------------------------------------------------------------------------

def test_min_score_one_never_refreshes_and_changes_nothing(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    on, off = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    f0, k0 = _dev(gpu, sc, 0, "rgb8")
    for g in (on, off):
        g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    on.set_template_refresh(2, 1.0)
    for t in range(8):
        f, k = _dev(gpu, sc, t, "rgb8")
        a, b = on.update_device([f]), off.update_device([f])
        assert _res(a[0]) == _res(b[0]) and a[0].success
        assert np.array_equal(_tpl(on), _tpl(off))
    st = on.template_refresh_stats(0)
    assert st["generation"] == 0 and st["last_frame"] == 0 and st["period"] == 2 and st["min_score"] == 1.0
    assert off.template_refresh_stats(0)["period"] == 0
    on.close()
    off.close()


def test_no_refresh_while_the_target_is_hidden(gpu, weights_tiny):
    """clip (c): updates 11-16 fail; no refresh there, the first due success refreshes again"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0, hide=(10, 16))
    main, twin = _pair(gpu, weights_tiny, [sc], ["rgb8"], 4)
    gens, ok = [], []
    for t in range(30):
        f, k = _dev(gpu, sc, t, "rgb8")
        rm, rt = main.update_device([f]), twin.g.update_device([f])
        twin.after_pass([0], [f], rt)
        _assert_equal(main, twin, rm, rt, f"update {t + 1}")
        gens.append(main.template_refresh_stats(0)["generation"])
        ok.append(rm[0].success)
    failed = [i for i, s in enumerate(ok) if not s]
    assert failed, "the occlusion failed no update: the test shows nothing"
    for i in failed:
        assert gens[i] == gens[i - 1], f"update {i + 1} failed and refreshed"
    after = failed[-1] + 1
    assert ok[after] and gens[after] == gens[after - 1] + 1, "the first due success after the occlusion did not refresh"
    assert gens[-1] >= 5
    main.close()
    twin.close()


# ---- 3. geometry ---------------------------------------------------------------------------------------------------------

def test_geometry_skip_equals_the_twin(gpu, weights_tiny):
    """clip (b): a fast target (every 20th clip frame): some due refreshes fail rule 6 and wait for the next update"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=3)
    ts = list(range(0, 16 * 20, 20))
    rec, stats, rules = _run_full(gpu, weights_tiny, [sc], ["rgb8"], ts, 2)
    assert stats[0]["skipped_geometry"] >= 1 and stats[0]["generation"] >= 1
    assert stats[0]["skipped_geometry"] == len(rules[0].skipped), (stats[0], rules[0].skipped)


def test_template_over_the_frame_edge_refreshes_with_black_taps(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=5, center=(40.0, 240.0), amp=3.0)
    main, twin = _pair(gpu, weights_tiny, [sc], ["nv12"], 2)
    for t in range(4):
        f, k = _dev(gpu, sc, t, "nv12")
        rm, rt = main.update_device([f]), twin.g.update_device([f])
        twin.after_pass([0], [f], rt)
        _assert_equal(main, twin, rm, rt, f"update {t + 1}")
        assert tap_rect(np.float32(rm[0].bbox), 2.0, twin.rules[0].T)[0] < 0, "the template crop does not leave the frame"
    assert main.template_refresh_stats(0)["generation"] == 2
    main.close()
    twin.close()


# ---- 4. subset and candidate passes --------------------------------------------------------------------------------------

def test_subset_passes_refresh_in_a_slot_that_is_not_the_stream(gpu, weights_tiny):
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(4)]
    main, twin = _pair(gpu, weights_tiny, scs, ["nv12"] * 4, 2)
    moved = 0
    for p, L in enumerate([None, [3, 1], None, [2], [0, 3, 1], None, [1, 0]]):
        pairs = [_dev(gpu, sc, p) for sc in scs]
        streams = L if L is not None else list(range(4))
        frames = [pairs[s][0] for s in streams]
        rm, rt = main.update_device(frames, streams=L), twin.g.update_device(frames, streams=L)
        acts = twin.after_pass(streams, frames, rt)
        _assert_equal(main, twin, rm, rt, f"pass {p} {L}")
        moved += sum(1 for i, s in enumerate(streams) if L is not None and i != s and acts.get(s) == "fire")
    assert moved >= 2, "no refresh fired in a slot other than the stream's own index"
    main.close()
    twin.close()


def test_candidate_pass_refreshes_the_winner_only(gpu, weights_tiny):
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(4)]
    main, twin = _pair(gpu, weights_tiny, scs, ["nv12"] * 4, 2)
    pairs = [_dev(gpu, sc, 0) for sc in scs]
    frames = [p[0] for p in pairs]
    rm, rt = main.update_device(frames), twin.g.update_device(frames)
    twin.after_pass([0, 1, 2, 3], frames, rt)
    _assert_equal(main, twin, rm, rt, "full pass")
    # three slots for stream 2: a corner of the frame, the stream's own box, a slightly shifted one
    box = main.read_state(2)["box"]
    cands = [(2, [4.0, 4.0, 40.0, 40.0]), (2, None), (2, [float(box[0]) + 6, float(box[1]) - 4, float(box[2]), float(box[3])])]
    pairs = [_dev(gpu, sc, 1) for sc in scs]
    slot_frames = [pairs[2][0]] * 3
    before = [_tpl(main, s) for s in range(4)]
    (rm, wm), (rt, wt) = main.update_device_candidates(cands, slot_frames), twin.g.update_device_candidates(cands, slot_frames)
    assert wm == wt and wm[0] in (1, 2) and rm[wm[0]].success
    acts = twin.after_pass([2, 2, 2], slot_frames, rt, winners=wt)
    assert acts == {2: "fire"}
    _assert_equal(main, twin, rm, rt, "candidate pass")
    assert main.template_refresh_stats(2)["generation"] == 1, "exactly one refresh: the committed slot's"
    assert tuple(main.read_state(2)["box"]) == tuple(float(v) for v in rm[wm[0]].bbox)
    for s in (0, 1, 3):
        assert np.array_equal(_tpl(main, s), before[s]) and main.template_refresh_stats(s)["generation"] == 0
    assert not np.array_equal(_tpl(main, 2), before[2])
    pairs = [_dev(gpu, sc, 2) for sc in scs]
    frames = [p[0] for p in pairs]
    rm, rt = main.update_device(frames), twin.g.update_device(frames)
    twin.after_pass([0, 1, 2, 3], frames, rt)
    _assert_equal(main, twin, rm, rt, "full pass after the candidate pass")
    main.close()
    twin.close()


# ---- 5. pipelined host ingest ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("margin_pct", [0, -1])
def test_pipelined_equals_synchronous(gpu, weights_tiny, margin_pct):
    """B 3, 24 frames, period 2: enqueue_host / wait_next against update_host. With margin -1 the speculative windows are
    the exact ones of the old box: passes are redone, and as a refresh fires in every second update of every stream,
    every rewound span (two passes) holds one - the rewound tpl_gen must find the old template in the other buffer."""
    B, N = 3, 24
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    frames = [[sc.frame_rgb8(2 * i) for sc in scs] for i in range(N)]

    def make():
        g = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=margin_pct)
        for s in range(B):
            g.init_host(s, frames[0][s], gpu.BBox.new(*scs[s].gt_box(0)))
        g.set_template_refresh(2, 0.0)
        return g

    sync = make()
    want, gens = [], []
    for i in range(N):
        want.append([_res(r) for r in sync.update_host(frames[i])])
        gens.append([sync.template_refresh_stats(s)["generation"] for s in range(B)])
    for i in range(2, N):
        for s in range(B):
            assert gens[i][s] - gens[i - 2][s] >= 1, f"stream {s}: no refresh in updates {i}, {i + 1}"
    pipe = make()
    pipe.enqueue_host(frames[0])
    with pytest.raises(gpu.VtError) as ei:
        pipe.set_template_refresh(3, 0.0)
    assert ei.value.code == INVALID
    for i in range(1, N):
        pipe.enqueue_host(frames[i])
        got = [_res(r) for r in pipe.wait_next()]
        assert got == want[i - 1], f"frame {i - 1}: pipelined {got} vs synchronous {want[i - 1]}"
    assert [_res(r) for r in pipe.wait_next()] == want[N - 1]
    for s in range(B):
        a, b = pipe.template_refresh_stats(s), sync.template_refresh_stats(s)
        assert (a["generation"], a["last_frame"], a["period"]) == (b["generation"], b["last_frame"], 2), f"stream {s}"
        assert np.array_equal(_tpl(pipe, s), _tpl(sync, s)), f"stream {s}: template"
        assert np.array_equal(pipe.read_tensor("state", s).view(np.uint32), sync.read_tensor("state", s).view(np.uint32))
    if margin_pct < 0:
        assert pipe.host_redos() > 0, "no pass was redone: the rollback was not exercised"
    assert sync.host_redos() == 0
    sync.close()
    pipe.close()


def test_pipelined_equals_synchronous_at_the_frame_edge(gpu, weights_tiny, capsys):
    """A large target (3 source pixels per search-crop pixel) that moves along the left frame edge, margin -1: the search
    rectangle hangs over the edge, where a speculative window can end inside it without a miss (rule 7 then reports the
    pass as a miss and the redo refreshes). Whatever the windows were: results, template and refresh state equal the
    synchronous run's."""
    N = 16
    sc = gpu.synth.MovingSquare(W, H, 96, seed=7, center=(70.0, 240.0), amp=22.0)
    frames = [[sc.frame_rgb8(3 * i)] for i in range(N)]

    def make():
        g = gpu.Group(weights_tiny, n_streams=1, host_window_margin_pct=-1)
        g.init_host(0, frames[0][0], gpu.BBox.new(*sc.gt_box(0)))
        g.set_template_refresh(2, 0.0)
        return g

    sync = make()
    want = [_res(sync.update_host(frames[i])[0]) for i in range(N)]
    pipe = make()
    pipe.enqueue_host(frames[0])
    for i in range(1, N):
        pipe.enqueue_host(frames[i])
        assert _res(pipe.wait_next()[0]) == want[i - 1], f"frame {i - 1}"
    assert _res(pipe.wait_next()[0]) == want[N - 1]
    a, b = pipe.template_refresh_stats(0), sync.template_refresh_stats(0)
    with capsys.disabled():
        print(f"\n[refresh at the edge] generation {b['generation']}, redos {pipe.host_redos()}, box {sync.read_state(0)['box']}")
    assert (a["generation"], a["last_frame"]) == (b["generation"], b["last_frame"])
    assert np.array_equal(_tpl(pipe), _tpl(sync))
    assert np.array_equal(pipe.read_tensor("state", 0).view(np.uint32), sync.read_tensor("state", 0).view(np.uint32))
    assert b["generation"] >= 1, "no refresh fired: the test shows nothing"
    sync.close()
    pipe.close()


# ---- 6. crop tiers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tier", [0, 1, 2, 3])
def test_every_crop_tier_writes_the_rows_of_init(gpu, weights_tiny, tier):
    """a 64-px target at template size 64 is 2 source pixels per output pixel: the tile of tiers 0 and 1 does not fit its
    buffer (the tile body's per-pixel path), tiers 2 and 3 (= 2) stage it in LDS"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    main, twin = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    f0, k0 = _dev(gpu, sc, 0, "rgb8")
    for g in (main, twin):
        g.set_tuning("crop_tier", tier)
        g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    main.set_template_refresh(2, 0.0)
    for t in range(2):
        f, k = _dev(gpu, sc, t, "rgb8")
        r = main.update_device([f])[0]
    assert main.template_refresh_stats(0)["generation"] == 1, "the refresh did not fire"
    twin.init_device(0, f, gpu.BBox.new(*r.bbox))
    assert np.array_equal(_tpl(main), _tpl(twin))
    assert _tpl(main).any()
    main.close()
    twin.close()


# ---- 7. ticket width: eight template tiles per slot -------------------------------------------------------------------------

def test_eight_tiles_per_slot_cfg2(gpu, weights_cfg2):
    sc = _clip(gpu, _fixture("traj_cfg2_300.npz"))
    rec, stats, rules = _run_full(gpu, weights_cfg2, [sc] * 4, ["nv12"] * 4, list(range(8)), 2)
    assert all(st["generation"] >= 3 for st in stats), stats


# ---- 8. the wide-store path (patch 14) ---------------------------------------------------------------------------------------

def test_wide_path_cfg5_writes_the_rows_of_init(gpu):
    weights = gpu.weights.ensure_weights("cfg5")
    sc = _clip(gpu, _fixture("traj_cfg5_300.npz"))
    main, twin = gpu.Group(weights, n_streams=1), gpu.Group(weights, n_streams=1)
    assert main.model_info().patch == 14
    f0, k0 = _dev(gpu, sc, 0)
    for g in (main, twin):
        g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    main.set_template_refresh(2, 0.0)
    for t in range(3):
        f, k = _dev(gpu, sc, t)
        r = main.update_device([f])[0]
        if t == 1:
            assert main.template_refresh_stats(0)["generation"] == 1, "the refresh did not fire"
            twin.init_device(0, f, gpu.BBox.new(*r.bbox))
            assert np.array_equal(_tpl(main), _tpl(twin))
    st = main.template_refresh_stats(0)
    assert st["generation"] == 1 and st["last_frame"] == 2
    main.close()
    twin.close()


# ---- 9. single tracker ---------------------------------------------------------------------------------------------------------

def test_single_tracker_equals_a_twin_tracker(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    main, twin = gpu.VitTrack(weights_tiny), gpu.VitTrack(weights_tiny)
    mi = main.model_info()
    rule = Rule(mi.template_size, mi.search_size, 2, 0.0)
    for trk in (main, twin):
        trk.init(sc.frame_rgb8(0), gpu.BBox.new(*sc.gt_box(0)))
    main.set_template_refresh(2, 0.0)
    tg = twin.as_group()
    for t in range(12):
        fr = sc.frame_rgb8(t)
        a, b = main.update(fr), twin.update(fr)
        assert _res(a) == _res(b), f"update {t + 1}: {a} vs {b}"
        st = tg.read_state(0)
        if rule.step(b, geo=st["geo"], window_miss=st["window_miss"] == st["frames_done"]) == "fire":
            twin.init(fr, gpu.BBox.new(*b.bbox))
        got = main.template_refresh_stats()
        assert (got["generation"], got["last_frame"]) == (rule.generation, rule.last_frame), f"update {t + 1}"
        assert np.array_equal(_tpl(main.as_group()), _tpl(tg)), f"update {t + 1}: template"
    assert rule.generation == 6
    main.close()
    twin.close()


# ---- 10. against the oracle -------------------------------------------------------------------------------------------------------

def test_device_policy_against_the_oracle_under_the_rule(gpu, oracle, weights_tiny, capsys):
    """clip (a), 60 updates, period 5: the closed-loop bars of tests/test_gpu_pipeline.py::_assert_parity, restated"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    ts, frames = clip_frames(sc, 60)
    ref = OracleTracker(weights_tiny)
    rule = Rule(ref.ref.m.T, ref.ref.m.S, 5, 0.0)
    want = drive(ref, frames, sc.gt_box(0), rule)
    trk = gpu.VitTrack(weights_tiny)
    trk.init(frames[0], gpu.BBox.new(*sc.gt_box(0)))
    trk.set_template_refresh(5, 0.0)
    got = [trk.update(fr) for fr in frames]
    st = trk.template_refresh_stats()
    trk.close()
    d = np.abs(np.array([r.bbox for r in got]) - np.array([r.bbox for r in want]))
    ious = [iou(a.bbox, b.bbox) for a, b in zip(got, want)]
    gt_iou = [iou(r.bbox, sc.gt_box(t)) for r, t in zip(want, ts)]
    dscore = max(abs(a.score - b.score) for a, b in zip(got, want))
    with capsys.disabled():
        print(f"\n[refresh vs oracle] max |delta| {d.max()} px, mean IoU {np.mean(ious):.4f}, max |dscore| {dscore:.4f}, "
              f"oracle min IoU vs GT {min(gt_iou):.3f}, generation {st['generation']} (oracle {rule.generation})")
    assert d.max() <= 1, f"max |delta| = {d.max()} px at frame {int(d.max(axis=1).argmax())}"
    assert np.mean(ious) >= 0.99, f"mean IoU(hip, oracle) = {np.mean(ious):.4f}"
    assert all(bool(a.success) == bool(b.success) for a, b in zip(got, want)), "success flags differ"
    assert dscore < 0.03
    assert min(gt_iou) > 0.5, f"oracle lost the target: min IoU vs GT {min(gt_iou):.3f}"
    # the device gate fired where the restated rule did: every fifth update, the last one at update 60
    assert rule.fired == list(range(5, 61, 5))
    assert (st["generation"], st["last_frame"], st["skipped_geometry"]) == (rule.generation, rule.last_frame, 0)


# ---- 11. argument errors and the memory cap ----------------------------------------------------------------------------------------

def test_bad_arguments_change_nothing(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = gpu.Group(weights_tiny, n_streams=2)
    f0, k0 = _dev(gpu, sc, 0)
    for s in range(2):
        g.init_device(s, f0, gpu.BBox.new(*sc.gt_box(0)))
    g.set_template_refresh(3, 0.25, stream=1)
    caps = g.graph_captures()
    want = [g.template_refresh_stats(s) for s in range(2)]
    assert (want[0]["period"], want[1]["period"], want[1]["min_score"]) == (0, 3, 0.25)
    nan, inf = float("nan"), float("inf")
    for stream, period, score in [(2, 2, 0.5), (-2, 2, 0.5), (0, 1, 0.5), (0, -1, 0.5), (None, -7, 0.5), (0, 1000001, 0.5),
                                  (0, 2, nan), (0, 2, inf), (1, 2, -0.1), (None, 2, 1.5)]:
        with pytest.raises(gpu.VtError) as ei:
            if stream == -2:
                gpu._check(gpu.lib().vt_group_set_template_refresh(g._h, -2, period, score))
            else:
                g.set_template_refresh(period, score, stream=stream)
        assert ei.value.code == INVALID, (stream, period, score)
        assert [g.template_refresh_stats(s) for s in range(2)] == want and g.graph_captures() == caps
    with pytest.raises(gpu.VtError) as ei:
        g.template_refresh_stats(2)
    assert ei.value.code == INVALID
    g.set_template_refresh(1000000, 1.0)               # the bounds themselves are fine; -1 (None) is every stream
    assert [g.template_refresh_stats(s)["period"] for s in range(2)] == [1000000, 1000000]
    g.set_template_refresh(0)
    assert g.template_refresh_stats(1)["period"] == 0 and g.update_device([f0, f0])[0].success
    g.close()


def test_enable_under_a_memory_cap_is_refused_and_the_engine_still_tracks(gpu, weights_tiny):
    """64 tiny streams: the second template buffers are 64 x 24 KiB = 1.5 MiB. Under the smallest max_device_mib that
    still creates the engine, less than 1 MiB is left: the enable must return VT_ERR_OOM and change nothing."""
    B = 64

    def create(mib):
        try:
            return gpu.Group(weights_tiny, n_streams=B, max_device_mib=mib, use_graph=False)
        except gpu.VtError as e:
            assert e.code == OOM
            return None

    lo, hi = 0, 4096                                    # (refused, created]
    assert create(1) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        g = create(mid)
        if g is None:
            lo = mid
        else:
            g.close()
            hi = mid
    g = create(hi)
    assert g is not None
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    f0, k0 = _dev(gpu, sc, 0)
    for s in range(B):
        g.init_device(s, f0, gpu.BBox.new(*sc.gt_box(0)))
    tpl = _tpl(g, 5)
    with pytest.raises(gpu.VtError) as ei:
        g.set_template_refresh(2, 0.0)
    assert ei.value.code == OOM
    assert g.template_refresh_stats(5) == dict(period=0, min_score=0.0, generation=0, last_frame=0, skipped_geometry=0)
    f1, k1 = _dev(gpu, sc, 1)
    res = g.update_device([f1] * B)
    assert all(r.success for r in res) and np.array_equal(_tpl(g, 5), tpl)
    g.close()
    roomy = gpu.Group(weights_tiny, n_streams=B, max_device_mib=hi + 2, use_graph=False)
    roomy.set_template_refresh(2, 0.0)
    assert roomy.template_refresh_stats(0)["period"] == 2
    roomy.close()
