"""Frame health, engine level ("health*" keys of vt_group_set_tuning), on the MI355X.

Tiny model, three streams on 320 x 240 MovingSquare NV12 clips. After every collected pass each stream's record is compared
with the NumPy model of tests/frame_health_util.py run on the pictures that stream was shown: exact integers through
Group.frame_health. Refresh periods are 2, the least the refresh policy accepts."""
import numpy as np
import pytest

import frame_health_util as fh
from test_gpu_stream_subsets import _res
from test_gpu_template_refresh import _tpl

pytestmark = pytest.mark.gpu

W, H, B, SIDE = 320, 240, 3, 48
FIELDS = ("status", "frames_done", "flags", "c", "Wg", "Hg", "still", "S1", "S2", "G", "D", "HD", "G_ref")
_cache = {}


def _scs(gpu):
    if "scs" not in _cache:
        _cache["scs"] = [gpu.synth.MovingSquare(W, H, SIDE, seed=5 + s) for s in range(B)]
    return _cache["scs"]


def _buf(gpu, s, t):
    return _scs(gpu)[s].frame_nv12(t)


def _dev(gpu, bufs):
    """device frames of the buffers, one copy each (the overlay draws into them) -> (CFrames, the objects that own them)"""
    devs = [fh.DevFrame(gpu, "nv12", b, W, H) for b in bufs]
    return [d.frame for d in devs], devs


def _group(gpu, weights):
    g = gpu.Group(weights, n_streams=B)
    f0, keep = _dev(gpu, [_buf(gpu, s, 0) for s in range(B)])
    for s in range(B):
        g.init_device(s, f0[s], gpu.BBox.new(*_scs(gpu)[s].gt_box(0)))
    return g


def _check(g, s, want):
    got = g.frame_health(s)
    for k in FIELDS:
        assert got[k] == int(want[k]), f"stream {s}: {k} {got[k]}, model {int(want[k])}"
    for k in ("evaluated", "flagged"):
        assert got[k] == want[k], f"stream {s}: {k} {got[k]}, model {want[k]}"


def _frames_done(g, s):
    return int(g.read_state(s)["frames_done"])


OTHERS = [lambda g, gpu: g.set_template_refresh(2, 0.0), lambda g, gpu: (g.enable_chips(32, gpu.CHIP_RGB8), g.set_chips(2.0)),
          lambda g, gpu: g.set_peaks(3), lambda g, gpu: g.set_tuning("result_overlay", 7)]


def _observe(g):
    chips, infos = g.read_chips()
    return dict(states=[g.read_tensor("state", s).tobytes() for s in range(B)], templates=[_tpl(g, s).tobytes() for s in range(B)],
                peaks=g.last_peaks().tobytes(), chips=chips.tobytes(), chip_infos=infos,
                overlay=[g.result_overlay_stats(s) for s in range(B)], refresh=[g.template_refresh_stats(s) for s in range(B)])


def _same(a, b, ra, rb, what, drawn=None):
    assert [_res(r) for r in ra] == [_res(r) for r in rb], f"{what}: results differ"
    oa, ob = _observe(a), _observe(b)
    for key in oa:
        assert oa[key] == ob[key], f"{what}: {key} differs between the enabled engine and the plain one"
    if drawn:
        assert all(bool((x.t == y.t).all()) for x, y in zip(*drawn)), f"{what}: the drawn frames differ"


# ---- 1. report only ------------------------------------------------------------------------------------------------------

def test_report_only_identity_on_every_kind_of_pass(gpu, weights_tiny):
    """gate 0, refresh, chips, peaks and the overlay on in both engines: the enabled engine equals the plain one in every bit
    the host can see, over two full device passes, a subset pass, a candidate pass, a synchronous host pass and two pipelined
    host passes; records equal the model on device passes and are status 4 on host passes"""
    main, plain = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    for g in (main, plain):
        for enable in OTHERS:
            enable(g, gpu)
    main.set_health(True, still_run=2)
    models = [fh.Stream() for _ in range(B)]
    t = 0

    def device_pass(what, slots, run):
        nonlocal t
        t += 1
        (fa, ka), (fb, kb) = (_dev(gpu, [_buf(gpu, s, t) for s in slots]) for _ in range(2))
        rgb = {s: k.rgb for s, k in zip(slots, ka)}
        ra, rb = run(main, fa), run(plain, fb)
        _same(main, plain, ra[0] if isinstance(ra, tuple) else ra, rb[0] if isinstance(rb, tuple) else rb, what, (ka, kb))
        for s in sorted(set(slots)):
            _check(main, s, models[s].step(rgb[s], still_run=2, frames_done=_frames_done(main, s)))

    for _ in range(2):
        device_pass("full device pass", list(range(B)), lambda g, f: g.update_device(f))
    kept = main.frame_health(1)
    device_pass("subset pass", [2, 0], lambda g, f: g.update_device(f, streams=[2, 0]))
    assert main.frame_health(1) == kept, "a stream that was not in the pass lost its record"
    x, y, w, h = (float(v) for v in main.read_state(0)["box"])
    cands = [(0, (x + 5, y - 4, w, h)), (0, None), 1]
    device_pass("candidate pass", [0, 0, 1], lambda g, f: g.update_device_candidates(cands, f))
    t += 1
    host = lambda: [gpu.NV12Frame(_buf(gpu, s, t), W, H) for s in range(B)]
    ra, rb = main.update_host(host()), plain.update_host(host())
    _same(main, plain, ra, rb, "synchronous host pass")
    for s in range(B):
        _check(main, s, models[s].step(fh.to_rgb("nv12", _buf(gpu, s, t), W, H), still_run=2, device=False, frames_done=_frames_done(main, s)))
        assert main.frame_health(s)["status"] == 4 and main.frame_health(s)["has_prev"] == 0
    for g in (main, plain):
        for k in (1, 2):
            g.enqueue_host([gpu.NV12Frame(_buf(gpu, s, t + k), W, H) for s in range(B)])
    for k in (1, 2):
        ra, rb = main.wait_next(), plain.wait_next()
        assert [_res(r) for r in ra] == [_res(r) for r in rb], f"pipelined host pass {k}: results differ"
    _same(main, plain, ra, rb, "pipelined host pass 2")
    assert all(main.frame_health(s)["status"] == 4 for s in range(B))
    t += 2
    device_pass("device pass behind the host passes", list(range(B)), lambda g, f: g.update_device(f))
    assert all(main.frame_health(s)["status"] == 5 for s in range(B)), "a host pass leaves no previous thumbnail"
    assert sum(main.template_refresh_stats(s)["generation"] for s in range(B)) >= 3 and main.frame_health(0)["gated"] == 0
    main.close()
    plain.close()


# ---- 2. the gate -----------------------------------------------------------------------------------------------------------

def _clip(gpu, s):
    """24 frames: 8-13 repeat frame 7, the picture changes from frame 16 on (luma / 4 + 150), 20 and 21 are constant grey"""
    out = []
    for t in range(24):
        b = _buf(gpu, s, 7 if 8 <= t <= 13 else t).copy()
        if t >= 16:
            b[:W * H] = (b[:W * H].astype(np.int32) // 4 + 150).astype(np.uint8)
        if t in (20, 21):
            b[:] = 128
        out.append(b)
    return out


def _flags_of(gpu, s):
    m = fh.Stream()
    return [m.step(fh.to_rgb("nv12", b, W, H), still_run=2, frames_done=t) for t, b in enumerate(_clip(gpu, s)) if t > 0]


def test_the_clip_shows_every_flag():
    """no GPU work: the model must flag at least one pass of each kind on the clip the gate test relies on"""
    import gstreamer_vit_tracker_amd as vt
    seen = {f for r in _flags_of(vt, 0) for f in (fh.FROZEN, fh.FLAT, fh.CUT) if r["flags"] & f}
    assert seen == {fh.FROZEN, fh.FLAT, fh.CUT}


@pytest.mark.parametrize("pipelined", [False, True])
def test_gate_equals_a_host_twin_under_rule_10(gpu, weights_tiny, pipelined):
    """A: refresh period 2 and the gate. B: gate 0, its host switches a stream's refresh off before exactly the passes the
    model flags and on again behind them. Equal in results, states and template rows on every pass; A's gated counter equals
    the refreshes B's host suppressed, i.e. the flagged passes in which B's refresh, left on, would have fired. pipelined:
    A runs enqueue_device + wait two calls apart from B's synchronous passes - the same bits"""
    a, b = _group(gpu, weights_tiny), _group(gpu, weights_tiny)
    for g in (a, b):
        g.set_template_refresh(2, 0.0)
    a.set_health(True, gate=True, still_run=2)
    b.set_health(True, gate=False, still_run=2)
    clips = [_clip(gpu, s) for s in range(B)]
    want = [_flags_of(gpu, s) for s in range(B)]
    suppressed = [0] * B
    for t in range(1, 24):
        for s in range(B):
            b.set_template_refresh(0 if want[s][t - 1]["flags"] else 2, 0.0, stream=s)
        (fa, ka), (fb, kb) = (_dev(gpu, [clips[s][t] for s in range(B)]) for _ in range(2))
        gen = [b.template_refresh_stats(s)["generation"] for s in range(B)]
        if pipelined:
            a.enqueue_device(fa)
            ra = a.wait()
        else:
            ra = a.update_device(fa)
        rb = b.update_device(fb)
        assert [_res(r) for r in ra] == [_res(r) for r in rb], f"update {t}"
        for s in range(B):
            _check(a, s, dict(want[s][t - 1], evaluated=a.frame_health(s)["evaluated"], flagged=a.frame_health(s)["flagged"]))
            assert a.frame_health(s)["flags"] == b.frame_health(s)["flags"] == want[s][t - 1]["flags"]
            sa, sb = a.read_state(s), b.read_state(s)
            assert all(np.array_equal(sa[k], sb[k]) for k in sa), f"update {t}, stream {s}: states differ"
            assert np.array_equal(_tpl(a, s), _tpl(b, s)), f"update {t}, stream {s}: template rows differ"
            # B's host suppressed a refresh where the stream was due by rules 1-5 in a flagged pass
            st, r = sb, rb[s]
            if want[s][t - 1]["flags"] and r.success and int(st["frames_done"]) - int(st["tpl_frame"]) >= 2 and \
                    int(st["window_miss"]) != int(st["frames_done"]):
                suppressed[s] += 1
            assert b.template_refresh_stats(s)["generation"] - gen[s] in (0, 1)
    gated = [a.frame_health(s)["gated"] for s in range(B)]
    assert gated == suppressed and sum(gated) >= 3, (gated, suppressed)
    assert sum(a.template_refresh_stats(s)["generation"] for s in range(B)) >= 3, "the run must refresh too"
    assert all(b.frame_health(s)["gated"] == 0 for s in range(B))
    a.close()
    b.close()


# ---- 3. plumbing -----------------------------------------------------------------------------------------------------------

def test_plumbing(gpu, weights_tiny):
    g = _group(gpu, weights_tiny)
    with pytest.raises(gpu.VtError):
        g.frame_health(0)                               # not enabled
    g.set_tuning("health_max_cells", 8192)
    g.set_health(True, still_run=1)
    with pytest.raises(gpu.VtError):
        g.set_tuning("health_max_cells", 4096)          # frozen by the enable
    for bad in (("health", 2), ("health_cell", 5), ("health_period", 0), ("health_flat_q", 4081), ("health_nothing", 1)):
        with pytest.raises(gpu.VtError):
            g.set_tuning(*bad)
    captures = g.graph_captures()

    def run(t):
        f, keep = _dev(gpu, [_buf(gpu, s, t) for s in range(B)])
        return g.update_device(f)

    run(1)
    run(1)
    assert all(g.frame_health(s)["flags"] == fh.FROZEN and g.frame_health(s)["still"] == 1 for s in range(B))
    assert g.frame_health(0)["c"] == 4 and g.frame_health(0)["Wg"] * g.frame_health(0)["Hg"] == 4800
    # init, import and copy reset the stream: the next pass has nothing to compare with
    f, keep = _dev(gpu, [_buf(gpu, 0, 1)])
    g.init_device(0, f[0], gpu.BBox.new(*_scs(gpu)[0].gt_box(1)))
    blob = g.export_stream(2)
    g.import_stream(1, blob)
    for s in (0, 1):
        r = g.frame_health(s)
        assert (r["status"], r["has_prev"], r["still"], r["flags"]) == (0, 0, 0, 0), (s, r)
    assert g.frame_health(2)["flags"] == fh.FROZEN
    run(1)
    assert [g.frame_health(s)["status"] for s in range(B)] == [5, 5, 1]
    g.copy_stream(2, g, 0)
    assert g.frame_health(0)["status"] == 0 and g.frame_health(0)["has_prev"] == 0
    run(1)
    assert [g.frame_health(s)["status"] for s in range(B)] == [5, 1, 1]
    # "health" 0 zeroes the records and the bookkeeping; the launches leave at once
    counts = [g.frame_health(s)["evaluated"] for s in range(B)]
    g.set_tuning("health", 0)
    assert all(g.frame_health(s)["status"] == 0 and g.frame_health(s)["has_prev"] == 0 and g.frame_health(s)["on"] == 0 for s in range(B))
    run(2)
    assert all(g.frame_health(s)["status"] == 0 for s in range(B)) and [g.frame_health(s)["evaluated"] for s in range(B)] == counts
    g.set_tuning("health", 1)
    run(2)
    assert all(g.frame_health(s)["status"] == 5 for s in range(B))
    g.set_tuning("health_period", 2)
    done = _frames_done(g, 0)
    run(3)
    assert g.frame_health(0)["frames_done"] == (done + 1 if (done + 1) % 2 == 0 else done)      # not due: the record stays
    assert g.graph_captures() == captures, "an update captured a graph"
    v = g.read_tensor("health", 0)
    assert v.shape == (24,) and v[16:22].tolist() == [2, 0, 1, 32, 500, 0]
    g.close()
