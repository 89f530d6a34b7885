"""Motion prior inside the passes (the "motion_*" keys of vt_group_set_tuning), on the MI355X.

Tiny model, the 480 x 360 clip of tests/golden/motion_prior_tiny.npz (24-px target, up to 31 px per update, one occlusion
of three updates), 3 streams at different phases of it. The tests rest on the twin identity: a motion-enabled engine equals, bit for bit, a
plain engine whose host moves the boxes through vt_group_set_state_box as tests/motion_prior_util.py (the NumPy-float32 model)
says - results, state words, records, and with them templates, chips, peaks and drawn frames."""
import importlib.util
import os
import struct

import numpy as np
import pytest

import motion_prior_util as mu

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
B, PHASES, UPDATES = 3, (0, 5, 11), 40
_cache = {}


def _fx():
    """the fixture, its scene and UPDATES + max(PHASES) + 1 RGB8 frames of it - made once for the whole module"""
    if not _cache:
        spec = importlib.util.spec_from_file_location("_make_motion_prior", os.path.join(HERE, "golden", "make_motion_prior.py"))
        mk = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mk)
        sc, ts, frames = mk.clip(UPDATES + max(PHASES) + 1)
        _cache.update(mk=mk, fx=dict(np.load(os.path.join(HERE, "golden", "motion_prior_tiny.npz"))), sc=sc, ts=ts, frames=frames)
    return _cache


def _pol():
    return mu.Policy(*_fx()["fx"]["policy"])


def _res(r):
    return tuple(r.bbox), int(r.success), struct.unpack("<I", struct.pack("<f", r.score))[0]


def _states(g):
    return [g.read_tensor("state", s).tobytes() for s in range(g.streams)]


class Up:
    """an RGB8 frame uploaded to the device"""

    def __init__(self, gpu, rgb):
        import torch
        h, w, _ = rgb.shape
        self.buf = np.ascontiguousarray(rgb, np.uint8).reshape(-1)
        self.t = torch.from_numpy(self.buf.copy()).cuda()
        self.frame = gpu.frame_rgb8(self.t.data_ptr(), w, h)

    def read(self):
        return self.t.cpu().numpy()


def _ups(gpu, frames):
    """the frames uploaded; the caller keeps the list for as long as a pass may read them (a CFrame holds an address only)"""
    return [Up(gpu, f) for f in frames]


def _frame_of(s, k):
    """stream s's frame of its update k (k = 0: the init frame), and the ground truth there"""
    c = _fx()
    return c["frames"][PHASES[s] + k], c["sc"].gt_box(c["ts"][PHASES[s] + k])


def _group(gpu, weights, n=B, motion=True, init=None, **kw):
    g = gpu.Group(weights, n_streams=n, **kw)
    for s in (range(n) if init is None else init):
        fr, box = _frame_of(s, 0)
        u = Up(gpu, fr)
        g.init_device(s, u.frame, gpu.BBox.new(*box))
    if motion:
        g.set_motion_prior(*[(bool(v) if i == 0 else int(v)) for i, v in enumerate(_pol().tuple())])
    return g


def _check_records(a, tw, what):
    for s in range(a.streams):
        got = a.read_tensor("motion", s)
        assert got.tobytes() == tw.recs[s].read_out(1).tobytes(), f"{what}: the record of stream {s} is not the model's: {got}"


def _pass(gpu, a, t, tw, kind, k):
    """one pass of `kind` on the motion engine a and on the plain twin t (driven through tw); -> (results a, results t)"""
    host = kind.startswith("host")
    fr = [_frame_of(s, k)[0] for s in range(B)]
    keep = [] if host else [_ups(gpu, fr), _ups(gpu, fr)]       # alive until both passes have returned
    fa = fr if host else [u.frame for u in keep[0]]
    ft = fr if host else [u.frame for u in keep[1]]
    winners = has_box = None
    if kind in ("full", "host"):
        lst = list(range(B))
        tw.before(lst)
        ra = a.update_host(fa) if host else a.update_device(fa)
        rt = t.update_host(ft) if host else t.update_device(ft)
    elif kind in ("subset", "host_subset"):
        lst = [2, 0]        # slot 0 is stream 2
        tw.before(lst)
        sa, st_ = [fa[s] for s in lst], [ft[s] for s in lst]
        ra = a.update_host(sa, streams=lst) if host else a.update_device(sa, streams=lst)
        rt = t.update_host(st_, streams=lst) if host else t.update_device(st_, streams=lst)
    else:                   # candidates: stream 0 twice - its own (predicted) box and one the caller places -, stream 1 plain
        box = a.read_state(0)["box"]
        assert box.tobytes() == t.read_state(0)["box"].tobytes()
        off = (14.0, -9.0) if k % 2 else (-40.0, 30.0)     # near: it may win; far: it loses
        cands = [0, (0, (float(box[0]) + off[0], float(box[1]) + off[1], float(box[2]), float(box[3]))), 1]
        lst, has_box = [0, 0, 1], [0, 1, 0]
        tw.before(lst)
        sa, st_ = [fa[s] for s in lst], [ft[s] for s in lst]
        if host:
            (ra, winners), (rt, wt) = a.update_host_candidates(cands, sa), t.update_host_candidates(cands, st_)
        else:
            (ra, winners), (rt, wt) = a.update_device_candidates(cands, sa), t.update_device_candidates(cands, st_)
        assert winners == wt
    tw.after(lst, rt, winners, has_box)
    return ra, rt, lst, winners


KINDS = {"device": ("full", "subset", "cand", "full", "full"), "host": ("host", "host_subset", "host_cand", "host")}


@pytest.mark.parametrize("route", ["device", "host"])
def test_twin_identity_on_every_kind_of_pass(gpu, weights_tiny, route, capsys):
    """40 updates, 3 streams at different phases of the clip (each meets the occlusion at another time; streams left out of a
    subset pass meet larger jumps): full, subset (slot != stream) and candidate passes with mixed has_box - on device frames,
    and through the synchronous host calls"""
    a, t = _group(gpu, weights_tiny), _group(gpu, weights_tiny, motion=False)
    tw = mu.Twin(t, _pol())
    caps = a.graph_captures()
    placed_wins = fails = 0
    for k in range(1, UPDATES + 1):
        kind = KINDS[route][k % len(KINDS[route])]
        ra, rt, lst, winners = _pass(gpu, a, t, tw, kind, k)
        assert [_res(r) for r in ra] == [_res(r) for r in rt], f"update {k} ({kind}): results differ from the twin's"
        assert _states(a) == _states(t), f"update {k} ({kind}): state words differ from the twin's"
        _check_records(a, tw, f"update {k} ({kind})")
        if winners is not None:
            placed_wins += winners[0] == 1
        fails += sum(1 for i, r in enumerate(ra) if not r.success and (winners is None or winners[i] == i))
    m = [a.motion(s) for s in range(B)]
    assert a.graph_captures() == caps, "a graph was captured after the enable"
    assert sum(x["n_shift"] for x in m) >= 30 and fails >= 3, "the run exercises little: few shifts or no failed update"
    assert sum(x["n_coast"] for x in m) >= 3, "no failed update coasted"
    with capsys.disabled():
        print(f"\n[{route}] shifts {[x['n_shift'] for x in m]} coasts {[x['n_coast'] for x in m]} failed updates {fails} "
              f"placed slot won {placed_wins}x")
    with pytest.raises(gpu.VtError):
        t.read_tensor("motion", 0)          # never enabled
    a.close()
    t.close()


def test_oracle_parity_and_the_plain_engine_loses_the_target(gpu, weights_tiny, capsys):
    """the fixture's clip on one stream: every box within 1 px of the oracle's, equal success flags, the target held where the
    fixture says the reference holds it - and a plain engine, like the plain oracle, never finds it again behind the gap"""
    c = _fx()
    fx, mk = c["fx"], c["mk"]
    n = int(fx["n"]) - 1
    a, p = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    for g in (a, p):
        u = Up(gpu, c["frames"][0])
        g.init_device(0, u.frame, gpu.BBox.new(*[int(v) for v in fx["box0"]]))
    a.set_motion_prior(True, *[int(v) for v in fx["policy"][1:]])
    worst, ious = 0, []
    for i in range(n):
        ua, up = Up(gpu, c["frames"][i + 1]), Up(gpu, c["frames"][i + 1])
        ra = a.update_device([ua.frame])[0]
        rp = p.update_device([up.frame])[0]
        d = max(abs(int(x) - int(y)) for x, y in zip(ra.bbox, fx["bbox"][i]))
        worst = max(worst, d)
        assert d <= 1, f"update {i}: box {tuple(ra.bbox)} against the oracle's {tuple(fx['bbox'][i])}"
        assert int(ra.success) == int(fx["success"][i]), f"update {i}: success {ra.success}, the oracle's {fx['success'][i]}"
        assert int(rp.success) == int(fx["plain_success"][i]), f"update {i}: the plain engine's success differs from the plain oracle's"
        ious.append(mu.iou(ra.bbox, fx["gt"][i]))
    vis = fx["hidden"] == 0
    ious = np.array(ious)
    assert ious[vis].min() >= float(fx["min_iou"]) - 0.15, "the motion engine leaves the target where the reference holds it"
    last_hidden = int(np.flatnonzero(~vis).max())
    assert not fx["plain_success"][last_hidden + 1:].any() and p.read_state(0)["success_count"] == int(fx["plain_success"].sum())
    m = a.motion(0)
    assert m["n_coast"] == int(fx["rec_words"][-1][10]) and m["n_shift"] == int(fx["rec_words"][-1][9])
    with capsys.disabled():
        print(f"\nworst box difference {worst} px, min IoU on visible frames {ious[vis].min():.3f} (the oracle's {float(fx['min_iou']):.3f})")
    a.close()
    p.close()


def test_pipelined_host_equals_synchronous_and_redoes(gpu, weights_tiny, capsys):
    """enqueue_host / wait_next two deep, the _streams forms, a camera joining through enqueue_init_host: results of every
    pass, final states and records equal the synchronous motion engine's. A 5 % margin makes speculative windows miss on this
    clip, so the records are rewound with the states (host_redos > 0)."""
    p = _group(gpu, weights_tiny, init=(0, 1), host_window_margin_pct=5)
    s = _group(gpu, weights_tiny, init=(0, 1))
    JOIN = 9
    plan = []       # (k, list) per pass; stream 2 joins behind pass JOIN
    for k in range(1, 31):
        lst = [0, 1] if k <= JOIN else ([0, 1, 2] if k % 3 else [2, 0])
        plan.append((k, lst))

    def frames_of(k, lst):
        # stream 2's clock starts when it joins
        return [_frame_of(x, k - JOIN if x == 2 else k)[0] for x in lst]

    def sync_pass(k, lst):
        if k == JOIN + 1:
            fr, box = _frame_of(2, 0)
            s.init_host(2, fr, gpu.BBox.new(*box))
        full = lst == list(range(B))
        return s.update_host(frames_of(k, lst), streams=None if full else lst)

    got, want = [], []
    for i, (k, lst) in enumerate(plan):
        if k == JOIN + 1:       # while pass JOIN is still outstanding
            fr, box = _frame_of(2, 0)
            p.enqueue_init_host(2, fr, gpu.BBox.new(*box))
        full = lst == list(range(B))
        if full:
            p.enqueue_host(frames_of(k, lst))
        else:
            p.enqueue_host(frames_of(k, lst), streams=lst)
        if i >= 1:
            got.append(p.wait_next())
            want.append(sync_pass(*plan[i - 1]))
        if k == 15:             # refused while a pass is outstanding, with nothing changed
            before = p.host_redos()
            for key, v in (("motion_prior", 0), ("motion_gain_pct", 10), ("motion_coast", 1), ("motion_max_pct", 10)):
                with pytest.raises(gpu.VtError):
                    p.set_tuning(key, v)
            assert p.host_redos() == before
    got.append(p.wait_next())
    want.append(sync_pass(*plan[-1]))
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert [_res(r) for r in g_] == [_res(r) for r in w_], f"pass {plan[i]}: the pipelined results differ from the synchronous ones"
    assert _states(p) == _states(s)
    for x in range(B):
        assert p.read_tensor("motion", x).tobytes() == s.read_tensor("motion", x).tobytes(), f"record of stream {x}"
    assert p.host_redos() > 0 and s.host_redos() == 0, "no speculative window missed: the rewind of the records is not exercised"
    assert p.motion(0)["on"] == 1 and p.motion(0)["n_shift"] > 10
    with capsys.disabled():
        print(f"\nhost_redos {p.host_redos()} in {len(plan)} pipelined passes at a 5 % margin")
    p.close()
    s.close()


def test_launches_and_captures(gpu, weights_tiny):
    """a never-enabled engine launches what it always did, an enabled one exactly two more; nothing is captured after the
    enable - across both crop-tier boundaries and after every refused call"""
    a, t = _group(gpu, weights_tiny, motion=False), _group(gpu, weights_tiny, motion=False)
    ups = _ups(gpu, [_frame_of(s, 1)[0] for s in range(B)])
    fr = [u.frame for u in ups]
    plain = t.profile_device(fr, 1)
    assert a.profile_device(fr, 1) is not None
    assert not [p for p in plain if "motion" in p["name"]]
    caps0 = a.graph_captures()
    a.set_tuning("motion_gain_pct", 70)        # remembered: no capture, no record yet
    assert a.graph_captures() == caps0
    with pytest.raises(gpu.VtError):
        a.read_tensor("motion", 0)
    a.set_motion_prior(True, coast=5, max_pct=200)
    caps = a.graph_captures()
    assert caps > caps0, "the enable did not capture the passes again"
    on = a.profile_device(fr, 1)
    names_on, names_plain = [p["name"] for p in on], [p["name"] for p in plain]
    assert names_on[0] == "motion_place" and [n for n in names_on if not n.startswith("motion_")] == names_plain
    assert sum(p["launches"] for p in on) == sum(p["launches"] for p in plain) + 2
    k = names_on.index("motion_settle")
    assert "decode" in names_on[k - 1], f"settle is not directly behind the decode: {names_on}"
    assert [p["name"] for p in t.profile_device(fr, 1)] == names_plain
    a.set_motion_prior(False)      # off and on again: copies, no capture
    a.set_motion_prior(True)
    replays0 = a.read_tensor("graph_replays").copy()
    # the tiny model's crop changes its tier between 40 and 48 px and between 56 and 64 px (preproc_tier_for_box); the pass
    # behind a set_state_box takes the tier of that box
    for side in (24, 48, 64, 56, 40, 100, 24):
        for s in range(B):
            a.set_state_box(s, (100.0 + s, 90.0, float(side), float(side)))
        a.update_device(fr)
    rep = a.read_tensor("graph_replays") - replays0
    assert rep.tolist() == [3, 2, 2], f"not every crop tier's graph was replayed: {rep}"
    for key, v in (("motion_prior", 2), ("motion_gain_pct", 0), ("motion_gain_pct", 101), ("motion_coast", 61), ("motion_max_pct", 201),
                   ("motion_nonsense", 1)):
        before = [a.read_tensor("motion", s).tobytes() for s in range(B)]
        with pytest.raises(gpu.VtError):
            a.set_tuning(key, v)
        assert [a.read_tensor("motion", s).tobytes() for s in range(B)] == before
    for key in ("motion_gain_pct", "motion_coast", "motion_max_pct"):      # later changes: one copy, no capture
        a.set_tuning(key, 7)
        a.set_tuning(key, -1)
    a.update_device(fr)
    assert a.graph_captures() == caps, "a graph was captured after the enable"
    a.close()
    t.close()


def test_interplay_with_refresh_chips_peaks_and_overlay(gpu, weights_tiny, oracle):
    """all four optional launches beside the prior: the engine equals the set_state_box twin with the same four enabled -
    templates, chips, peak records and the drawn frames' bytes"""
    a, t = _group(gpu, weights_tiny), _group(gpu, weights_tiny, motion=False)
    tw = mu.Twin(t, _pol())
    for g in (a, t):
        g.set_template_refresh(3, 0.0)
        g.enable_chips(64, gpu.CHIP_RGB8)
        g.set_chips(2.0)
        g.set_peaks(4, 2, 0.0)
        g.set_result_overlay(min_score_pct=0)
    drawn = 0
    for k in range(1, 29):
        lst = list(range(B)) if k % 4 else [1, 2]
        ua, ut = [Up(gpu, _frame_of(s, k)[0]) for s in lst], [Up(gpu, _frame_of(s, k)[0]) for s in lst]
        tw.before(lst)
        full = len(lst) == B
        ra = a.update_device([u.frame for u in ua], streams=None if full else lst)
        rt = t.update_device([u.frame for u in ut], streams=None if full else lst)
        tw.after(lst, rt)
        assert [_res(r) for r in ra] == [_res(r) for r in rt], f"update {k}"
        assert _states(a) == _states(t), f"update {k}: states"
        for s in range(B):
            assert np.array_equal(a.read_tensor("template", s), t.read_tensor("template", s)), f"update {k}: template of stream {s}"
        ca, ia = a.read_chips()
        ct, it = t.read_chips()
        assert np.array_equal(ca, ct) and ia == it, f"update {k}: chips"
        assert a.last_peaks().tobytes() == t.last_peaks().tobytes(), f"update {k}: peaks"
        for x, y in zip(ua, ut):
            fa = x.read()
            assert np.array_equal(fa, y.read()), f"update {k}: drawn frames differ"
            drawn += int((fa != x.buf).any())
    assert drawn >= 20 and sum(a.template_refresh_stats(s)["generation"] for s in range(B)) >= 3
    assert sum(a.motion(s)["n_shift"] for s in range(B)) >= 20
    a.close()
    t.close()


def test_resets_snapshots_and_refusals(gpu, weights_tiny):
    """every call that gives a stream a state from outside zeroes its record (and no other stream's); the record is no part of
    a snapshot; switching the prior off zeroes every record"""
    a, plain = _group(gpu, weights_tiny), _group(gpu, weights_tiny, motion=False)
    other = _group(gpu, weights_tiny)
    clock = [0]

    def run(n=3, check=False):
        for _ in range(n):
            clock[0] += 1
            for g in (a, other):
                ups = _ups(gpu, [_frame_of(s, clock[0])[0] for s in range(B)])
                g.update_device([u.frame for u in ups])
        for s in range(B):
            m = a.motion(s)
            assert not check or (m["v"] != (0.0, 0.0) and m["live"] == 5), "the warm-up left no velocity to reset"

    def rec(g, s):
        return g.read_tensor("motion", s).tobytes()

    zero = mu.Record().read_out(1).tobytes()
    run(check=True)
    blob = a.export_stream(0)
    # init_device / init_host / set_state_box: the stream's own record, nobody else's
    fr, box = _frame_of(0, clock[0])
    u0 = Up(gpu, fr)
    a.init_device(0, u0.frame, gpu.BBox.new(*box))
    assert rec(a, 0) == zero and rec(a, 1) != zero and rec(a, 2) != zero
    fr1, box1 = _frame_of(1, clock[0])
    a.init_host(1, fr1, gpu.BBox.new(*box1))
    assert rec(a, 1) == zero and rec(a, 2) != zero
    a.set_state_box(2, a.read_state(2)["box"])
    assert rec(a, 2) == zero
    run()
    assert all(rec(a, s) != zero for s in range(B))
    # import_stream, and the DESTINATION of copy_stream (its source keeps its record)
    a.import_stream(0, blob)
    assert rec(a, 0) == zero and rec(a, 1) != zero
    other.copy_stream(2, a, 1)
    assert rec(a, 1) == zero and rec(other, 2) != zero and rec(a, 2) != zero
    # enqueue_init_host behind an outstanding pass zeroes the record of the stream it starts, and only that
    a.enqueue_host([_frame_of(s, clock[0] + 1)[0] for s in (0, 1)], streams=[0, 1])
    fr2, box2 = _frame_of(2, clock[0])
    a.enqueue_init_host(2, fr2, gpu.BBox.new(*box2))
    a.wait_next()
    assert rec(a, 2) == zero
    # a single tracker: the same keys through vt_tracker_as_group, and vt_import_state resets
    trk = gpu.VitTrack.new(weights_tiny)
    f0, b0 = _frame_of(0, 0)
    u0 = Up(gpu, f0)
    trk.init_device(u0.frame, gpu.BBox.new(*b0))
    trk.set_motion_prior(True, 70, 5, 200)
    for k in range(1, 4):
        u0 = Up(gpu, _frame_of(0, k)[0])
        trk.update_device(u0.frame)
    assert trk.motion()["v"] != (0.0, 0.0) and trk.motion()["on"] == 1
    trk.import_state(trk.export_state())
    assert trk.motion()["v"] == (0.0, 0.0) and trk.motion()["live"] == 0 and trk.motion()["n_shift"] == 0
    # no part of a snapshot: size and bytes are those of a never-enabled engine holding the same stream
    assert a.snapshot_bytes() == plain.snapshot_bytes() == gpu.snapshot_bytes(a.model_info())
    src = a.export_stream(0)
    plain.import_stream(0, src)
    assert plain.export_stream(0) == src
    # switching off zeroes every record, and an engine that is off learns nothing
    a.set_motion_prior(False)
    off = mu.Record().read_out(0).tobytes()
    assert all(rec(a, s) == off for s in range(B))
    run(1)
    assert all(a.motion(s)["v"] == (0.0, 0.0) and a.motion(s)["n_shift"] == 0 and a.motion(s)["live"] == 0 for s in range(B))
    for g in (a, plain, other):
        g.close()
    trk.close()
