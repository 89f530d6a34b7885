"""Pipelined host passes over a subset of a group's streams (vt_group_enqueue_host_streams / vt_group_wait_next) and
the queued init (vt_group_enqueue_init_host).

A multi-camera host updates only the cameras that are tracking (src/tracker_context.rs:88-90,120) and initialises a
camera when its selection is confirmed, while the others keep tracking. The yardstick of every check is the synchronous
path on a second group fed the same frames, lists and init boxes (vt_group_update_host_streams / vt_group_update_host /
vt_group_init_host): every equality is bit-identity of box, success flag and score - and, where stated, of the raw
state words - so no tolerance is chosen anywhere in this file.

The loop every pipelined run here uses keeps two passes in flight: queued inits of frame t (two passes outstanding),
collect pass t-2, enqueue pass t (upload beside pass t-1)."""
import ctypes
import struct
import threading

import numpy as np
import pytest

from conftest import iou
from test_gpu_trajectories import BARS, LOW_IOU_FRAMES, _clip, _fixture

pytestmark = pytest.mark.gpu

W, H, B, N = 640, 480, 8, 28
INVALID, NOT_INIT = -1, -6
FRAMES_DONE = 11                        # StreamState word that counts the stream's own passes
FMTS = ["nv12", "rgb8", "nv12", "rgb8", "nv12", "rgb8", "bgrx", "nv12"]     # stream -> format of its camera
FRAME_BYTES = {"nv12": W * H * 3 // 2, "rgb8": W * H * 3, "bgrx": W * H * 4}
_PIXELS = {}


def _clips(gpu, n=B):
    return [gpu.synth.MovingSquare(W, H, 48 + 4 * i, seed=20 + i) for i in range(n)]


def _pixels(sc, fmt, t):
    """the bytes of frame t of a clip in a format (cached: several tests and both groups of a test read them)"""
    key = (sc.seed, sc.sq, fmt, t)
    if key not in _PIXELS:
        if fmt == "nv12":
            a = np.ascontiguousarray(sc.frame_nv12(t))
        else:
            a = sc.frame_rgb8(t)
            if fmt == "bgrx":
                a = np.concatenate([a[..., ::-1], np.full(a.shape[:2] + (1,), 7, np.uint8)], axis=2)
            a = np.ascontiguousarray(a)
        _PIXELS[key] = a
    return _PIXELS[key]


def _frame(gpu, sc, fmt, t, into=None):
    """host frame object of frame t; `into`: a byte buffer the pixels are copied to and used from (registered memory)"""
    a = _pixels(sc, fmt, t)
    if into is not None:
        v = into[:a.size].reshape(a.shape)
        v[...] = a
        a = v
    if fmt == "nv12":
        return gpu.NV12Frame(a, W, H)
    return gpu.BGRXFrame(a) if fmt == "bgrx" else a


def _frames(gpu, scs, t, L=None):
    return [_frame(gpu, scs[s], FMTS[s], t) for s in (range(len(scs)) if L is None else L)]


def _words(g, s):
    return g.read_tensor("state", s).view(np.uint32).copy()


def _res(r):
    """a result as exact bits: box, success flag, score's float32 pattern"""
    return tuple(r.bbox), int(r.success), struct.unpack("<I", struct.pack("<f", r.score))[0]


def _replays(g):
    return int(g.read_tensor("graph_replays").sum())


def _init_all(gpu, groups, scs, streams=None, frame_of=None):
    for s in (range(len(scs)) if streams is None else streams):
        f = frame_of(s, 0) if frame_of else _frame(gpu, scs[s], FMTS[s], 0)
        for g in groups:
            g.init_host(s, f, gpu.BBox.new(*scs[s].gt_box(0)))


def _pipelined(grp, n, pass_at, inits_at=None, t0=1, on_enqueued=None):
    """passes t0..n-1, two in flight. pass_at(t) -> (list or None for the full pass, frames); inits_at(t) -> [(stream,
    frame, box)] queued before pass t, while passes t-2 and t-1 are outstanding. -> {t: results}"""
    got = {}
    for t in range(t0, n):
        for s, f, box in (inits_at(t) if inits_at else []):
            grp.enqueue_init_host(s, f, box)
        if t - 2 >= t0:
            got[t - 2] = grp.wait_next()
        L, frames = pass_at(t)
        grp.enqueue_host(frames, streams=L)
        if on_enqueued:
            on_enqueued(t, L)
    for t in range(max(n - 2, t0), n):
        got[t] = grp.wait_next()
    return got


def _synchronous(grp, n, pass_at, inits_at=None, t0=1):
    want = {}
    for t in range(t0, n):
        for s, f, box in (inits_at(t) if inits_at else []):
            grp.init_host(s, f, box)
        L, frames = pass_at(t)
        want[t] = grp.update_host(frames, streams=L)
    return want


def _assert_equal(got, want, lists):
    assert sorted(got) == sorted(want)
    for t in sorted(want):
        assert len(got[t]) == len(want[t]) == len(lists[t]), (t, len(got[t]), len(want[t]))
        for i, s in enumerate(lists[t]):
            assert _res(got[t][i]) == _res(want[t][i]), f"frame {t}, stream {s} (slot {i}): {got[t][i]} vs {want[t][i]}"


def _schedule(seed=5):
    """the list of every frame 1..N-1 from a seeded generator, with the cases the test names pinned at fixed frames"""
    rng = np.random.default_rng(seed)
    sched = {t: [int(s) for s in rng.permutation(B)[:int(rng.integers(2, B))]] for t in range(1, N)}
    sched[3] = [3]                                          # n = 1
    sched[6] = list(range(B))                               # n = B, identity order: the full pass
    sched[7] = [int(s) for s in rng.permutation(B)]        # n = B permuted
    if sched[7] == list(range(B)):
        sched[7] = sched[7][::-1]
    sched[10], sched[11] = [0, 1, 2], [4, 5, 6]             # disjoint consecutive lists
    sched[12] = [5, 6, 7, 0]                                # shares 5 and 6 with the pass before it
    sched[14] = [7, 1, 3]
    for t in range(15, 19):                                 # stream 7 sits out four frames ...
        sched[t] = [s for s in sched[t] if s != 7] or [2]
    sched[19] = [2, 7]                                      # ... and returns
    return sched


def _check_schedule(sched):
    sizes = {len(L) for L in sched.values()}
    assert 1 in sizes and list(range(B)) in sched.values()
    assert any(len(L) == B and L != list(range(B)) for L in sched.values())
    ts = sorted(sched)
    assert any(not set(sched[a]) & set(sched[b]) for a, b in zip(ts, ts[1:]))
    assert any(set(sched[a]) & set(sched[b]) and set(sched[a]) != set(sched[b]) for a, b in zip(ts, ts[1:]))
    out = [t for t in ts if 7 not in sched[t]]
    assert any(all(t + k in out for k in range(3)) and any(7 in sched[u] for u in ts if u > t + 2) for t in out)
    assert len(ts) >= 24 and all(len(set(L)) == len(L) for L in sched.values())


def _varying_lists(gpu, weights, margin_pct, zero_copy=0, frame_of=None):
    """case 1's run: -> (pipelined group, synchronous group), every check of the case made"""
    scs = _clips(gpu)
    sched = _schedule()
    _check_schedule(sched)
    pipe = gpu.Group(weights, n_streams=B, host_window_margin_pct=margin_pct, host_zero_copy=zero_copy)
    sync = gpu.Group(weights, n_streams=B)
    _init_all(gpu, [pipe], scs, frame_of=frame_of)
    _init_all(gpu, [sync], scs)
    caps = pipe.graph_captures()
    replays = {}

    def pipe_pass(t):
        L = sched[t]
        return L, [frame_of(s, t) for s in L] if frame_of else _frames(gpu, scs, t, L)

    def note(t, L):
        if L == list(range(B)):
            replays[t] = _replays(pipe)

    before = _replays(pipe)
    got = _pipelined(pipe, N, pipe_pass, on_enqueued=note)
    want = _synchronous(sync, N, lambda t: (sched[t], _frames(gpu, scs, t, sched[t])))
    _assert_equal(got, want, sched)
    # the identity list replayed the captured graph; no list captured one
    assert replays and all(v > before for v in replays.values()), (before, replays)
    assert pipe.graph_captures() == caps
    done = [sum(s in L for L in sched.values()) for s in range(B)]
    for s in range(B):
        ws, wp = _words(sync, s), _words(pipe, s)
        assert ws[FRAMES_DONE] == done[s], (s, ws[FRAMES_DONE], done[s])
        assert np.array_equal(wp, ws), f"state words of stream {s}"
    return pipe, sync


# ---- 1. pipelined = synchronous, varying lists ----------------------------------------------------------------------

@pytest.mark.parametrize("margin_pct,expect_redo", [(0, False), (-1, True)])
def test_pipelined_subset_passes_equal_synchronous_ones(gpu, weights_tiny, margin_pct, expect_redo):
    """27 frames whose list changes every frame (n = 1, the identity list, a permuted full list, disjoint and
    overlapping neighbours, a stream that sits out four frames): every listed stream's result of every frame, and at
    the end every stream's state words, equal the synchronous group's - with the default enlargement (no redo) and
    with it switched off, where moving targets leave their speculative windows and passes are redone over their own
    lists."""
    pipe, sync = _varying_lists(gpu, weights_tiny, margin_pct)
    assert (pipe.host_redos() > 0) == expect_redo, pipe.host_redos()
    if not expect_redo:
        assert pipe.host_redos() == 0


# ---- 2. exact windows for streams outside the outstanding pass ---------------------------------------------------

def test_streams_outside_the_outstanding_pass_get_exact_windows(gpu, weights_tiny):
    """no enlargement (margin -1), moving targets: two alternating DISJOINT lists never redo - a stream that is not in
    the outstanding pass has an exact known box - where one constant list on the same clips does"""
    scs = _clips(gpu)
    even, odd = [0, 2, 4, 6], [1, 3, 5, 7]
    redos = {}
    for name, list_at in (("alternating", lambda t: even if t % 2 == 0 else odd), ("constant", lambda t: even + odd)):
        pipe = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1)
        sync = gpu.Group(weights_tiny, n_streams=B)
        _init_all(gpu, [pipe, sync], scs)
        pass_at = lambda t: (list_at(t), _frames(gpu, scs, t, list_at(t)))
        got = _pipelined(pipe, N, pass_at)
        want = _synchronous(sync, N, pass_at)
        _assert_equal(got, want, {t: list_at(t) for t in range(1, N)})
        redos[name] = pipe.host_redos()
    assert redos["alternating"] == 0 and redos["constant"] > 0, redos


# ---- 3. full and subset passes interleaved -----------------------------------------------------------------------

def test_full_and_subset_passes_interleave(gpu, weights_tiny):
    """enqueue_host, enqueue_host_streams, enqueue_host ... two in flight, equal to the synchronous sequence; a
    wait_next with room for more results than the collected pass had writes that pass's entries only"""
    L_ = gpu.lib()
    scs = _clips(gpu)
    pipe, sync = gpu.Group(weights_tiny, n_streams=B), gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, [pipe, sync], scs)
    subsets = [[6, 1], [3], [7, 6, 5, 4, 3, 2, 1], [0, 2, 4], [5, 7, 0, 1]]
    list_at = lambda t: None if t % 2 else subsets[(t // 2) % len(subsets)]
    lists = {t: list_at(t) or list(range(B)) for t in range(1, 14)}
    pass_at = lambda t: (list_at(t), _frames(gpu, scs, t, list_at(t)))
    caps, r0 = pipe.graph_captures(), _replays(pipe)
    got = _pipelined(pipe, 14, pass_at)
    want = _synchronous(sync, 14, pass_at)
    _assert_equal(got, want, lists)
    assert _replays(pipe) == r0 + sum(list_at(t) is None for t in range(1, 14)) and pipe.graph_captures() == caps
    assert pipe.host_redos() == 0
    # n larger than the collected pass: a guard value behind its entries stays
    pipe.enqueue_host(_frames(gpu, scs, 14, [5, 2, 3]), streams=[5, 2, 3])
    pipe.enqueue_host(_frames(gpu, scs, 15))
    exp = sync.update_host(_frames(gpu, scs, 14, [5, 2, 3]), streams=[5, 2, 3])
    exp_full = sync.update_host(_frames(gpu, scs, 15))
    out = (gpu.CResult * (B + 2))()
    guard = (77, -3.5, -12345)

    def guarded(i):
        return (out[i].success, out[i].score, out[i].bbox.x) == guard

    for i in range(B + 2):
        out[i].success, out[i].score, out[i].bbox.x = guard
    assert L_.vt_group_wait_next(pipe._h, out, B + 2) == 0
    assert [_res(gpu.TrackResult(out[i])) for i in range(3)] == [_res(r) for r in exp]
    assert all(guarded(i) for i in range(3, B + 2))
    assert L_.vt_group_wait_next(pipe._h, out, B + 2) == 0
    assert [_res(gpu.TrackResult(out[i])) for i in range(B)] == [_res(r) for r in exp_full]
    assert all(guarded(i) for i in range(B, B + 2))
    for s in range(B):
        assert np.array_equal(_words(pipe, s), _words(sync, s))


# ---- 4. argument checks change nothing -----------------------------------------------------------------------------

def test_argument_checks_change_nothing(gpu, weights_tiny):
    """the bad-input table of the synchronous subset calls on vt_group_enqueue_host_streams, with two passes
    outstanding, and a third enqueue behind them: the status code of each, no state word, replay counter or capture
    count moved, and the outstanding passes still collect to the synchronous results"""
    L_ = gpu.lib()
    scs = _clips(gpu)
    pipe, sync = gpu.Group(weights_tiny, n_streams=B), gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, [pipe, sync], scs, streams=range(B - 1))          # stream 7 is never initialised
    L1, L2 = [4, 2, 0], [1, 2, 5, 6]
    pipe.enqueue_host(_frames(gpu, scs, 1, L1), streams=L1)
    pipe.enqueue_host(_frames(gpu, scs, 2, L2), streams=L2)
    keep = _frames(gpu, scs, 3)
    arr = (gpu.CFrame * (B + 1))(*[gpu.Group._host_frame(f)[0] for f in keep + [keep[0]]])

    def snapshot():
        return [_words(pipe, s) for s in range(B)], _replays(pipe), pipe.graph_captures(), pipe.host_redos()

    def ids(*v):
        return (ctypes.c_int32 * max(len(v), 1))(*v)

    def unchanged(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1:] == b[1:]

    before = snapshot()
    bad = [(ids(1, 1), 2), (ids(0, 8), 2), (ids(-1), 1), (ids(0), 0), (ids(*range(B), 0), B + 1), (None, 2)]
    for streams, n in bad:
        assert L_.vt_group_enqueue_host_streams(pipe._h, streams, arr, n) == INVALID, (list(streams or []), n)
        assert unchanged(snapshot(), before), (list(streams or []), n)
    assert L_.vt_group_enqueue_host_streams(pipe._h, ids(0, 1), None, 2) == INVALID
    assert L_.vt_group_enqueue_host_streams(None, ids(0), arr, 1) == INVALID
    assert L_.vt_group_enqueue_host_streams(pipe._h, ids(0, 7), arr, 2) == NOT_INIT
    assert unchanged(snapshot(), before)
    # a third pass behind two outstanding ones
    assert L_.vt_group_enqueue_host_streams(pipe._h, ids(0, 1), arr, 2) == INVALID
    assert b"vt_group_wait_next" in L_.vt_last_error()
    with pytest.raises(gpu.VtError) as ei:
        pipe.enqueue_host(_frames(gpu, scs, 3, [3]), streams=[3])
    assert ei.value.code == INVALID
    assert unchanged(snapshot(), before)
    got = [pipe.wait_next(), pipe.wait_next()]
    want = [sync.update_host(_frames(gpu, scs, 1, L1), streams=L1), sync.update_host(_frames(gpu, scs, 2, L2), streams=L2)]
    assert [[_res(r) for r in p] for p in got] == [[_res(r) for r in p] for p in want]
    for s in range(B):
        assert np.array_equal(_words(pipe, s), _words(sync, s))
    with pytest.raises(gpu.VtError):
        pipe.wait_next()                                              # nothing was enqueued by the refused calls


# ---- 5. queued init -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("margin_pct,expect_redo", [(0, False), (-1, True)])
def test_streams_join_through_queued_inits(gpu, weights_tiny, margin_pct, expect_redo):
    """streams 0..5 track pipelined; at frame 5 streams 6 (the group's first BGRX camera: its init captures the second
    graph set) and 7 are initialised behind the two outstanding passes and join; at frame 9 stream 2 leaves, at frame
    13 it is re-initialised on a new box and joins again. Frame by frame equal to a group that does init_host /
    update_host_streams at the same points; a queued init of a stream that is in an outstanding pass is refused; the
    full pass after the sequence finds every stream's template rows in place."""
    scs = _clips(gpu)
    n, t1, t2, t3 = 20, 5, 9, 13
    pipe = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=margin_pct)
    sync = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, [pipe, sync], scs, streams=range(6))

    def list_at(t):
        L = [0, 1, 2, 3, 4, 5] + ([6, 7] if t >= t1 else [])
        return [s for s in L if not (s == 2 and t2 <= t < t3)]

    def inits_at(t):
        joining = {t1: [6, 7], t3: [2]}.get(t, [])
        return [(s, _frame(gpu, scs[s], FMTS[s], t), gpu.BBox.new(*scs[s].gt_box(t))) for s in joining]

    refused = []

    def refusal(t, L):
        if t == t1 + 1:          # passes t1 and t1+1 are outstanding and both list stream 0
            before = [_words(pipe, s) for s in range(B)]
            with pytest.raises(gpu.VtError) as ei:
                pipe.enqueue_init_host(0, _frame(gpu, scs[0], FMTS[0], t), gpu.BBox.new(*scs[0].gt_box(t)))
            assert ei.value.code == INVALID and "vt_group_wait_next" in str(ei.value)
            assert all(np.array_equal(before[s], _words(pipe, s)) for s in range(B))
            refused.append(t)

    pass_at = lambda t: (list_at(t), _frames(gpu, scs, t, list_at(t)))
    caps = pipe.graph_captures()
    got = _pipelined(pipe, n, pass_at, inits_at, on_enqueued=refusal)
    want = _synchronous(sync, n, pass_at, inits_at)
    _assert_equal(got, want, {t: list_at(t) for t in range(1, n)})
    assert refused == [t1 + 1]
    assert pipe.graph_captures() == sync.graph_captures() > caps     # the BGRX stream's graph set, captured once
    assert (pipe.host_redos() > 0) == expect_redo, pipe.host_redos()
    for s in range(B):
        assert np.array_equal(_words(pipe, s), _words(sync, s)), f"state words of stream {s}"
    # restore_segments: the full pass needs every stream's template rows in its own segment, the joined ones' too
    full_p, full_s = pipe.update_host(_frames(gpu, scs, n)), sync.update_host(_frames(gpu, scs, n))
    assert [_res(r) for r in full_p] == [_res(r) for r in full_s]
    for s in range(B):
        assert np.array_equal(_words(pipe, s), _words(sync, s))
        assert np.array_equal(pipe.read_tensor("patches", s), sync.read_tensor("patches", s))


# ---- 6. registered host memory ---------------------------------------------------------------------------------------

def test_registered_frames_take_the_zero_copy_route(gpu, weights_tiny):
    """case 1 (default margin) with every frame in a vt_host_register pool and host_zero_copy = 1: equal to the
    synchronous group on the packed route"""
    scs = _clips(gpu)
    offs, total = {}, 0
    for s in range(B):
        for t in range(N):
            offs[(s, t)] = total
            total += (FRAME_BYTES[FMTS[s]] + 4095) & ~4095
    pool = np.zeros(total, np.uint8)
    hm = gpu.HostMapping(pool)
    try:
        frame_of = lambda s, t: _frame(gpu, scs[s], FMTS[s], t, into=pool[offs[(s, t)]:offs[(s, t)] + FRAME_BYTES[FMTS[s]]])
        pipe, sync = _varying_lists(gpu, weights_tiny, 0, zero_copy=1, frame_of=frame_of)
        assert pipe.host_redos() == 0
        pipe.close()
    finally:
        hm.close()


# ---- 7. closed loop at the headline model ----------------------------------------------------------------------------

def test_closed_loop_with_streams_joining_and_leaving_pipelined(gpu, capsys):
    """the pipelined twin of test_gpu_stream_subsets.py::test_closed_loop_with_streams_joining_and_leaving:
    traj_cfg3_300's clip on stream 0 of a 30-stream cfg3 group; every 3 frames the other streams of the list change -
    those that join are initialised by enqueue_init_host behind the two outstanding passes - so that the pass size
    runs between 1 and 30. Stream 0 meets the bars of its fixture AND every listed stream equals, bit for bit, the
    synchronous subset run with init_host at the same points."""
    name = "traj_cfg3_300.npz"
    fx, bar = _fixture(name), BARS[name]
    weights = gpu.weights.ensure_weights(str(fx["config"]))
    sc = _clip(gpu, fx)
    w, h, n, G = sc.w, sc.h, int(fx["frames"]), 30
    pipe, sync = gpu.Group(weights, n_streams=G), gpu.Group(weights, n_streams=G)
    rng = np.random.default_rng(11)
    sizes = [1, 30, 7, 19, 2, 29, 12, 1, 24, 4, 30, 16]
    lists, inits, seen, L = {}, {}, set(), []
    for t in range(n):
        inits[t] = []
        if t % 3 == 0:
            k = sizes[(t // 3) % len(sizes)]
            new = [0] + [int(s) for s in rng.choice(np.arange(1, G), k - 1, replace=False)]
            new = [int(s) for s in rng.permutation(new)]
            gx, gy, gw, gh = sc.gt_box(t)
            for s in sorted(set(new) - set(L) - {0}):
                inits[t].append((s, (gx + int(rng.integers(-12, 13)), gy + int(rng.integers(-12, 13)),
                                     gw + int(rng.integers(-8, 9)), gh + int(rng.integers(-8, 9)))))
            L = new
            seen.add(k)
        lists[t] = L
    inits[0].insert(0, (0, tuple(sc.gt_box(0))))
    assert {1, 30} <= seen
    frames = {}

    def frame(t):                       # both runs read the same object; frames of collected passes are dropped
        if t not in frames:
            frames[t] = gpu.NV12Frame(sc.frame_nv12(t), w, h)
            frames.pop(t - 4, None)
        return frames[t]

    got, want = {}, {}
    for t in range(n):                  # the two groups in step: one set of frames alive
        f = frame(t)
        for s, box in inits[t]:
            pipe.enqueue_init_host(s, f, gpu.BBox.new(*box))
            sync.init_host(s, f, gpu.BBox.new(*box))
        if t >= 2:
            got[t - 2] = pipe.wait_next()
        pipe.enqueue_host([f] * len(lists[t]), streams=lists[t])
        want[t] = sync.update_host([f] * len(lists[t]), streams=lists[t])
    got[n - 2], got[n - 1] = pipe.wait_next(), pipe.wait_next()
    _assert_equal(got, want, lists)
    res = [got[t][lists[t].index(0)] for t in range(n)]
    boxes = np.array([r.bbox for r in res])
    scores = np.array([r.score for r in res])
    succ = np.array([int(r.success) for r in res])
    d = np.abs(boxes - fx["bbox"])
    ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, fx["bbox"])])
    dscore = np.abs(scores - fx["score"])
    low = max(LOW_IOU_FRAMES[name])
    with capsys.disabled():
        print(f"\n[{name}, 30-stream group, pipelined, pass sizes {sorted(seen)}] {n} frames: max |delta| {d.max()} px, "
              f"IoU min {ious.min():.4f} mean {ious.mean():.5f}, frames below 0.99: {(ious < 0.99).sum()} (bar {low}), "
              f"max |delta score| {dscore.max():.4f}, redos {pipe.host_redos()}")
    assert d.max() <= bar["px"], f"max |delta| = {d.max()} px at frame {int(d.max(axis=1).argmax())}"
    assert ious.mean() >= bar["mean_iou"] and ious.min() >= bar["min_iou"]
    assert (ious < 0.99).sum() <= low
    assert np.array_equal(succ, fx["success"].astype(int)), "success flags differ"
    assert dscore.max() < 0.10


# ---- 8. threads ------------------------------------------------------------------------------------------------------

def test_two_groups_pipelining_subset_passes_on_two_threads(gpu, weights_tiny):
    """two groups, each on its own thread, each pipelining subset passes over its own lists: every result equals the
    group's single-threaded run"""
    scs = _clips(gpu)
    rngs = [np.random.default_rng(71), np.random.default_rng(72)]
    scheds = [{t: [int(s) for s in r.permutation(B)[:int(r.integers(1, B + 1))]] for t in range(1, N)} for r in rngs]
    for sched in scheds:
        for t in range(1, N):
            _frames(gpu, scs, t, sched[t])               # fill the pixel cache before the threads start

    def run(k, out, errs):
        try:
            g = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1 if k else 0)
            _init_all(gpu, [g], scs)
            got = _pipelined(g, N, lambda t: (scheds[k][t], _frames(gpu, scs, t, scheds[k][t])))
            out.extend([_res(r) for r in got[t]] for t in sorted(got))
            g.close()
        except Exception as e:          # surfaced by the assertion below
            errs.append(repr(e))

    refs, errs = [[], []], []
    for k in range(2):
        run(k, refs[k], errs)
    assert not errs, errs
    assert refs[0] != refs[1]
    outs = [[], []]
    th = [threading.Thread(target=run, args=(k, outs[k], errs)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    assert outs[0] == refs[0] and outs[1] == refs[1]
