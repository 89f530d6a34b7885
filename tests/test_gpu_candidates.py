"""Candidate passes (vt_group_update_*_candidates): several search windows per stream, the best one committed.

A pass whose slots are (stream, optional box) pairs; a stream may fill several slots, each a complete, independent
update around the slot's box; the device picks every stream's best slot and commits only that one. Checked here on
the MI355X:
  * every slot's result and head output are BIT-identical to those of a fresh n-stream group given the same template,
    box and frame; the winner is the rule's; the stream's state is the winner's, with one update counted and the box
    left alone when the winner failed;
  * a list of distinct streams without boxes IS the subset pass; unlisted streams are untouched; the next full pass
    finds the template rows back in place;
  * the host form (shared frames staged once, zero-copy route included) equals the device form; bad input changes
    nothing; no graph is captured inside an update;
  * re-acquisition against the committed oracle scan (tests/golden/reacquire_cfg{2,3}.npz) beside 29 tracking streams."""
import ctypes
import math
import os

import numpy as np
import pytest

from test_gpu_stream_subsets import (B, FRAMES_DONE, H, INVALID, NOT_INIT, SUCCESS_COUNT, W, _clips, _dev, _frames_at,
                                     _init_all, _replays, _res, _words)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rule(results, streams):
    """winner[i] by the header's rule, from the slots' results: greatest score, NaN loses, lowest slot on a tie"""
    win = []
    for s in streams:
        best = None
        for j, (r, sj) in enumerate(zip(results, streams)):
            if sj != s:
                continue
            if best is None:
                best = j
                continue
            a, b = r.score, results[best].score
            if (not math.isnan(a)) and (math.isnan(b) or a > b):
                best = j
        win.append(best)
    return win


def _box_of(words):
    return words[0:4].view(np.float32).copy()


def _shift(box, dx, dy, dw=0.0, dh=0.0):
    return [float(box[0]) + dx, float(box[1]) + dy, float(box[2]) + dw, float(box[3]) + dh]


FAR = [4.0, 4.0, 40.0, 40.0]          # a corner of the frame: background only


def _schedule(boxes):
    """candidate lists of an 8-stream group as (stream, box or None); boxes[s]: stream s's state box before the pass.
    Repeats of one stream, two scanning streams beside tracking ones, a full 8-slot scan, lists with and without
    boxes, an all-failing stream (FAR windows) and the same frame and box twice (bit-equal scores)."""
    b = boxes
    return [
        [(2, None), (2, _shift(b[2], 6, -4)), (2, _shift(b[2], -10, 8))],
        [(5, _shift(b[5], 3, 3)), (1, None), (5, _shift(b[5], 3, 3)), (0, None)],                    # slots 0 and 2: equal scores
        [(3, FAR), (3, _shift(FAR, 30, 10)), (6, None), (3, _shift(FAR, 0, 40)), (7, None)],           # stream 3: every slot fails
        [(4, _shift(b[4], dx, dy)) for dx in (-24, 0, 24) for dy in (-16, 16)] + [(4, None), (4, _shift(b[4], 0, 0, 6, -4))],
        [(0, None), (1, _shift(b[1], -8, 0)), (1, _shift(b[1], 8, 0)), (2, None), (6, _shift(b[6], 0, 12)), (6, _shift(b[6], 0, -12)),
         (6, None)],
        [(7, _shift(b[7], 5, 5))],
        [(1, None), (1, None)],                                                                        # no boxes, one stream twice
        [(0, _shift(b[0], 12, 0)), (3, None), (0, _shift(b[0], -12, 0)), (5, None), (0, FAR), (4, None), (2, None), (0, None)],
        [(6, FAR), (6, FAR)],                                                                          # equal AND failing
        [(3, _shift(b[3], 0, 0)), (2, _shift(b[2], 2, 2, 4, 4)), (3, _shift(b[3], 14, -14)), (7, None), (1, None)],
        [(5, None), (5, _shift(b[5], -20, -20)), (4, _shift(b[4], 20, 20)), (4, None)],
    ]


@pytest.mark.parametrize("cfg", ["tiny", "cfg3"])
def test_candidate_pass_is_bit_identical_to_an_engine_of_that_size(gpu, cfg, capsys):
    """Every pass of the schedule against a fresh n-stream group: stream j holds slot j's stream's template and has its
    box set to the slot's box. Slot results and head outputs equal; the winner is the rule's; the stream's state equals
    the reference winner's but for its own history (one more update, the winner's success) and, where the winner
    failed, the box - which stays what it was before the pass."""
    weights = gpu.weights.ensure_weights(cfg)
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    grp = gpu.Group(weights, n_streams=B)
    _init_all(gpu, grp, frames0, scs)
    caps = grp.graph_captures()
    failing_winner = tie_seen = 0
    n_passes = len(_schedule([np.zeros(4)] * B))
    assert n_passes >= 10
    for p in range(n_passes):
        frames, keep = _frames_at(gpu, scs, p + 1)
        before = [_words(grp, s) for s in range(B)]
        cands = _schedule([_box_of(w) for w in before])[p]
        streams = [c[0] for c in cands]
        slot_frames = [frames[s] for s in streams]
        res, win = grp.update_device_candidates(cands, slot_frames)
        after = [_words(grp, s) for s in range(B)]
        n = len(cands)
        small = gpu.Group(weights, n_streams=n)
        for j, (s, box) in enumerate(cands):
            small.init_device(j, frames0[s], gpu.BBox.new(*scs[s].gt_box(0)))
            small.set_state_box(j, box if box is not None else _box_of(before[s]))
        ref = small.update_device(slot_frames)
        for j in range(n):
            assert _res(res[j]) == _res(ref[j]), f"pass {p} slot {j}: {res[j]} vs {ref[j]}"
            assert np.array_equal(grp.read_tensor("slot.head_out", j).view(np.uint32),
                                  small.read_tensor("head_out", j).view(np.uint32)), f"pass {p} slot {j}: head_out"
        assert win == _rule(ref, streams), f"pass {p}: winners {win}"
        for s in set(range(B)) - set(streams):
            assert np.array_equal(before[s], after[s]), f"pass {p}: stream {s} (not listed) changed"
        for s in set(streams):
            w = win[streams.index(s)]
            assert all(win[j] == w for j in range(n) if streams[j] == s)
            got, exp = after[s].copy(), _words(small, w)
            assert got[FRAMES_DONE] == before[s][FRAMES_DONE] + 1, f"pass {p}: stream {s} counts one update"
            assert got[SUCCESS_COUNT] == before[s][SUCCESS_COUNT] + int(ref[w].success)
            got[[FRAMES_DONE, SUCCESS_COUNT]] = exp[[FRAMES_DONE, SUCCESS_COUNT]]
            if not ref[w].success:
                failing_winner += 1
                assert np.array_equal(got[0:4], before[s][0:4]), f"pass {p}: stream {s} failed, its box moved"
                got[0:4] = exp[0:4]
            assert np.array_equal(got, exp), f"pass {p}: state of stream {s}"
            # the stream's per-pass tensors are its winning slot's
            assert np.array_equal(grp.read_tensor("head_out", s).view(np.uint32), small.read_tensor("head_out", w).view(np.uint32))
            ties = [j for j in range(n) if streams[j] == s and j != w and _res(ref[j])[2] == _res(ref[w])[2]]
            if ties:
                tie_seen += 1
                assert w < min(ties), f"pass {p}: equal scores, slot {w} won over {ties}"
        small.close()
    with capsys.disabled():
        print(f"\n[candidates {cfg}] {n_passes} passes: {failing_winner} failing winners, {tie_seen} ties")
    assert failing_winner >= 1 and tie_seen >= 1
    assert grp.graph_captures() == caps
    grp.close()


def test_distinct_streams_without_boxes_are_the_subset_pass(gpu, weights_tiny):
    """results and every state word of update_device(..., streams=L) on a twin group; the identity list replays the graph"""
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    a, b = gpu.Group(weights_tiny, n_streams=B), gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, a, frames0, scs)
    _init_all(gpu, b, frames0, scs)
    caps = a.graph_captures()
    for t, L in enumerate([[5, 2, 7], list(range(B)), [0], [7, 6, 5, 4, 3, 2, 1, 0], list(range(B)), [3, 1]], start=1):
        frames, keep = _frames_at(gpu, scs, t)
        r0 = _replays(a)
        ra, win = a.update_device_candidates(L, [frames[s] for s in L])
        rb = b.update_device([frames[s] for s in L], streams=L)
        assert [_res(r) for r in ra] == [_res(r) for r in rb] and win == list(range(len(L)))
        assert _replays(a) == r0 + (1 if L == list(range(B)) else 0)
        for s in range(B):
            assert np.array_equal(_words(a, s), _words(b, s)), (L, s)
        assert np.array_equal(a.read_tensor("head_out", L[-1]), b.read_tensor("head_out", L[-1]))
    assert a.graph_captures() == caps


def test_unlisted_streams_keep_every_state_word(gpu, weights_tiny):
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    grp = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, grp, frames0, scs, streams=range(6))          # streams 6, 7 are never initialised and never listed
    caps = grp.graph_captures()
    rng = np.random.default_rng(5)
    done = np.zeros(B, int)
    for t in range(1, 13):
        frames, keep = _frames_at(gpu, scs, t)
        n = int(rng.integers(1, B + 1))
        streams = [int(s) for s in rng.integers(0, 6, n)]
        before = [_words(grp, s) for s in range(B)]
        cands = [(s, None if rng.random() < 0.3 else _shift(_box_of(before[s]), *rng.integers(-20, 21, 2))) for s in streams]
        grp.update_device_candidates(cands, [frames[s] for s in streams])
        for s in range(B):
            w = _words(grp, s)
            if s in streams:
                done[s] += 1
                assert w[FRAMES_DONE] == done[s]
            else:
                assert np.array_equal(w, before[s]), f"t={t} {streams}: stream {s} changed"
    assert grp.graph_captures() == caps


@pytest.mark.parametrize("use_graph", [True, False])
def test_full_pass_after_a_candidate_pass_restores_the_templates(gpu, weights_tiny, use_graph):
    """A: init 8, a candidate pass in which stream 3 fills three slots, then a full pass. B: the same init, then the full
    pass. Every stream but 3 gives bit-identical results - which fails if the first segments of the patch matrix still
    hold stream 3's template."""
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    frames1, keep1 = _frames_at(gpu, scs, 1)
    frames2, keep2 = _frames_at(gpu, scs, 2)
    a = gpu.Group(weights_tiny, n_streams=B, use_graph=use_graph)
    b = gpu.Group(weights_tiny, n_streams=B, use_graph=use_graph)
    _init_all(gpu, a, frames0, scs)
    _init_all(gpu, b, frames0, scs)
    caps = a.graph_captures()
    box = _box_of(_words(a, 3))
    a.update_device_candidates([(3, _shift(box, 5, 0)), (3, None), (3, _shift(box, -5, 0))], [frames1[3]] * 3)
    ra, rb = a.update_device(frames2), b.update_device(frames2)
    for s in range(B):
        if s != 3:
            assert _res(ra[s]) == _res(rb[s]), f"stream {s}: {ra[s]} vs {rb[s]}"
            assert np.array_equal(_words(a, s), _words(b, s))
            assert np.array_equal(a.read_tensor("patches", s), b.read_tensor("patches", s))
    assert _words(a, 3)[FRAMES_DONE] == 2 and _words(b, 3)[FRAMES_DONE] == 1
    assert a.graph_captures() == caps


# ---- host frames ----------------------------------------------------------------------------------------------------

def _nv21(buf, w, h):
    out = buf.copy()
    uv = out[w * h:].reshape(-1, 2)
    uv[:] = uv[:, ::-1]
    return out


@pytest.mark.parametrize("fmt", ["nv12", "nv21"])
@pytest.mark.parametrize("zero_copy", [-1, 1])
def test_host_candidates_equal_device_candidates(gpu, weights_tiny, fmt, zero_copy):
    """update_host_candidates gives bit for bit what update_device_candidates gives on the same pixels: slots repeated
    on ONE shared host frame (staged once, as the bounding rectangle of their windows) and on distinct copies of it,
    NV12 and a format of the any-layout crop kernels, packed (-1) and, from vt_host_register'ed memory, zero-copy (1):
    there the frames read through the mapping as device frames give the same again."""
    import torch
    scs = _clips(gpu)
    T = 5
    conv = (lambda b: b) if fmt == "nv12" else (lambda b: _nv21(b, W, H))
    clip = np.stack([np.stack([conv(sc.frame_nv12(t)) for t in range(T)]) for sc in scs])      # [B, T, bytes]
    fb = clip.shape[2]
    HostF = gpu.NV12Frame if fmt == "nv12" else gpu.NV21Frame
    devf = gpu.frame_nv12 if fmt == "nv12" else gpu.frame_nv21
    dclip = torch.from_numpy(clip).cuda()

    def dev(s, t):
        p = dclip.data_ptr() + (s * T + t) * fb
        return devf(p, p + W * H, W, H)

    def host(s, t, copy=False):
        return HostF(clip[s, t].copy() if copy else clip[s, t], W, H)     # not copied: a view into `clip` (the registered range)

    hm = gpu.HostMapping(clip) if zero_copy == 1 else None
    try:
        hd = gpu.Group(weights_tiny, n_streams=B, host_zero_copy=zero_copy)
        dv = gpu.Group(weights_tiny, n_streams=B)
        vm = gpu.Group(weights_tiny, n_streams=B) if hm else None
        for s in range(B):
            hd.init_host(s, host(s, 0), gpu.BBox.new(*scs[s].gt_box(0)))
            dv.init_device(s, dev(s, 0), gpu.BBox.new(*scs[s].gt_box(0)))
            if vm:
                p = hm.d_ptr + (s * T) * fb
                vm.init_device(s, devf(p, p + W * H, W, H), gpu.BBox.new(*scs[s].gt_box(0)))
        caps = hd.graph_captures()
        for t in range(1, T):
            bx = [_box_of(_words(dv, s)) for s in range(B)]
            lists = {
                1: [(2, _shift(bx[2], -30, -20)), (2, None), (2, _shift(bx[2], 30, 20)), (5, None), (2, _shift(bx[2], 0, 40))],
                2: [(s, _shift(bx[s], 8, 8)) for s in (0, 0, 7, 7, 7)] + [(3, None)],
                3: [(4, _shift(bx[4], dx, dy)) for dx in (-40, 40) for dy in (-40, 40)] + [(1, None), (6, None), (4, FAR), (4, None)],
                4: [(6, None), (1, None), (3, None)],
            }[t]
            streams = [c[0] for c in lists]
            shared = {s: host(s, t) for s in set(streams)}
            # t odd: repeated slots share one host frame object; t even: every slot brings a copy of its own
            hf = [shared[s] if t % 2 else host(s, t, copy=zero_copy != 1) for s in streams]
            rh, wh = hd.update_host_candidates(lists, hf)
            rd, wd = dv.update_device_candidates(lists, [dev(s, t) for s in streams])
            assert [_res(r) for r in rh] == [_res(r) for r in rd], (t, rh, rd)
            assert wh == wd
            if vm:
                rv, wv = vm.update_device_candidates(lists, [devf(hm.d_ptr + (s * T + t) * fb, hm.d_ptr + (s * T + t) * fb + W * H, W, H)
                                                             for s in streams])
                assert [_res(r) for r in rv] == [_res(r) for r in rd] and wv == wd
            for s in range(B):
                assert np.array_equal(_words(hd, s), _words(dv, s)), (t, s)
        assert hd.graph_captures() == caps
    finally:
        if hm:
            hm.close()


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_argument_checks_change_nothing(gpu, weights_tiny):
    """every refusal of the header: the status code, no state word of any stream changed, no result written; refused
    while a pipelined pass is outstanding, accepted after wait_next"""
    L_ = gpu.lib()
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    frames1, keep1 = _frames_at(gpu, scs, 1)
    grp = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, grp, frames0, scs, streams=range(7))           # stream 7 is never initialised
    last, _ = grp.update_device_candidates([(4, None), (4, [200, 200, 50, 50])], [frames1[4]] * 2)
    arr = (gpu.CFrame * (B + 1))(*(list(frames1) + [frames1[0]]))
    host1 = [gpu.NV12Frame(sc.frame_nv12(1), W, H) for sc in scs]
    harr = (gpu.CFrame * (B + 1))(*([gpu.Group._host_frame(f)[0] for f in host1] + [gpu.Group._host_frame(host1[0])[0]]))
    SENT = 0x5a5a5a5a

    def fresh():
        out, win = (gpu.CResult * (B + 1))(), (ctypes.c_int32 * (B + 1))()
        ctypes.memset(out, 0x5a, ctypes.sizeof(out))
        ctypes.memset(win, 0x5a, ctypes.sizeof(win))
        return out, win

    def untouched(out, win):
        return bytes(out) == b"\x5a" * ctypes.sizeof(out) and all(v == SENT for v in win)

    def snapshot():
        return [_words(grp, s) for s in range(B)], _replays(grp), grp.graph_captures()

    def cands(*items):
        return gpu.Group._cands(list(items))

    nan, inf = float("nan"), float("inf")
    null_frame = gpu.CFrame(None, None, W, H, W, W, gpu.PIX_NV12, 0, 0, 0, 0, 0)
    bad_frame, bad_host = (gpu.CFrame * 2)(arr[0], null_frame), (gpu.CFrame * 2)(harr[0], null_frame)
    before = snapshot()
    invalid = [(cands(0, 8), arr, 2), (cands(-1), arr, 1), (cands(0), arr, 0), (cands(*([0] * (B + 1))), arr, B + 1),
               (cands(0, 1), bad_frame, 2),
               (cands((0, [nan, 10, 50, 50])), arr, 1), (cands((0, [10, 10, inf, 50])), arr, 1),
               (cands((0, [10, 10, 0.5, 50])), arr, 1), (cands((0, [10, 10, 50, 40000])), arr, 1),
               (cands((0, [70000, 10, 50, 50])), arr, 1), (cands((0, [10, -70000, 50, 50])), arr, 1),
               (cands(1, (0, [10, 10, 50, -1])), arr, 2)]
    for fn, frames_of in ((L_.vt_group_update_device_candidates, lambda a: a),
                          (L_.vt_group_update_host_candidates, lambda a: harr if a is arr else bad_host)):
        for c, fr, n in invalid:
            out, win = fresh()
            assert fn(grp._h, c, frames_of(fr), n, out, win) == INVALID, (fn.__name__, n, [(x.stream, list(x.box)) for x in c])
            assert untouched(out, win)
        out, win = fresh()
        assert fn(grp._h, None, frames_of(arr), 1, out, win) == INVALID
        assert fn(grp._h, cands(0), None, 1, out, win) == INVALID
        assert fn(grp._h, cands(0), frames_of(arr), 1, None, win) == INVALID
        assert fn(None, cands(0), frames_of(arr), 1, out, win) == INVALID
        assert fn(grp._h, cands(0, 7), frames_of(arr), 2, out, win) == NOT_INIT
        assert fn(grp._h, cands((7, [10, 10, 50, 50]), (7, None)), frames_of(arr), 2, out, win) == NOT_INIT
        assert untouched(out, win)
    now = snapshot()
    assert all(np.array_equal(x, y) for x, y in zip(now[0], before[0])) and now[1:] == before[1:]
    assert [_res(r) for r in grp.wait()] == [_res(r) for r in last]
    # a null winner table is allowed
    out, _ = fresh()
    assert L_.vt_group_update_device_candidates(grp._h, cands(0, (0, [100, 100, 50, 50])), arr, 2, out, None) == 0
    # a pipelined host pass owns the states until it is collected
    L7 = list(range(7))
    grp.enqueue_host([host1[s] for s in L7], streams=L7)
    mid = snapshot()
    out, win = fresh()
    assert L_.vt_group_update_device_candidates(grp._h, cands(0, 0), arr, 2, out, win) == INVALID
    assert L_.vt_group_update_host_candidates(grp._h, cands(0, 0), harr, 2, out, win) == INVALID
    assert untouched(out, win)
    assert len(grp.wait_next()) == 7
    res, w = grp.update_host_candidates([(0, None), (0, [100, 100, 50, 50])], [host1[0]] * 2)
    assert len(res) == 2 and w[0] == w[1] and _words(grp, 0)[FRAMES_DONE] == mid[0][0][FRAMES_DONE] + 1
    assert grp.graph_captures() == before[2]


# ---- re-acquisition against the oracle -------------------------------------------------------------------------------

def _reacquire_fixture(gpu, cfg):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_reacquire", os.path.join(ROOT, "tests", "golden", "make_reacquire.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with np.load(os.path.join(ROOT, "tests", "golden", f"reacquire_{cfg}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    assert gen.sha256_file(gpu.weights.ensure_weights(cfg)) == str(fx["weights_sha256"]), "fixture made with other weights"
    return gen, fx


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_reacquisition_follows_the_oracle_scan(gpu, cfg, host, capsys):
    """The fixture clip on stream 0 of a 30-stream group: frames 0-2 tracked, the target then jumps ~550 px. The plain
    update on frame 3 fails like the oracle's; Group.reacquire scans the frame in 30-slot chunks and finds the target
    in the oracle's stop chunk, slot for slot as the oracle scored the windows; 20 closed-loop frames follow the
    oracle's. The 29 other streams track clips of their own throughout - on frame 3 in ONE mixed candidate pass with
    the lost stream - and give what a twin group gives that ran subset passes of the same sizes and never scanned."""
    gen, fx = _reacquire_fixture(gpu, cfg)
    weights = gpu.weights.ensure_weights(cfg)
    w, h, G, jump = int(fx["frame_w"]), int(fx["frame_h"]), 30, int(fx["jump_at"])
    assert int(fx["chunk"]) == G
    frame0, gt0 = gen.clip()
    others = [gpu.synth.MovingSquare(w, h, 56 + 2 * (i % 9), seed=100 + i) for i in range(1, G)]
    L = list(range(1, G)) + [0]                 # stream 0 in the last slot: a subset pass of all 30, not the identity
    grp = gpu.Group(weights, n_streams=G)
    twin = gpu.Group(weights, n_streams=G)
    caps = grp.graph_captures()
    twin_sc0 = gpu.synth.MovingSquare(w, h, int(fx["square"]), seed=0)      # the clip without the jump

    def frames_at(t):
        """per stream: (frame for the group's entry points, keep-alive); stream 0 first"""
        bufs = [frame0(t)] + [sc.frame_nv12(t) for sc in others]
        if host:
            return [gpu.NV12Frame(b, w, h) for b in bufs], gpu.NV12Frame(twin_sc0.frame_nv12(t), w, h), None
        pairs = [_dev(gpu, b, w, h) for b in bufs]
        t0 = _dev(gpu, twin_sc0.frame_nv12(t), w, h)
        return [p[0] for p in pairs], t0[0], (pairs, t0)

    def subset(g, fr):
        return g.update_host(fr, streams=L) if host else g.update_device(fr, streams=L)

    def check_others(ra, rb, t):
        assert [_res(r) for r in ra[:G - 1]] == [_res(r) for r in rb[:G - 1]], f"frame {t}: the tracking streams differ from the twin's"

    dscore_ok = dscore_fail = 0.0
    for t in range(jump + 1 + 20):
        fr, tw0, keep = frames_at(t)
        if t == 0:
            for g, f0 in ((grp, fr[0]), (twin, tw0)):
                init = g.init_host if host else g.init_device
                init(0, f0, gpu.BBox.new(*gt0(0)))
                for i, sc in enumerate(others, start=1):
                    init(i, fr[i], gpu.BBox.new(*sc.gt_box(0)))
        lf = [fr[s] for s in L]
        rb = subset(twin, lf[:-1] + [tw0])
        if t != jump:
            ra = subset(grp, lf)
            check_others(ra, rb, t)
            r0 = ra[-1]
            if t < jump:
                exp_box, exp_score, exp_succ = fx["pre_bbox"][t], fx["pre_score"][t], fx["pre_success"][t]
            else:
                k = t - jump - 1
                exp_box, exp_score, exp_succ = fx["track_bbox"][k], fx["track_score"][k], fx["track_success"][k]
            assert np.abs(np.array(r0.bbox) - exp_box).max() <= 1, f"frame {t}: {r0} vs oracle {exp_box}"
            assert bool(r0.success) == bool(exp_succ), f"frame {t}: {r0}"
            if t < jump:
                assert abs(r0.score - exp_score) < 0.03, f"frame {t}: {r0} vs oracle score {exp_score}"
            continue
        # frame 3: ONE mixed candidate pass - 29 tracking slots without a box and the lost stream's slot with a box (its
        # own state box, spelt out: the plain update) - then the scan
        state0 = _words(grp, 0)
        cands = [(s, None) for s in L[:-1]] + [(0, _box_of(state0))]
        fn = grp.update_host_candidates if host else grp.update_device_candidates
        ra, win = fn(cands, lf)
        assert win == list(range(G))
        check_others(ra, rb, t)
        plain = ra[-1]
        assert not plain.success and abs(plain.score - float(fx["plain_score"])) < 0.03, f"plain update {plain}"
        assert np.array_equal(_words(grp, 0)[0:4], state0[0:4])
        bw, bh = float(fx["state_before"][2]), float(fx["state_before"][3])
        assert np.abs(gpu.scan_windows(w, h, bw, bh) - fx["boxes"]).max() <= 1e-3
        done = _words(grp, 0)[FRAMES_DONE]
        best = grp.reacquire(0, fr[0], box_wh=(bw, bh), host=host)
        scan = grp.last_scan
        stop = int(fx["stop_chunk"])
        assert len(scan) == stop + 1, f"{len(scan)} chunks scanned, the oracle stops in chunk {stop}"
        assert _words(grp, 0)[FRAMES_DONE] == done + stop + 1          # each chunk is one update of the stream
        for c, (res, cw) in enumerate(scan):
            o_score = fx["slot_score"][c * G:(c + 1) * G]
            o_succ = fx["slot_success"][c * G:(c + 1) * G]
            assert len(res) == len(o_score) and all(v == cw[0] for v in cw)
            assert bool(res[cw[0]].success) == (c == stop), f"chunk {c}: winner {res[cw[0]]}"
            assert [bool(r.success) for r in res] == [bool(v) for v in o_succ], f"chunk {c}: success flags"
            assert cw == _rule(res, [0] * len(res))
            for r, osc, ok in zip(res, o_score, o_succ):
                d = abs(r.score - float(osc))
                if ok:
                    dscore_ok = max(dscore_ok, d)
                else:
                    dscore_fail = max(dscore_fail, d)
        with capsys.disabled():
            print(f"\n[reacquire {cfg} {'host' if host else 'device'}] max |score - oracle|: succeeding slots {dscore_ok:.5f}, "
                  f"failing slots {dscore_fail:.5f}; winner {best}")
        assert max(dscore_ok, dscore_fail) < 0.03
        o_score = fx["slot_score"][stop * G:(stop + 1) * G]
        hw = scan[stop][1][0]
        assert o_score[hw] >= o_score.max() - 0.06, f"winner slot {hw}: oracle score {o_score[hw]} vs best {o_score.max()}"
        o_win = int(fx["chunk_winner"][stop])
        assert np.abs(np.array(best.bbox) - fx["slot_bbox"][o_win]).max() <= 1, f"{best} vs oracle {fx['slot_bbox'][o_win]}"
        assert best.success and _res(best) == _res(scan[stop][0][hw])
        assert np.array_equal(_box_of(_words(grp, 0)), np.array(best.bbox, np.float32))
    assert grp.graph_captures() == caps and twin.graph_captures() == caps
