"""Passes over a chosen subset of a group's streams (vt_group_*_streams).

A multi-camera host updates only the cameras that are tracking (src/tracker_context.rs:88-90,120); a group pass over
streams[0..n) runs the full pass's kernels on n compacted slots. Checked here on the MI355X:
  * every listed stream's results and state are BIT-identical to those of a fresh n-stream group given the same
    template, box and frame (same M, same kernels, rows independent: nothing else is correct);
  * streams that are not listed are untouched, need not be initialised, and a full pass after a subset pass finds
    every stream's template rows back in place;
  * the host path equals the device path, no graph is captured inside an update, bad input changes nothing;
  * one stream of a 30-stream cfg3 group whose pass size varies between 1 and 30 meets the closed-loop bars of its
    committed oracle trajectory."""
import ctypes
import struct

import numpy as np
import pytest

from conftest import iou
from test_gpu_trajectories import BARS, LOW_IOU_FRAMES, _clip, _fixture

pytestmark = pytest.mark.gpu

W, H, B = 640, 480, 8
INVALID, NOT_INIT = -1, -6


def _clips(gpu, n=B):
    return [gpu.synth.MovingSquare(W, H, 48 + 4 * i, seed=20 + i) for i in range(n)]


def _dev(gpu, buf, w=W, h=H):
    """(device NV12 frame, keep-alive tensor)"""
    import torch
    d = torch.from_numpy(buf).cuda()
    return gpu.frame_nv12(d.data_ptr(), d.data_ptr() + w * h, w, h), d


def _frames_at(gpu, scs, t):
    pairs = [_dev(gpu, sc.frame_nv12(t)) for sc in scs]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def _words(g, s):
    return g.read_tensor("state", s).view(np.uint32).copy()


def _res(r):
    """a result as exact bits: box, success flag, score's float32 pattern"""
    return tuple(r.bbox), int(r.success), struct.unpack("<I", struct.pack("<f", r.score))[0]


def _replays(g):
    return int(g.read_tensor("graph_replays").sum())


def _init_all(gpu, g, frames0, scs, streams=None):
    for s in (range(len(scs)) if streams is None else streams):
        g.init_device(s, frames0[s], gpu.BBox.new(*scs[s].gt_box(0)))


SCHEDULE = [[5, 2, 7], [0], [7, 6, 5, 4, 3, 2, 1], [3, 1], [1, 4, 6, 0, 2], [0, 1, 2, 3, 4, 5, 6, 7], [6],
            [7, 6, 5, 4, 3, 2, 1, 0], [2, 0], [4, 7, 1]]
FRAMES_DONE, SUCCESS_COUNT = 11, 12       # StreamState words that count the stream's own history


@pytest.mark.parametrize("cfg", ["tiny", "cfg3"])
def test_subset_pass_is_bit_identical_to_an_engine_of_that_size(gpu, cfg):
    """Every pass of SCHEDULE against a fresh group of n streams holding the same templates (init on the same frame and
    box) and the same crop boxes (vt_group_set_state_box with the big group's box before the pass): results and state
    words equal; frames_done / success_count, which count the stream's own history, advance by one pass. Streams not
    listed keep every state word."""
    weights = gpu.weights.ensure_weights(cfg)
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    grp = gpu.Group(weights, n_streams=B)
    _init_all(gpu, grp, frames0, scs)
    for p, L in enumerate(SCHEDULE):
        frames, keep = _frames_at(gpu, scs, p + 1)
        before = [_words(grp, s) for s in range(B)]
        res = grp.update_device([frames[s] for s in L], streams=L)
        assert len(res) == len(L)
        after = [_words(grp, s) for s in range(B)]
        for s in set(range(B)) - set(L):
            assert np.array_equal(before[s], after[s]), f"pass {L}: stream {s} (not listed) changed"
        small = gpu.Group(weights, n_streams=len(L))
        for j, s in enumerate(L):
            small.init_device(j, frames0[s], gpu.BBox.new(*scs[s].gt_box(0)))
            small.set_state_box(j, before[s][0:4].view(np.float32))
        ref = small.update_device([frames[s] for s in L])
        for j, s in enumerate(L):
            assert _res(res[j]) == _res(ref[j]), f"pass {L}: stream {s} (slot {j}) {res[j]} vs {ref[j]}"
            got, exp = after[s].copy(), _words(small, j)
            assert got[FRAMES_DONE] == before[s][FRAMES_DONE] + 1
            assert got[SUCCESS_COUNT] == before[s][SUCCESS_COUNT] + int(res[j].success)
            got[[FRAMES_DONE, SUCCESS_COUNT]] = exp[[FRAMES_DONE, SUCCESS_COUNT]]
            assert np.array_equal(got, exp), f"pass {L}: state of stream {s}"
            # per-pass tensors are those of the stream's slot
            assert np.array_equal(grp.read_tensor("head_out", s).view(np.uint32), small.read_tensor("head_out", j).view(np.uint32))
        small.close()
        if len(L) < B:
            with pytest.raises(gpu.VtError) as ei:
                grp.read_tensor("head_out", (set(range(B)) - set(L)).pop())
            assert ei.value.code == INVALID
    grp.close()


def test_streams_not_listed_are_untouched(gpu, weights_tiny):
    """state words, host-visible results and pass count of every unlisted stream stay as they were over a run of
    subset passes; the listed ones advance by exactly one pass each"""
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    grp = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, grp, frames0, scs)
    done = np.zeros(B, int)
    rng = np.random.default_rng(3)
    for t in range(1, 13):
        frames, keep = _frames_at(gpu, scs, t)
        L = [int(s) for s in rng.permutation(B)[:int(rng.integers(1, B))]]
        before = [_words(grp, s) for s in range(B)]
        grp.update_device([frames[s] for s in L], streams=L)
        for s in range(B):
            w = _words(grp, s)
            if s in L:
                done[s] += 1
                assert w[FRAMES_DONE] == done[s]
            else:
                assert np.array_equal(w, before[s]), f"t={t} pass {L}: stream {s} changed"


@pytest.mark.parametrize("use_graph", [True, False])
def test_full_pass_after_a_subset_pass_restores_the_templates(gpu, weights_tiny, use_graph):
    """A: init 8, a pass over [3] alone, then a full pass. B: the same init, then the full pass. Every stream but 3 gives
    bit-identical results in A and B - which fails if segment 0 of the patch matrix still holds stream 3's template."""
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    frames1, keep1 = _frames_at(gpu, scs, 1)
    frames2, keep2 = _frames_at(gpu, scs, 2)
    a = gpu.Group(weights_tiny, n_streams=B, use_graph=use_graph)
    b = gpu.Group(weights_tiny, n_streams=B, use_graph=use_graph)
    _init_all(gpu, a, frames0, scs)
    _init_all(gpu, b, frames0, scs)
    a.update_device([frames1[3]], streams=[3])
    ra, rb = a.update_device(frames2), b.update_device(frames2)
    for s in range(B):
        if s != 3:
            assert _res(ra[s]) == _res(rb[s]), f"stream {s}: {ra[s]} vs {rb[s]}"
            assert np.array_equal(_words(a, s), _words(b, s))
            assert np.array_equal(a.read_tensor("patches", s), b.read_tensor("patches", s))
    assert _words(a, 3)[FRAMES_DONE] == 2 and _words(b, 3)[FRAMES_DONE] == 1


def test_uninitialised_streams_may_sit_out(gpu, weights_tiny):
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    frames1, keep1 = _frames_at(gpu, scs, 1)
    grp = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, grp, frames0, scs, streams=range(5))
    L = [0, 1, 2, 3, 4]
    res = grp.update_device([frames1[s] for s in L], streams=L)
    assert len(res) == len(L) and all(_words(grp, s)[FRAMES_DONE] == 1 for s in L)
    before = [_words(grp, s) for s in range(B)]
    with pytest.raises(gpu.VtError) as ei:
        grp.update_device([frames1[0], frames1[6]], streams=[0, 6])
    assert ei.value.code == NOT_INIT
    with pytest.raises(gpu.VtError) as ei:
        grp.enqueue_device([frames1[6]], streams=[6])
    assert ei.value.code == NOT_INIT
    assert all(np.array_equal(before[s], _words(grp, s)) for s in range(B))
    with pytest.raises(gpu.VtError) as ei:        # the full pass still needs every stream
        grp.update_device(frames1)
    assert ei.value.code == NOT_INIT
    assert all(np.array_equal(before[s], _words(grp, s)) for s in range(B))
    assert [_res(r) for r in grp.wait()] == [_res(r) for r in res]


@pytest.mark.parametrize("fmt", ["nv12", "rgb8"])
def test_host_streams_equal_device_streams(gpu, weights_tiny, fmt):
    """update_host_streams (windows cut around each listed stream's own box, packed, one upload) gives bit for bit what
    update_device_streams gives on the same frames"""
    import torch
    scs = _clips(gpu)
    hd, dv = gpu.Group(weights_tiny, n_streams=B), gpu.Group(weights_tiny, n_streams=B)
    keep = []

    def frames(t):
        if fmt == "nv12":
            host = [gpu.NV12Frame(sc.frame_nv12(t), W, H) for sc in scs]
            dev = [_dev(gpu, f.buf) for f in host]
        else:
            host = [sc.frame_rgb8(t) for sc in scs]
            dev = []
            for a in host:
                d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
                dev.append((gpu.frame_rgb8(d.data_ptr(), W, H), d))
        keep.append(dev)
        return host, [d[0] for d in dev]

    host0, dev0 = frames(0)
    for s in range(B):
        hd.init_host(s, host0[s], gpu.BBox.new(*scs[s].gt_box(0)))
        dv.init_device(s, dev0[s], gpu.BBox.new(*scs[s].gt_box(0)))
    for t, L in enumerate([[6, 1, 3], [0], [2, 3, 4, 5, 6, 7, 1], [7, 0]], start=1):
        host, dev = frames(t)
        rh = hd.update_host([host[s] for s in L], streams=L)
        rd = dv.update_device([dev[s] for s in L], streams=L)
        assert [_res(r) for r in rh] == [_res(r) for r in rd], (L, rh, rd)
        for s in range(B):
            assert np.array_equal(_words(hd, s), _words(dv, s))


def test_no_capture_inside_an_update(gpu, weights_tiny):
    """subset passes launch eagerly: the capture count stays where creation left it; full passes interleaved with them
    still replay the captured graph"""
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    grp = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, grp, frames0, scs)
    caps = grp.graph_captures()
    assert caps >= 1
    for t, L in enumerate([[1, 2], None, [7], [0, 1, 2, 3, 4, 5, 7], None, [5, 3]], start=1):
        frames, keep = _frames_at(gpu, scs, t)
        r0 = _replays(grp)
        if L is None:
            grp.update_device(frames)
            assert _replays(grp) == r0 + 1
        else:
            grp.enqueue_device([frames[s] for s in L], streams=L)
            assert len(grp.wait()) == len(L)
            assert _replays(grp) == r0
        assert grp.graph_captures() == caps


def test_argument_checks_change_nothing(gpu, weights_tiny):
    """duplicates, out-of-range indices, n = 0, n > B, null pointers and a call while a pipelined host pass is
    outstanding: VT_ERR_INVALID_ARG, nothing enqueued, no state changed"""
    L_ = gpu.lib()
    scs = _clips(gpu)
    frames0, keep0 = _frames_at(gpu, scs, 0)
    frames1, keep1 = _frames_at(gpu, scs, 1)
    grp = gpu.Group(weights_tiny, n_streams=B)
    _init_all(gpu, grp, frames0, scs)
    last = grp.update_device([frames1[s] for s in (4, 2)], streams=[4, 2])
    arr = (gpu.CFrame * (B + 1))(*(list(frames1) + [frames1[0]]))
    out = (gpu.CResult * (B + 1))()

    def snapshot():
        return [_words(grp, s) for s in range(B)], _replays(grp), grp.graph_captures()

    def ids(*v):
        return (ctypes.c_int32 * max(len(v), 1))(*v)

    before = snapshot()
    bad = [(ids(1, 1), 2), (ids(0, 8), 2), (ids(-1), 1), (ids(0), 0), (ids(*range(B), 0), B + 1), (None, 2)]
    for streams, n in bad:
        assert L_.vt_group_enqueue_device_streams(grp._h, streams, arr, n) == INVALID, (list(streams or []), n)
        assert L_.vt_group_update_device_streams(grp._h, streams, arr, n, out) == INVALID
    assert L_.vt_group_enqueue_device_streams(grp._h, ids(0, 1), None, 2) == INVALID
    assert L_.vt_group_update_device_streams(grp._h, ids(0, 1), None, 2, out) == INVALID
    assert L_.vt_group_update_device_streams(grp._h, ids(0, 1), arr, 2, None) == INVALID
    assert L_.vt_group_update_host_streams(grp._h, ids(0, 1), None, 2, out) == INVALID
    assert L_.vt_group_update_host_streams(grp._h, None, arr, 2, out) == INVALID
    assert L_.vt_group_update_host_streams(grp._h, ids(3, 3), arr, 2, out) == INVALID
    assert L_.vt_group_enqueue_device_streams(None, ids(0), arr, 1) == INVALID
    now = snapshot()
    assert all(np.array_equal(x, y) for x, y in zip(now[0], before[0])) and now[1:] == before[1:]
    assert [_res(r) for r in grp.wait()] == [_res(r) for r in last]
    # a pipelined host pass owns the states until it is collected
    host1 = [gpu.NV12Frame(sc.frame_nv12(1), W, H) for sc in scs]
    grp.enqueue_host(host1)
    assert L_.vt_group_update_device_streams(grp._h, ids(0, 1), arr, 2, out) == INVALID
    assert L_.vt_group_enqueue_device_streams(grp._h, ids(0), arr, 1) == INVALID
    hf = (gpu.CFrame * 1)(gpu.Group._host_frame(host1[0])[0])
    assert L_.vt_group_update_host_streams(grp._h, ids(0), hf, 1, out) == INVALID
    full = grp.wait_next()
    assert len(full) == B
    after = [_words(grp, s) for s in range(B)]
    assert all(after[s][FRAMES_DONE] == before[0][s][FRAMES_DONE] + 1 for s in range(B))   # the pipelined pass only


def test_closed_loop_with_streams_joining_and_leaving(gpu, capsys):
    """traj_cfg3_300's clip followed by stream 0 of a 30-stream cfg3 group; the other 29 streams (boxes offset from the
    target) join and leave every 3 frames, so that the pass size runs between 1 and 30 and stream 0 sits in varying
    slots - alone on some passes. Stream 0 meets the bars the closed-loop tests apply to this fixture."""
    name = "traj_cfg3_300.npz"
    fx, bar = _fixture(name), BARS[name]
    weights = gpu.weights.ensure_weights(str(fx["config"]))
    sc = _clip(gpu, fx)
    w, h, n, G = sc.w, sc.h, int(fx["frames"]), 30
    grp = gpu.Group(weights, n_streams=G)
    rng = np.random.default_rng(11)
    sizes = [1, 30, 7, 19, 2, 29, 12, 1, 24, 4, 30, 16]
    boxes, scores, succ, seen = [], [], [], set()
    for t in range(n):
        f, keep = _dev(gpu, sc.frame_nv12(t), w, h)
        if t == 0:
            gx, gy, gw, gh = sc.gt_box(0)
            grp.init_device(0, f, gpu.BBox.new(gx, gy, gw, gh))
            for s in range(1, G):
                grp.init_device(s, f, gpu.BBox.new(gx + int(rng.integers(-12, 13)), gy + int(rng.integers(-12, 13)),
                                                   gw + int(rng.integers(-8, 9)), gh + int(rng.integers(-8, 9))))
        if t % 3 == 0:
            k = sizes[(t // 3) % len(sizes)]
            L = [0] + [int(s) for s in rng.choice(np.arange(1, G), k - 1, replace=False)]
            L = [int(s) for s in rng.permutation(L)]
            seen.add(k)
        res = grp.update_device([f] * len(L), streams=L)
        r = res[L.index(0)]
        boxes.append(r.bbox)
        scores.append(r.score)
        succ.append(int(r.success))
    assert {1, 30} <= seen
    boxes, scores, succ = np.array(boxes), np.array(scores), np.array(succ)
    d = np.abs(boxes - fx["bbox"])
    ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, fx["bbox"])])
    dscore = np.abs(scores - fx["score"])
    low = max(LOW_IOU_FRAMES[name])
    with capsys.disabled():
        print(f"\n[{name}, 30-stream group, pass sizes {sorted(seen)}] {n} frames: max |delta| {d.max()} px, IoU min "
              f"{ious.min():.4f} mean {ious.mean():.5f}, frames below 0.99: {(ious < 0.99).sum()} (bar {low}), "
              f"max |delta score| {dscore.max():.4f}")
    assert d.max() <= bar["px"], f"max |delta| = {d.max()} px at frame {int(d.max(axis=1).argmax())}"
    assert ious.mean() >= bar["mean_iou"] and ious.min() >= bar["min_iou"]
    assert (ious < 0.99).sum() <= low
    assert np.array_equal(succ, fx["success"].astype(int)), "success flags differ"
    assert dscore.max() < 0.10
