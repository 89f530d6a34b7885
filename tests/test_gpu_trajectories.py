"""north_star parity gate at full length: the HIP path against COMMITTED oracle
trajectories (tests/golden/traj_*.npz, forced_*.npz; generator tests/golden/make_traj.py), so the GPU
run does not pay seconds of CPU oracle per frame.

  * closed loop, 300 frames on the headline config cfg3, on cfg2 and on cfg5 (4K, ViT-L/14):
    per-frame |dx|,|dy|,|dw|,|dh| <= 1 px, equal success flags, |dscore| < 0.03, and the IoU report:
    SURVEY.md section 8(d) wrote "IoU >= 0.99 per frame", which +-1 px on a 64-px box cannot
    guarantee (one coordinate off by one is IoU 0.969, two are 0.94): the test asserts what both
    statements allow together - every frame within +-1 px, MEAN IoU >= 0.99, min IoU >= 0.90 - and
    prints the minimum and the number of frames below 0.99.
  * teacher-forced tests assert the FLOAT box (StreamState.last_fbox vs the fixture's `fbox`) to 0.15 px,
    closed-loop tests the score to 0.01 on every frame whose input was bit-identical, and the number of
    frames below IoU 0.99 may not exceed round 3's count by more than the stated headroom; the gen-1 head also runs CLOSED loop,
    bounded as ASSERTED there: max <= 6 px, at most 8 % of the frames beyond 2 px, mean IoU >= 0.975 (bars set from the
    round-4 measurement - max 4 px, 5 % beyond 2 px, mean 0.982-0.985 - so this gate catches a regression of an
    ill-conditioned head's closed loop, it does not bound the divergence a priori).
  * teacher-forced (open loop) on the FIRST-GENERATION noisy head (fitted on 128 CPU samples only,
    tests/golden/head_gen1_cfg3.npz): before every frame the HIP tracker's state is overwritten with
    the state the oracle had (vt_group_set_state_box), so each frame measures the divergence of ONE
    forward pass on an ill-conditioned head instead of a trajectory that re-synchronises. Asserted:
    same argmax cell wherever the oracle's top-1/top-2 response margin is >= MARGIN_EPS, box within
    +-1 px on every frame; the margins and the disagreements below MARGIN_EPS are printed.

The oracle is parity-unpinned against the reference (no vectors exist there)."""
import hashlib
import os

import numpy as np
import pytest

from conftest import iou

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN_EPS = 0.01      # response units (sigmoid * hann, in [0, 1])


def _sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.hexdigest()


def _fixture(name):
    path = os.path.join(GOLD, name)
    assert os.path.exists(path), f"{name} missing: python tests/golden/make_traj.py (see its docstring)"
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def _clip(gpu, fx):
    hide = tuple(int(v) for v in fx["hide"]) if "hide" in fx and fx["hide"][1] > fx["hide"][0] else None
    return gpu.synth.MovingSquare(int(fx["frame_w"]), int(fx["frame_h"]), int(fx["square"]),
                                  seed=int(fx["seed"]), hide=hide)


# Bars per fixture: the north_star's - every one of the first 300 frames within +-1 px - on all three
# configurations. (Round 2 held the 4K ViT-L/14 clip to +-2 px over 60 frames. Round 3 arbitrated: against
# an un-quantised float64 formulation both bf16 implementations are equally far from the truth at every
# stage (tools/arbiter.py, profiles/r03_arbiter_cfg5.txt: residual stream 2.2e-3 both, decoded float box
# 0.03 px both) - bf16 noise, not a kernel; what turned it into 2 px in closed loop was the head's
# conditioning on 160-px targets, so the cfg5 head was refitted on targets of that size with feature noise.)
# The `_b` fixtures are second clips: other background noise, path phase and target size (cfg3 80 px, cfg2 48 px,
# cfg5 128 px; seed 9) - the heads were fitted on a range of sizes, the first clips use one each.
BARS = {"traj_cfg3_300.npz": dict(px=1, min_iou=0.90, mean_iou=0.99),
        "traj_cfg2_300.npz": dict(px=1, min_iou=0.90, mean_iou=0.99),
        "traj_cfg5_300.npz": dict(px=1, min_iou=0.95, mean_iou=0.99),
        "traj_cfg3_300_b.npz": dict(px=1, min_iou=0.90, mean_iou=0.99),
        "traj_cfg2_300_b.npz": dict(px=1, min_iou=0.88, mean_iou=0.99),
        "traj_cfg5_300_b.npz": dict(px=1, min_iou=0.95, mean_iou=0.99)}
# Frames with IoU(hip, oracle) < 0.99 (a box off by one pixel in one coordinate): MEASURED counts of round 6's final
# run (profiles/r06_gpu_tests.log; fixtures and kernels on numerical specification v3) for the single tracker / the
# recommended-size engine. +-1 px is the guarantee, so a kernel change that moves one bf16 rounding may legitimately move a
# few of these frames: the bar is the measured count + max(2, 25 %) (round-4 advice), printed beside the measurement.
# (rounds 3-5, specification v2: cfg3 1/1, cfg2 1/1, cfg5 8/22, cfg3_b 5/6, cfg2_b 0/0, cfg5_b 3/4)
LOW_IOU_MEASURED = {"traj_cfg3_300.npz": (1, 0), "traj_cfg2_300.npz": (0, 1), "traj_cfg5_300.npz": (10, 10),
                    "traj_cfg3_300_b.npz": (2, 2), "traj_cfg2_300_b.npz": (0, 0), "traj_cfg5_300_b.npz": (6, 7)}
LOW_IOU_FRAMES = {k: tuple(c + max(2, (c + 3) // 4) for c in v) for k, v in LOW_IOU_MEASURED.items()}
# result.score where both implementations evaluated the SAME input and picked the same cell: closed-loop frames
# whose incoming state (the previous frame's integer box and success flag) is identical - then the crops are
# bit-identical and the score differs by one forward pass's bf16 noise only (teacher-forced: <= 0.003 measured)
SCORE_BAR_SAME_INPUT = 0.01
FBOX_BAR_PX = 0.15      # |HIP float box - oracle float box| per coordinate on identical inputs (measured <= 0.05)
FIXTURES = [n for n in BARS if not n.endswith("_b.npz") or os.path.exists(os.path.join(GOLD, n))]   # first clips: required


def _same_input(boxes, succ, fx):
    """frames of a closed-loop run on which HIP and oracle cut bit-identical crops: frame 0 (both start from
    the ground-truth box) and every frame whose previous results agree exactly (box and success flag) - the
    state of both is then the same integer box"""
    prev_same = (np.abs(boxes[:-1] - fx["bbox"][:-1]).max(axis=1) == 0) & (succ[:-1] == fx["success"][:-1].astype(int))
    # a state that was identical stays identical only while every earlier frame agreed, or a success re-synchronised
    # it: after a success both states ARE the reported integer box, so agreement of the previous frame is enough
    # when that frame succeeded; a lost frame keeps the older state
    ok = np.zeros(len(boxes), bool)
    ok[0] = True
    for t in range(1, len(boxes)):
        ok[t] = prev_same[t - 1] and (bool(succ[t - 1]) or ok[t - 1])
    return ok


@pytest.mark.parametrize("name", FIXTURES)
def test_closed_loop_trajectory_vs_committed_oracle(gpu, name, capsys):
    fx = _fixture(name)
    bar = BARS[name]
    cfg = str(fx["config"])
    weights = gpu.weights.ensure_weights(cfg)
    assert _sha256(weights) == str(fx["weights_sha256"]), "fixture was made with other weights"
    sc = _clip(gpu, fx)
    w, h, n = sc.w, sc.h, int(fx["frames"])
    trk = gpu.VitTrack(weights)
    g = trk.as_group()
    boxes, scores, succ, idx = [], [], [], []
    for t in range(n):
        f = gpu.NV12Frame(sc.frame_nv12(t), w, h)
        if t == 0:      # init then update on the SAME frame (src/tracker_context.rs:88-90)
            trk.init(f, gpu.BBox.new(*sc.gt_box(0)))
        r = trk.update(f)
        boxes.append(r.bbox)
        scores.append(r.score)
        succ.append(int(r.success))
        idx.append(g.read_state()["last_idx"])
    boxes, idx = np.array(boxes), np.array(idx)
    same_cell = idx == fx["idx"]
    dscore = np.abs(np.array(scores) - fx["score"])
    d = np.abs(boxes - fx["bbox"])
    same_in = _same_input(boxes, np.array(succ), fx)
    ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, fx["bbox"])])
    gt_iou = np.array([iou(tuple(a), tuple(b)) for a, b in zip(fx["bbox"], fx["gt"])])
    with capsys.disabled():
        print(f"\n[{name}] {n} frames: max |delta| {d.max()} px, IoU(hip, oracle) min {ious.min():.4f} "
              f"mean {ious.mean():.5f}, frames below 0.99: {(ious < 0.99).sum()}, identical boxes: "
              f"{(d.max(axis=1) == 0).sum()}; oracle vs ground truth min IoU {gt_iou.min():.3f}; "
              f"min top-1/top-2 margin {fx['margin'].min():.4f}; argmax cell differs on "
              f"{(~same_cell).sum()} frames (largest oracle margin among them "
              f"{fx['margin'][~same_cell].max() if (~same_cell).any() else 0:.4f}); max |delta score| "
              f"{dscore[same_cell].max():.4f} same cell / {dscore[~same_cell].max() if (~same_cell).any() else 0:.4f} other cell; "
              f"{same_in.sum()} frames on bit-identical input: max |delta score| {dscore[same_in & same_cell].max():.4f}")
    assert d.max() <= bar["px"], f"max |delta| = {d.max()} px at frame {int(d.max(axis=1).argmax())}"
    assert ious.mean() >= bar["mean_iou"] and ious.min() >= bar["min_iou"]
    assert (ious < 0.99).sum() <= LOW_IOU_FRAMES[name][0], f"{(ious < 0.99).sum()} frames below IoU 0.99 (bar {LOW_IOU_FRAMES[name][0]})"
    assert dscore[same_in & same_cell].max() < SCORE_BAR_SAME_INPUT
    assert np.array_equal(np.array(succ), fx["success"].astype(int)), "success flags differ"
    # result.score is the raw sigmoid of the ARGMAX cell, on crops that may differ by a pixel in a
    # closed loop (and by the cell where two implementations break a near-tie differently): the bar is
    # on the reported score staying on the same side of the host's 0.25 gate with a wide margin
    # (src/tracker_context.rs:93,122); the tight same-input comparison is the teacher-forced test below
    assert dscore.max() < 0.10
    assert gt_iou.min() > 0.5, "the oracle lost the target: the parity above would be vacuous"


@pytest.mark.parametrize("name", FIXTURES)
def test_closed_loop_through_the_batched_large_tile_path(gpu, name, capsys):
    """The same full-length gate on the path bench.py times: ONE engine of as many streams as
    vt_recommended_streams says (cfg3: 30 streams, M = 21,600 rows: every encoder GEMM on the 256x256
    kernels - persistent for QKV / fc1 -, attention on the LDS-DMA kernel), every stream fed the
    fixture's clip. The single-tracker test above runs the same weights through the small-tile
    kernels; here each stream must meet the fixture's bars, and - the inputs being identical - all
    streams must agree with each other exactly (a kernel whose result depended on the row's position
    in the batch would show here)."""
    fx, bar = _fixture(name), BARS[name]
    cfg = str(fx["config"])
    weights = gpu.weights.ensure_weights(cfg)
    assert _sha256(weights) == str(fx["weights_sha256"]), "fixture was made with other weights"
    sc = _clip(gpu, fx)
    w, h, n, B = sc.w, sc.h, int(fx["frames"]), gpu.weights.recommended_streams(cfg)
    assert B >= 30
    grp = gpu.Group(weights, n_streams=B)
    boxes, scores, succ = [], [], []
    for t in range(n):
        f = gpu.NV12Frame(sc.frame_nv12(t), w, h)
        if t == 0:
            for i in range(B):
                grp.init_host(i, f, gpu.BBox.new(*sc.gt_box(0)))
        res = grp.update_host([f] * B)
        boxes.append([r.bbox for r in res])
        scores.append([r.score for r in res])
        succ.append([int(r.success) for r in res])
    boxes, scores, succ = np.array(boxes), np.array(scores), np.array(succ)      # [n][B][4], [n][B]
    assert np.array_equal(boxes, np.repeat(boxes[:, :1], B, axis=1)), "streams with identical input disagree"
    assert np.array_equal(scores, np.repeat(scores[:, :1], B, axis=1))
    b0 = boxes[:, 0]
    d = np.abs(b0 - fx["bbox"])
    ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(b0, fx["bbox"])])
    dscore = np.abs(scores[:, 0] - fx["score"])
    same_in = _same_input(b0, succ[:, 0], fx)
    with capsys.disabled():
        print(f"\n[{name}, {B}-stream engine] {n} frames x {B} streams: max |delta| {d.max()} px, IoU(hip, oracle) min "
              f"{ious.min():.4f} mean {ious.mean():.5f}, frames below 0.99: {(ious < 0.99).sum()}, identical boxes: "
              f"{(d.max(axis=1) == 0).sum()}, max |delta score| {dscore.max():.4f} ({dscore[same_in].max():.4f} on the "
              f"{same_in.sum()} frames with bit-identical input); all {B} streams bit-identical to each other")
    assert d.max() <= bar["px"], f"max |delta| = {d.max()} px at frame {int(d.max(axis=1).argmax())}"
    assert ious.mean() >= bar["mean_iou"] and ious.min() >= bar["min_iou"]
    assert (ious < 0.99).sum() <= LOW_IOU_FRAMES[name][1], f"{(ious < 0.99).sum()} frames below IoU 0.99 (bar {LOW_IOU_FRAMES[name][1]})"
    assert dscore[same_in].max() < 2 * SCORE_BAR_SAME_INPUT        # the cell may differ at a near-tie: twice the same-cell bar
    assert np.array_equal(succ[:, 0], fx["success"].astype(int)), "success flags differ"
    assert dscore.max() < 0.10


def test_target_lost_and_reacquired_like_the_oracle(gpu, capsys):
    """occlusion: the target is absent from 12 frames of a cfg2 clip (tests/golden/traj_cfg2_160_occl.npz,
    make_traj.py --hide 80 92). The oracle reports success = 0 on exactly those frames (score ~ 0), keeps
    its state box, and re-acquires on the first frame the target is back. Closed loop, single tracker and
    a 67-stream engine: the same success flag on every frame, boxes within 1 px on every tracked frame,
    scores within 0.03 on the lost ones (the reference's host counts lost frames: src/tracker_context.rs:120-140)"""
    fx = _fixture("traj_cfg2_160_occl.npz")
    weights = gpu.weights.ensure_weights("cfg2")
    assert _sha256(weights) == str(fx["weights_sha256"]), "fixture was made with other weights"
    sc = _clip(gpu, fx)
    w, h, n = sc.w, sc.h, int(fx["frames"])
    lost = fx["success"] == 0
    assert lost.sum() >= 10 and not lost[:int(fx["hide"][0])].any() and fx["success"][int(fx["hide"][1]) + 1:].all()
    B = gpu.recommended_streams(gpu.model_info_for("cfg2"))
    trk, grp = gpu.VitTrack(weights), gpu.Group(weights, n_streams=B)
    boxes, succ, scores = [], [], []
    for t in range(n):
        f = gpu.NV12Frame(sc.frame_nv12(t), w, h)
        if t == 0:
            trk.init(f, gpu.BBox.new(*sc.gt_box(0)))
            for i in range(B):
                grp.init_host(i, f, gpu.BBox.new(*sc.gt_box(0)))
        r = trk.update(f)
        rg = grp.update_host([f] * B)
        assert all(x.bbox == rg[0].bbox and x.score == rg[0].score and x.success == rg[0].success for x in rg)
        assert rg[0].success == r.success and (not r.success or np.abs(np.array(rg[0].bbox) - np.array(r.bbox)).max() <= 1)
        boxes.append(r.bbox); succ.append(int(r.success)); scores.append(r.score)
    boxes, succ, scores = np.array(boxes), np.array(succ), np.array(scores)
    ok = ~lost
    d = np.abs(boxes[ok] - fx["bbox"][ok])
    with capsys.disabled():
        print(f"\n[occlusion, cfg2] {n} frames, {lost.sum()} lost by the oracle: success flags differ on "
              f"{(succ != fx['success']).sum()} frames; tracked frames: max |delta| {d.max()} px, identical boxes "
              f"{(d.max(axis=1) == 0).sum()} of {ok.sum()}; lost frames: max score {scores[lost].max():.4f} (oracle "
              f"{fx['score'][lost].max():.4f})")
    assert np.array_equal(succ, fx["success"].astype(int)), "success flags differ"
    assert d.max() <= 1
    assert np.abs(scores[lost] - fx["score"][lost]).max() < 0.03


def _teacher_forced(gpu, fx, weights, engine_streams):
    """one forward pass per frame on the oracle's own state; engine_streams = 1: the single tracker (4-wave
    kernels), else an engine of that many streams all fed the same frame (256x256 kernels), stream 0 reported
    after checking that every stream agrees bit for bit. Returns idx, integer boxes, scores, float boxes."""
    sc = _clip(gpu, fx)
    w, h, n = sc.w, sc.h, int(fx["frames"])
    B = engine_streams
    grp = gpu.Group(weights, n_streams=B)
    idx, boxes, scores, fboxes = [], [], [], []
    for t in range(n):
        f = gpu.NV12Frame(sc.frame_nv12(t), w, h)
        if t == 0:
            for i in range(B):
                grp.init_host(i, f, gpu.BBox.new(*sc.gt_box(0)))
        for i in range(B):
            grp.set_state_box(i, fx["state"][t])          # the oracle's state before its update of frame t
        res = grp.update_host([f] * B)
        assert all(r.bbox == res[0].bbox and r.score == res[0].score for r in res)
        st = grp.read_state(0)
        idx.append(st["last_idx"])
        fboxes.append(st["last_fbox"])
        boxes.append(res[0].bbox)
        scores.append(res[0].score)
    return np.array(idx), np.array(boxes), np.array(scores), np.array(fboxes)


def _check_teacher_forced(fx, tag, idx, boxes, scores, fboxes, capsys, fbox_bar=FBOX_BAR_PX, score_bar=SCORE_BAR_SAME_INPUT):
    assert "fbox" in fx, "fixture has no float boxes: python tests/golden/make_traj.py fbox <fixture>"
    n = len(idx)
    d = np.abs(boxes - fx["bbox"])
    clear = fx["margin"] >= MARGIN_EPS
    differ = idx != fx["idx"]
    ds = np.abs(scores - fx["score"])
    df = np.abs(fboxes - fx["fbox"]).max(axis=1)             # px, worst coordinate per frame
    with capsys.disabled():
        print(f"\n[teacher-forced, {tag}] {n} frames: frames with oracle margin < {MARGIN_EPS}: {(~clear).sum()}; argmax "
              f"differs on {differ.sum()} frames (largest oracle margin among them "
              f"{fx['margin'][differ].max() if differ.any() else 0:.5f}); max |delta box| {d.max()} px, identical boxes "
              f"{(d.max(axis=1) == 0).sum()}; FLOAT box: max |delta| {df[~differ].max():.4f} px, mean {df[~differ].mean():.4f} px "
              f"on the same cell{'' if not differ.any() else f', {df[differ].max():.4f} px on another cell'}; "
              f"max |delta score| {ds[~differ].max():.4f}")
    assert not (differ & clear).any(), \
        f"argmax differs at margin {fx['margin'][differ & clear].max():.4f} (frame {int(np.argmax(differ & clear))})"
    assert d.max() <= 1, f"open-loop box differs by {d.max()} px at frame {int(d.max(axis=1).argmax())}"
    # the integer box hides up to a pixel of float error: on identical inputs the FLOAT boxes must agree to a
    # fraction of a pixel wherever both decode around the same cell (a near-tie taken the other way moves the
    # 3x3 decode window by a cell: second-order, bounded by the +-1 px above)
    assert df[~differ].max() <= fbox_bar, \
        f"float box differs by {df[~differ].max():.3f} px at frame {int(np.argmax(np.where(~differ, df, 0)))}"
    assert df.max() <= 1.0
    assert ds[~differ].max() < score_bar and ds.max() < 0.10


@pytest.mark.parametrize("name", FIXTURES)
def test_teacher_forced_on_the_trajectory_fixtures(gpu, name, capsys):
    """open loop on the three shipped heads: before every frame the HIP state is overwritten with the
    oracle's state of that frame (the fixture's `state`), so each of the 300 frames is ONE forward pass on
    the oracle's own input - closed-loop runs can differ in the argmax cell merely because their crops
    differ by a pixel (cfg5: 2 frames); on identical inputs the cell must be the oracle's wherever its
    top-1/top-2 margin is >= MARGIN_EPS, the integer box within +-1 px, the FLOAT box (StreamState.last_fbox
    against the fixture's `fbox`) within FBOX_BAR_PX, the score within SCORE_BAR_SAME_INPUT on the same cell.
    Both kernel families: the single tracker and the recommended-size engine."""
    fx = _fixture(name)
    cfg = str(fx["config"])
    weights = gpu.weights.ensure_weights(cfg)
    assert _sha256(weights) == str(fx["weights_sha256"]), "fixture was made with other weights"
    _check_teacher_forced(fx, name, *_teacher_forced(gpu, fx, weights, 1), capsys)
    B = gpu.weights.recommended_streams(cfg)
    _check_teacher_forced(fx, f"{name}, {B}-stream engine", *_teacher_forced(gpu, fx, weights, B), capsys)


def test_the_configuration_bench_times_against_the_oracle(gpu, capsys):
    """Exactly what bench.py's headline times (round-4 verdict, item 2): cfg3, TWO engines of 30 streams, one host thread
    per engine released together by a barrier, vt_group_enqueue_host / vt_group_wait_next with the default speculative
    margin (upload of step t + 1 on the copy stream under the pass of step t), 300 frames of traj_cfg3_300's clip, the
    streams of an engine at six DISTINCT clip offsets (0, 3, ..., 15 frames: their boxes, windows and packed uploads
    differ). Asserted:
      * every stream at offset 0 (five per engine) meets the fixture's bars against the committed oracle trajectory;
      * every stream of the pipelined two-thread run is bit-identical - box, score, success flag, every frame - to the
        same stream of a synchronous vt_group_update_host run of one engine alone (a race between a copy stream and
        the neighbouring engine's pass, or a redo that restores the wrong state, would show here);
      * the redone passes are counted and reported.
    The reference's own loop is one tracker per process (src/pipeline.rs:55) calling update per frame
    (src/tracker_context.rs:88-98,120-131); this is its batched form."""
    import threading
    name = "traj_cfg3_300.npz"
    fx, bar = _fixture(name), BARS[name]
    weights = gpu.weights.ensure_weights(str(fx["config"]))
    assert _sha256(weights) == str(fx["weights_sha256"]), "fixture was made with other weights"
    sc = _clip(gpu, fx)
    w, h, n, B, G = sc.w, sc.h, int(fx["frames"]), 30, 2
    assert B == gpu.weights.recommended_streams(str(fx["config"]))
    offs = [[3 * ((g * B + i) % 6) for i in range(B)] for g in range(G)]
    frames = [gpu.NV12Frame(sc.frame_nv12(t), w, h) for t in range(n + 16)]

    def init(grp, g):
        for i, o in enumerate(offs[g]):
            grp.init_host(i, frames[o], gpu.BBox.new(*sc.gt_box(o)))

    def fr(g, t):
        return [frames[t + o] for o in offs[g]]

    def pack(res):
        return [(r.bbox, r.score, int(r.success)) for r in res]

    # synchronous reference: each engine alone, one call per step, no overlap
    want = []
    for g in range(G):
        grp = gpu.Group(weights, n_streams=B)
        init(grp, g)
        want.append([pack(grp.update_host(fr(g, t))) for t in range(n)])
        del grp

    # the timed configuration: both engines alive, one thread each, pipelined ingest
    grps = [gpu.Group(weights, n_streams=B) for _ in range(G)]
    for g in range(G):
        init(grps[g], g)
    got, errs = [None] * G, []
    start = threading.Barrier(G)

    def worker(g):
        try:
            out = []
            start.wait()
            grps[g].enqueue_host(fr(g, 0))
            for t in range(1, n):
                grps[g].enqueue_host(fr(g, t))
                out.append(pack(grps[g].wait_next()))
            out.append(pack(grps[g].wait_next()))
            got[g] = out
        except BaseException as e:      # a failing engine must not leave the other at the barrier
            errs.append(e)
            start.abort()

    th = [threading.Thread(target=worker, args=(g,)) for g in range(G)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    redos = [grps[g].host_redos() for g in range(G)]
    for g in range(G):
        assert got[g] == want[g], f"engine {g}: pipelined two-thread run differs from the synchronous run"
    # offset-0 streams against the oracle
    worst = dict(px=0, min_iou=1.0, low=0)
    for g in range(G):
        for i, o in enumerate(offs[g]):
            if o:
                continue
            boxes = np.array([got[g][t][i][0] for t in range(n)])
            scores = np.array([got[g][t][i][1] for t in range(n)])
            succ = np.array([got[g][t][i][2] for t in range(n)])
            d = np.abs(boxes - fx["bbox"])
            ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, fx["bbox"])])
            same_in = _same_input(boxes, succ, fx)
            assert d.max() <= bar["px"], f"engine {g} stream {i}: max |delta| = {d.max()} px at frame {int(d.max(axis=1).argmax())}"
            assert ious.mean() >= bar["mean_iou"] and ious.min() >= bar["min_iou"]
            assert (ious < 0.99).sum() <= LOW_IOU_FRAMES[name][1]
            assert np.array_equal(succ, fx["success"].astype(int)), "success flags differ"
            assert np.abs(scores - fx["score"])[same_in].max() < 2 * SCORE_BAR_SAME_INPUT
            worst = dict(px=max(worst["px"], int(d.max())), min_iou=min(worst["min_iou"], float(ious.min())),
                         low=max(worst["low"], int((ious < 0.99).sum())))
    # the other offsets have no oracle trajectory of their own (the fixture is ONE closed loop from frame 0): they
    # must track the ground truth like the oracle does on its clip
    gt_iou_min = min(iou(tuple(got[g][t][i][0]), sc.gt_box(t + o)) for g in range(G) for i, o in enumerate(offs[g])
                     for t in range(0, n, 7))
    with capsys.disabled():
        print(f"\n[bench configuration: cfg3, {G} engines x {B} streams, two threads, pipelined host ingest] {n} frames: all "
              f"{G * B} streams bit-identical to the synchronous run; offset-0 streams vs oracle: max |delta| {worst['px']} px, "
              f"min IoU {worst['min_iou']:.4f}, frames below 0.99: {worst['low']}; redone passes per engine {redos}; "
              f"min IoU vs ground truth over all offsets {gt_iou_min:.3f}")
    assert gt_iou_min > 0.8
    del grps


def _gen1_weights(gpu, fx):
    with np.load(os.path.join(GOLD, "head_gen1_cfg3.npz")) as z:
        head = {k: z[k] for k in z.files}
    weights = gpu.weights.ensure_weights(
        "cfg3", path=os.path.join(gpu.weights.default_cache_dir(), "vitb16_t192_s384_gen1head.vtw"),
        head=head)
    assert _sha256(weights) == str(fx["weights_sha256"]), "fixture was made with other weights"
    return weights


def test_teacher_forced_on_the_noisy_first_generation_head(gpu, capsys):
    fx = _fixture("forced_cfg3_300.npz")
    weights = _gen1_weights(gpu, fx)
    idx, boxes, scores, fboxes = _teacher_forced(gpu, fx, weights, 1)
    swapped = (idx != fx["idx"]) & (idx == fx["idx2"])           # HIP took the oracle's runner-up
    with capsys.disabled():
        print(f"\n[gen-1 head] oracle margin min {fx['margin'].min():.5f} median {np.median(fx['margin']):.4f}; "
              f"{swapped.sum()} frames on the oracle's runner-up; oracle success on {int(fx['success'].sum())} frames")
    _check_teacher_forced(fx, "gen-1 head", idx, boxes, scores, fboxes, capsys)
    _check_teacher_forced(fx, "gen-1 head, 30-stream engine", *_teacher_forced(gpu, fx, weights, 30), capsys)


def test_closed_loop_on_the_ill_conditioned_first_generation_head(gpu, capsys):
    """The shipped heads are well conditioned on purpose; closed-loop parity must not rest
    on that alone. forced_cfg3_300.npz IS the oracle's closed loop on the deliberately noisy gen-1 head (fitted
    on 128 samples: its box jitters by 1-2 px from frame to frame against the ground truth, top-1/top-2 margins
    down to 0.0008). HIP runs the same clip closed loop, single tracker and 30-stream engine. Measured (round 4,
    MI355X): 192 of 300 boxes identical, 66 off by 1 px, 27 by 2 px, 15 by 3-4 px, the two trajectories
    re-synchronise again and again (the last 30 frames are identical) - an ill-conditioned head turns one bf16
    rounding flip into a few pixels for a few frames, where the shipped heads give +-1 px. Round 6 (oracle and
    kernels on the 3-byte residual pair; the fixture regenerated): 159 / 176 identical (1 / 30 streams), 18 / 13
    frames at 3-5 px, min IoU 0.881 / 0.854 - another draw of the same noise: against the ground truth HIP reads
    0.9665 / 0.9668 mean IoU where the oracle reads 0.9656. This test REPORTS
    that and BOUNDS it: no frame beyond 6 px, at most 8 % of the frames beyond 2 px, mean IoU >= 0.975, min IoU
    >= 0.82 (the oracle itself is at 0.879 against the truth), equal
    success flags - and, the yardstick that matters for such a head, HIP is as close to the GROUND TRUTH as
    the oracle is (mean IoU within 0.01): the divergence is inside the head's own noise."""
    fx = _fixture("forced_cfg3_300.npz")
    weights = _gen1_weights(gpu, fx)
    sc = _clip(gpu, fx)
    w, h, n = sc.w, sc.h, int(fx["frames"])
    gt_oracle = np.array([iou(tuple(a), tuple(b)) for a, b in zip(fx["bbox"], fx["gt"])])
    for B in (1, 30):
        grp = gpu.Group(weights, n_streams=B)
        boxes, succ = [], []
        for t in range(n):
            f = gpu.NV12Frame(sc.frame_nv12(t), w, h)
            if t == 0:
                for i in range(B):
                    grp.init_host(i, f, gpu.BBox.new(*sc.gt_box(0)))
            res = grp.update_host([f] * B)
            assert all(r.bbox == res[0].bbox for r in res)
            boxes.append(res[0].bbox)
            succ.append(int(res[0].success))
        boxes = np.array(boxes)
        d = np.abs(boxes - fx["bbox"]).max(axis=1)
        ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, fx["bbox"])])
        gt_hip = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, fx["gt"])])
        with capsys.disabled():
            print(f"\n[closed loop, gen-1 head, {B} stream(s)] {n} frames: identical boxes {(d == 0).sum()}, off by 1 px "
                  f"{(d == 1).sum()}, by 2 px {(d == 2).sum()}, by 3 px or more {(d > 2).sum()} (max {d.max()} px, first "
                  f"beyond 1 px at frame {int(np.argmax(d > 1)) if (d > 1).any() else -1}); IoU(hip, oracle) min "
                  f"{ious.min():.4f} mean {ious.mean():.5f}, frames below 0.99: {(ious < 0.99).sum()}; against the ground "
                  f"truth: oracle mean IoU {gt_oracle.mean():.4f} min {gt_oracle.min():.3f}, HIP mean {gt_hip.mean():.4f} "
                  f"min {gt_hip.min():.3f}  [bars, set from the round-4 and round-6 runs: max <= 6 px, beyond 2 px <= {int(0.08 * n)} frames, "
                  f"mean IoU >= 0.975, min IoU >= 0.82]")
        assert d.max() <= 6, f"closed loop on the gen-1 head diverged by {d.max()} px at frame {int(d.argmax())}"
        assert (d > 2).sum() <= 0.08 * n and ious.mean() >= 0.975 and ious.min() >= 0.82
        assert np.array_equal(np.array(succ), fx["success"].astype(int)), "success flags differ"
        assert abs(gt_hip.mean() - gt_oracle.mean()) <= 0.01 and gt_hip.min() > 0.5
