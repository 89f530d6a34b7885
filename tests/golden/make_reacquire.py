"""Generates the committed oracle fixtures of the re-acquisition tests (tests/test_candidates_abi.py,
tests/test_gpu_candidates.py): a target that jumps out of its stream's search window, the scan that finds it again and
the closed loop behind it. CPU oracle only (oracle/vit_ref.py + oracle/vt_oracle.c, both unchanged).

  python tests/golden/make_reacquire.py cfg2      -> tests/golden/reacquire_cfg2.npz   (90 windows + 24 frames: 2-10 min,
  python tests/golden/make_reacquire.py cfg3      -> tests/golden/reacquire_cfg3.npz    depending on the cores the oracle gets)

The clip (1080p NV12, 64-px target): MovingSquare(seed=0) for frames 0-2, then the same scene - same background, same
target - on MovingSquare(seed=0, center=(0.23 W, 0.71 H), amp=0.05 min(W, H)) from frame 3 on: the target reappears
about 550 px away, far outside the 256-px search window.

Recorded:
  pre_*     init on frame 0, updates on frames 0, 1, 2 (the usual closed loop)
  plain_*   the plain update on frame 3: it must fail
  boxes     the scan windows of frame 3 (the grid of vt_scan_windows, restated here), 50 % overlap, grid order
  slot_*    the scan in chunks of CHUNK slots, each slot one update with the oracle's box set to the window's and the
            state put back afterwards (a slot is an independent update): score, success, integer box, argmax cell
  chunk_winner / stop_chunk   the winner of every chunk run (greatest score, lowest slot on a tie) and the first
            chunk whose winner succeeds; the scan stops there and the winner's box becomes the state
  track_*   20 closed-loop frames behind it (frames 4..23), with the ground truth

The conditions that keep the GPU test from being vacuous are asserted here, and again on the committed files by
tests/test_candidates_abi.py. Each file records the SHA-256 of the weight blob it was made with.
"""
from __future__ import annotations

import hashlib
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import gstreamer_vit_tracker_amd as vt  # noqa: E402  (weights writer + synthetic clip only)
from oracle import vit_ref as R  # noqa: E402

W, H, SQ, CHUNK, JUMP_AT, TRACK = 1920, 1080, 64, 30, 3, 20
THRESHOLD_GAP = 0.05


def sha256_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.hexdigest()


def clip():
    """(frame t -> packed NV12, frame t -> ground-truth box)"""
    a = vt.synth.MovingSquare(W, H, SQ, seed=0)
    b = vt.synth.MovingSquare(W, H, SQ, seed=0, center=(0.23 * W, 0.71 * H), amp=0.05 * min(W, H))
    pick = lambda t: a if t < JUMP_AT else b   # noqa: E731
    return (lambda t: pick(t).frame_nv12(t)), (lambda t: pick(t).gt_box(t))


def scan_windows(w, h, bw, bh, overlap_pct=50):
    """the grid of vt_scan_windows (include/vittrack_hip.h), in double precision, boxes rounded to float32"""
    side = 4.0 * math.sqrt(float(bw) * float(bh))
    stride = side * (100 - overlap_pct) / 100.0

    def axis(L):
        if L <= side:
            return [L / 2.0]
        n = int(math.ceil((L - side) / stride)) + 1
        return [side / 2.0 + i * (L - side) / (n - 1) for i in range(n)]
    return np.array([(cx - bw / 2.0, cy - bh / 2.0, bw, bh) for cy in axis(float(h)) for cx in axis(float(w))], np.float32)


def iou(a, b):
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    x2, y2 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = max(0, x2 - x1) * max(0, y2 - y1)
    return inter / float(a[2] * a[3] + b[2] * b[3] - inter)


def winner_of(scores):
    """greatest score; a NaN loses to any number; the lowest slot on a tie"""
    best = 0
    for j in range(1, len(scores)):
        sa, sb = scores[j], scores[best]
        if (not math.isnan(sa)) and (math.isnan(sb) or sa > sb):
            best = j
    return best


def check(fx):
    """the conditions the GPU test relies on; AssertionError names the one that does not hold"""
    thr = float(fx["threshold"])
    assert np.all(np.abs(fx["slot_score"] - thr) > THRESHOLD_GAP), "an oracle slot score lies within 0.05 of the threshold"
    ok = fx["slot_success"] != 0
    assert ok.any(), "no oracle slot succeeds"
    gt = fx["gt_jump"]
    assert np.all(np.abs(fx["slot_bbox"][ok] - gt[None, :]).max(axis=1) <= 1), "a succeeding slot's box is off the ground truth"
    assert int(fx["plain_success"]) == 0, "the plain update on the frame after the jump succeeds"
    ious = [iou(b, g) for b, g in zip(fx["track_bbox"], fx["track_gt"])]
    assert len(ious) == TRACK and min(ious) > 0.5 and np.all(fx["track_success"] != 0), "the oracle loses the target again"
    stop = int(fx["stop_chunk"])
    assert 0 <= stop < len(fx["chunk_winner"]) and fx["slot_success"][fx["chunk_winner"][stop]] != 0
    assert all(fx["slot_success"][wi] == 0 for wi in fx["chunk_winner"][:stop]), "a chunk before the stop chunk succeeds"


def run(cfg: str, out: str):
    weights = vt.weights.ensure_weights(cfg)
    frame, gt = clip()
    trk = R.VitTrackRef(weights)
    fr = lambda t: R.Frame.nv12(frame(t), W, H)   # noqa: E731
    t0 = time.time()
    rec = {k: [] for k in ("pre_bbox", "pre_score", "pre_success", "pre_gt", "slot_score", "slot_success", "slot_bbox",
                           "slot_idx", "chunk_winner", "track_bbox", "track_score", "track_success", "track_gt")}
    trk.init(fr(0), gt(0))
    for t in range(JUMP_AT):
        r = trk.update(fr(t))
        rec["pre_bbox"].append(r.bbox); rec["pre_score"].append(r.score)
        rec["pre_success"].append(int(r.success)); rec["pre_gt"].append(gt(t))
    f3 = fr(JUMP_AT)
    state = trk.box.copy()
    plain = trk.update(f3)
    print(f"[{cfg}] plain update on frame {JUMP_AT}: {plain} ({time.time() - t0:.0f}s)", flush=True)
    trk.box = state.copy()
    boxes = scan_windows(W, H, float(state[2]), float(state[3]))
    stop = -1
    for c0 in range(0, len(boxes), CHUNK):
        for b in boxes[c0:c0 + CHUNK]:
            trk.box = b.astype(np.float32).copy()
            r = trk.update(f3)
            trk.box = state.copy()          # a slot is an independent update: nothing of it stays
            rec["slot_score"].append(r.score); rec["slot_success"].append(int(r.success))
            rec["slot_bbox"].append(r.bbox); rec["slot_idx"].append(r.idx)
        wi = c0 + winner_of(rec["slot_score"][c0:])
        rec["chunk_winner"].append(wi)
        print(f"[{cfg}] chunk {c0 // CHUNK}: winner slot {wi} score {rec['slot_score'][wi]:.4f} "
              f"success {rec['slot_success'][wi]} box {rec['slot_bbox'][wi]} ({time.time() - t0:.0f}s)", flush=True)
        if rec["slot_success"][wi]:
            stop = c0 // CHUNK
            trk.box = np.array(rec["slot_bbox"][wi], np.float32)
            break
    for t in range(JUMP_AT + 1, JUMP_AT + 1 + TRACK):
        r = trk.update(fr(t))
        rec["track_bbox"].append(r.bbox); rec["track_score"].append(r.score)
        rec["track_success"].append(int(r.success)); rec["track_gt"].append(gt(t))
    fx = dict(config=cfg, frame_w=W, frame_h=H, square=SQ, chunk=CHUNK, jump_at=JUMP_AT, weights_sha256=sha256_file(weights),
              threshold=np.float32(trk.thr), state_before=state.astype(np.float32), gt_jump=np.array(gt(JUMP_AT), np.int32),
              plain_score=np.float32(plain.score), plain_success=np.int8(plain.success), plain_bbox=np.array(plain.bbox, np.int32),
              plain_idx=np.int32(plain.idx), boxes=boxes, stop_chunk=np.int32(stop),
              chunk_winner=np.array(rec["chunk_winner"], np.int32),
              slot_score=np.array(rec["slot_score"], np.float32), slot_success=np.array(rec["slot_success"], np.int8),
              slot_bbox=np.array(rec["slot_bbox"], np.int32), slot_idx=np.array(rec["slot_idx"], np.int32),
              pre_bbox=np.array(rec["pre_bbox"], np.int32), pre_score=np.array(rec["pre_score"], np.float32),
              pre_success=np.array(rec["pre_success"], np.int8), pre_gt=np.array(rec["pre_gt"], np.int32),
              track_bbox=np.array(rec["track_bbox"], np.int32), track_score=np.array(rec["track_score"], np.float32),
              track_success=np.array(rec["track_success"], np.int8), track_gt=np.array(rec["track_gt"], np.int32))
    check(fx)
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out)} bytes, {time.time() - t0:.0f}s)", flush=True)


if __name__ == "__main__":
    cfg = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
    assert cfg in ("cfg2", "cfg3"), cfg
    run(cfg, os.path.join(HERE, f"reacquire_{cfg}.npz"))
