"""Generates the committed oracle fixture of the motion-prior tests (tests/test_motion_prior_cases.py,
tests/test_gpu_motion_prior.py): a fast clip with one occlusion gap on which the oracle driven by the motion rule keeps the
target and the plain oracle loses it. CPU oracle only (oracle/vit_ref.py + oracle/vt_oracle.c, both unchanged), driven
through tests/motion_prior_util.py (the NumPy-float32 model of place / settle setting VitTrackRef.box).

  python tests/golden/make_motion_prior.py      -> tests/golden/motion_prior_tiny.npz   (seconds)

The clip (RGB8, 480 x 360, 24-px target, the `tiny` weights): MovingSquare(seed=2, period=240) sampled every 7th frame - up
to 31 px, about 1.3 box sides, between two updates - for 41 frames (init + 40 updates); on clip frames 140..160, three
updates, the target is occluded: blended into the background at 104 / 256 of its contrast (the occlusion of
tests/golden/make_reacquire.py - a window that holds background only - leaves a flat response map whose maximum is decided
by the last bits, so an implementation's box on such a frame says nothing; through a semi-transparent occluder the update
still fails, at a score of 0.01, but its argmax is decisive - recorded as `margin`, the best response over the best outside
its 3 x 3 neighbourhood - and the box on every frame can be compared). Policy: gain 70 (not representable in binary32),
coast 5, limit 200.

Recorded, per update: the oracle's integer boxes, scores, success flags and argmax cells for the driven and for the plain
oracle, the state box and the motion record behind every driven update, the ground truth, which updates are occluded, and
the measured minimum IoU against the ground truth over the visible updates.

The conditions that keep the tests from being vacuous are asserted here, and again on the committed file by
tests/test_motion_prior_cases.py. The file records the SHA-256 of the weight blob it was made with.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gstreamer_vit_tracker_amd as vt  # noqa: E402  (weights writer + synthetic clip only)
import motion_prior_util as mu  # noqa: E402

W, H, SQ, SEED, PERIOD, STEP, N = 480, 360, 24, 2, 240, 7, 41
HIDE = (20 * STEP, 23 * STEP)
FAINT = 104         # of 256: the target's share of an occluded frame
POLICY = (1, 70, 5, 200)
THRESHOLD_GAP = 0.05
OUT = os.path.join(HERE, "motion_prior_tiny.npz")


def scene():
    return vt.synth.MovingSquare(W, H, SQ, seed=SEED, period=PERIOD)


def clip(n=N):
    """-> (scene, clip times, RGB8 frames): n frames, every STEP-th of the scene, the occluded ones blended"""
    sc = scene()
    ts, frames = mu.clip_frames(sc, n, STEP)
    bg = vt.synth.MovingSquare(W, H, SQ, seed=SEED, period=PERIOD, hide=(0, 1 << 30)).frame_rgb8(0).astype(np.uint16)
    for i, t in enumerate(ts):
        if HIDE[0] <= t < HIDE[1]:
            frames[i] = ((bg * (256 - FAINT) + frames[i].astype(np.uint16) * FAINT + 128) >> 8).astype(np.uint8)
    return sc, ts, frames


class MarginTracker(mu.OracleTracker):
    """records, per update, how decisive the argmax was: the best response over the best outside its 3 x 3 neighbourhood"""

    def __init__(self, weights):
        super().__init__(weights)
        self.margins = []

    def update(self, rgb):
        from oracle import vit_ref as o
        r = self.ref.update(o.Frame.rgb8(rgb), taps=True)
        gs = self.ref.m.gs
        ho = np.asarray(self.ref.last["head_out"], np.float64).reshape(-1, 8)[:, 0]
        resp = (self.ref.m.t["hann"].reshape(-1).astype(np.float64) / (1.0 + np.exp(-ho))).reshape(gs, gs)
        by, bx = np.unravel_index(int(np.argmax(resp)), resp.shape)
        rest = resp.copy()
        rest[max(by - 1, 0):by + 2, max(bx - 1, 0):bx + 2] = 0.0
        self.margins.append(resp[by, bx] / max(rest.max(), 1e-300))
        return r


def sha256_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.hexdigest()


def check(fx):
    """the conditions the tests rely on; AssertionError names the one that does not hold"""
    vis = fx["hidden"] == 0
    thr = float(fx["threshold"])
    assert np.all(np.abs(fx["score"] - thr) > THRESHOLD_GAP), "a score of the driven oracle lies within 0.05 of the threshold"
    assert np.all(fx["success"][vis] != 0), "the driven oracle fails on a visible frame"
    ious = np.array([mu.iou(b, g) for b, g in zip(fx["bbox"], fx["gt"])])
    assert abs(float(ious[vis].min()) - float(fx["min_iou"])) < 1e-6 and float(fx["min_iou"]) > 0.3, "the driven oracle leaves the target"
    after = np.arange(len(vis)) > np.flatnonzero(~vis).max()
    assert ious[after].min() > 0.3, "the driven oracle does not re-acquire the target behind the gap"
    assert not fx["success"][~vis].any(), "the driven oracle succeeds on an occluded frame: no failed update is exercised"
    p_ious = np.array([mu.iou(b, g) for b, g in zip(fx["plain_bbox"], fx["gt"])])
    assert p_ious[after].max() < 0.3 and not fx["plain_success"][after].any(), "the plain oracle finds the target again"
    assert int(fx["rec_words"][-1][10]) >= 2, "fewer than two failed updates coasted"
    assert fx["margin"].min() >= 1.5, "an update's argmax is not decisive: its box depends on the last bits of the response map"
    assert np.abs(fx["rec_words"][:, 0:2].view(np.float32)).max() > float(SQ), "the velocity never exceeds a box side"


def run(out: str):
    weights = vt.weights.ensure_weights("tiny")
    sc, ts, frames = clip()
    pol = mu.Policy(*POLICY)
    trk = MarginTracker(weights)
    res, recs, boxes = mu.drive(trk, frames, sc.gt_box(0), pol, W, H)
    pres, _, pboxes = mu.drive(mu.OracleTracker(weights), frames, sc.gt_box(0), None, W, H)
    gt = np.array([sc.gt_box(t) for t in ts[1:]], np.int32)
    hidden = np.array([HIDE[0] <= t < HIDE[1] for t in ts[1:]], np.int8)
    bbox = np.array([r.bbox for r in res], np.int32)
    ious = np.array([mu.iou(b, g) for b, g in zip(bbox, gt)])
    thr = mu.OracleTracker(weights).ref.thr
    fx = dict(config="tiny", frame_w=W, frame_h=H, square=SQ, seed=SEED, period=PERIOD, step=STEP, n=N, hide=np.array(HIDE, np.int32),
              policy=np.array(POLICY, np.int32), weights_sha256=sha256_file(weights), threshold=np.float32(thr),
              times=np.array(ts, np.int32), box0=np.array(sc.gt_box(0), np.int32), gt=gt, hidden=hidden,
              bbox=bbox, score=np.array([r.score for r in res], np.float32), success=np.array([int(r.success) for r in res], np.int8),
              idx=np.array([r.idx for r in res], np.int32), state_box=np.array(boxes, np.float32),
              rec_words=np.array([r.words() for r in recs], np.uint32), margin=np.array(trk.margins, np.float64), faint=FAINT,
              plain_bbox=np.array([r.bbox for r in pres], np.int32), plain_score=np.array([r.score for r in pres], np.float32),
              plain_success=np.array([int(r.success) for r in pres], np.int8), plain_state_box=np.array(pboxes, np.float32),
              min_iou=np.float64(ious[hidden == 0].min()))
    check(fx)
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out)} bytes); min IoU on visible frames {float(fx['min_iou']):.3f}, "
          f"scores {fx['score'].min():.3f} .. {fx['score'].max():.3f} (threshold {thr:.2f}), "
          f"max |v| {np.abs(fx['rec_words'][:, 0:2].view(np.float32)).max():.1f} px")


if __name__ == "__main__":
    run(OUT)
