"""Generates the committed fixture of the reacquire-proposals tests (tests/test_proposals_cases.py,
tests/test_gpu_proposals.py): the re-acquisition clip of make_reacquire.py, found again through the proposals instead of
the scan. CPU only: the NumPy model of tests/proposals_util.py and the unchanged oracle (oracle/vit_ref.py).

  python tests/golden/make_proposals.py      -> tests/golden/proposals_cfg2.npz   (about a dozen oracle updates)

Recorded:
  state_box       the oracle's box behind the failed plain update on frame 3 (a failed update leaves it alone)
  c, grid, pattern_side
  proposal_*      what the model lists on frame 3 from the oracle's template rows, default policy (4 proposals, 0.5)
  runner_up_sim   the second-best similarity at threshold 0 (the best place outside proposal 0's suppression square)
  cand_*          one candidate pass over the listed boxes: each slot an independent oracle update around its box
  winner          the slot with the greatest score; its box becomes the state
  track_*         five closed-loop frames behind it (frames 4..8), with the ground truth

The conditions the tests rely on are asserted here (check, margins): proposal 0's centre within one cell side of the
ground truth's, sim[0] >= 0.8, the runner-up <= 0.5, the winner succeeds on the ground truth within 1 px, the oracle keeps
the target. Measured: sim[0] = 0.9471 at (416, 752) against the ground truth (413, 754); the runner-up at threshold 0 is
0.2304, so the default policy lists ONE proposal and the candidate pass has one slot. (With the cells outside the frame
compared as black pixels instead of left out, three frame corners scored 0.512 - 0.508: the reason the rule leaves them
out.)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import proposals_util as pu  # noqa: E402
from oracle import vit_ref as R  # noqa: E402
import gstreamer_vit_tracker_amd as vt  # noqa: E402  (weights writer + synthetic clip only)

sys.path.insert(0, HERE)
import make_reacquire as mr  # noqa: E402

TRACK = 5


def check(fx):
    c = float(fx["c"])
    gt = fx["gt_box"].astype(np.float64)
    b0 = fx["proposal_box"][0].astype(np.float64)
    assert abs(b0[0] + b0[2] / 2 - gt[0] - gt[2] / 2) <= c and abs(b0[1] + b0[3] / 2 - gt[1] - gt[3] / 2) <= c, "proposal 0 is off"
    assert int(fx["plain_success"]) == 0
    w = int(fx["winner"])
    assert fx["cand_success"][w] != 0 and np.abs(fx["cand_bbox"][w] - fx["gt_box"]).max() <= 1
    assert np.all(np.abs(fx["cand_score"] - float(fx["threshold"])) > mr.THRESHOLD_GAP)
    assert np.all(fx["track_success"] != 0)
    assert min(mr.iou(b, g) for b, g in zip(fx["track_bbox"], fx["track_gt"])) > 0.5


def margins(fx):
    s0, s1 = float(fx["proposal_sim"][0]), float(fx["runner_up_sim"])
    assert s0 >= 0.8 and s1 <= 0.5, f"the specified margins do not hold: sim[0] = {s0:.4f} (>= 0.8), sim[1] = {s1:.4f} (<= 0.5)"


def run(out):
    cfg = "cfg2"
    weights = vt.weights.ensure_weights(cfg)
    frame, gt = mr.clip()
    W, H, J = mr.W, mr.H, mr.JUMP_AT
    trk = R.VitTrackRef(weights)
    fr = lambda t: R.Frame.nv12(frame(t), W, H)   # noqa: E731
    trk.init(fr(0), gt(0))
    for t in range(J):
        trk.update(fr(t))
    f3 = fr(J)
    plain = trk.update(f3)
    state = trk.box.copy()
    m = trk.m
    rgb = pu.to_rgb("nv12", frame(J), W, H)
    na, nb = m.hdr["norm_a"], m.hdr["norm_b"]
    ev = pu.evaluate(rgb, state, trk.tpl, m.T, m.patch, na, nb)
    assert ev["status"] == 1
    p = ev["proposals"]
    loose = pu.listing(ev["map"], ev["M"], dict(c=ev["c"], X0=ev["X0"]), state, 2, 0.0)
    runner = float(loose["sim"][1]) if len(loose) > 1 else 0.0
    print(f"plain {plain}; c {ev['c']} grid {ev['Wg']}x{ev['Hg']}; proposals {[(float(s), b.tolist()) for s, b in zip(p['sim'], p['box'])]}; "
          f"runner-up at threshold 0: {runner:.4f}; ground truth {gt(J)}", flush=True)
    cand = dict(score=[], success=[], bbox=[])
    for b in p["box"]:
        trk.box = b.astype(np.float32).copy()
        r = trk.update(f3)
        trk.box = state.copy()
        cand["score"].append(r.score); cand["success"].append(int(r.success)); cand["bbox"].append(r.bbox)
    win = mr.winner_of(cand["score"])
    print(f"candidates {list(zip(cand['score'], cand['success'], cand['bbox']))} winner {win}", flush=True)
    trk.box = np.array(cand["bbox"][win], np.float32)
    track = dict(bbox=[], score=[], success=[], gt=[])
    for t in range(J + 1, J + 1 + TRACK):
        r = trk.update(fr(t))
        track["bbox"].append(r.bbox); track["score"].append(r.score); track["success"].append(int(r.success)); track["gt"].append(gt(t))
    fx = dict(config=cfg, weights_sha256=mr.sha256_file(weights), threshold=np.float32(trk.thr), jump_at=J,
              state_box=state.astype(np.float32), gt_box=np.array(gt(J), np.int32), plain_success=np.int8(plain.success),
              plain_score=np.float32(plain.score), c=np.float32(ev["c"]), grid=np.array([ev["Wg"], ev["Hg"]], np.int32),
              pattern_side=np.int32(ev["M"]), proposal_sim=p["sim"].copy(), proposal_box=p["box"].copy(), proposal_pos=p["pos"].copy(),
              runner_up_sim=np.float32(runner), cand_score=np.array(cand["score"], np.float32),
              cand_success=np.array(cand["success"], np.int8), cand_bbox=np.array(cand["bbox"], np.int32), winner=np.int32(win),
              track_bbox=np.array(track["bbox"], np.int32), track_score=np.array(track["score"], np.float32),
              track_success=np.array(track["success"], np.int8), track_gt=np.array(track["gt"], np.int32))
    check(fx)
    margins(fx)
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)", flush=True)


if __name__ == "__main__":
    run(os.path.join(HERE, "proposals_cfg2.npz"))
