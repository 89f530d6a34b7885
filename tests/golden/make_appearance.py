"""Generates the committed oracle fixture of the appearance-check tests (tests/test_appearance_cases.py,
tests/test_gpu_appearance.py). CPU oracle only (oracle/vit_ref.py + oracle/vt_oracle.c, both unchanged), scored by
tests/appearance_util.py.

  python tests/golden/make_appearance.py      -> tests/golden/appearance_tiny.npz   (seconds)

Part 1, the table of the signal (MovingSquare 640 x 360, 48-px target, the `tiny` weights: template 64, patch 16). The
anchor is the template crop of frame 0 at the ground-truth box; a probe is the same crop of another frame or box:
`same` (the moving target on frames 1..40 at its ground-truth box), `offset` (frame 0, the box shifted by 1 / 2 / 4 / 8
px in x), `blend` (frame 0, the target blended 25 / 50 / 75 / 100 % towards a grey checkerboard of similar brightness:
12-px cells of luma 200 +- 55, neutral chroma) and `absent` (frame 0 without the target). The rows of the anchor and of
one probe per case are committed, with the similarities measured here. A checkerboard in the target's own colours stays
above 0.92 at 100 %: the crop is half background, and bright-on-dark carries most of the correlation.

Part 2, the gate clip: 37 frames (init + 36 updates) of the same scene whose target alternates, in segments of 6 updates,
between its own texture and the impostor (the 100 % checkerboard, which the oracle tracks at scores of 0.56 - 0.63
against 0.60 - 0.71 on the target itself). Driven through the oracle with the refresh rule of
period 2 and the gate at 900 per mille (appearance_util.Rule; a refresh is ref.init(frame, result.bbox)): the own
segments refresh, the impostor segments are gated. Recorded per update: the oracle's box, score and success, the
similarity of the probe at that box against the anchor, and what the rule did.

The conditions that keep the tests from being vacuous are asserted here (check()), and again on the committed file by
tests/test_appearance_cases.py. The file records the SHA-256 of the weight blob it was made with.
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
import appearance_util as au  # noqa: E402

W, H, SQ, SEED = 640, 360, 48, 0
OFFSETS = (1, 2, 4, 8)
BLENDS = (25, 50, 75, 100)
N_SAME = 40
SEG, N_UPDATES = 6, 36
PERIOD, GATE_PM = 2, 900
TAU_GAP = 0.01
OUT = os.path.join(HERE, "appearance_tiny.npz")


def checkerboard():
    yy, xx = np.mgrid[0:SQ, 0:SQ]
    return np.where(((yy // 12) + (xx // 12)) % 2 == 0, 255, 145).astype(np.uint8)


def scene(blend_pct=0, hide=None):
    """the scene with the target blended blend_pct % towards the grey checkerboard: luma and both chroma values"""
    sc = vt.synth.MovingSquare(W, H, SQ, seed=SEED, hide=hide)
    if blend_pct:
        own = sc.sq_y.astype(np.int32)
        sc.sq_y = ((own * (100 - blend_pct) + checkerboard().astype(np.int32) * blend_pct + 50) // 100).astype(np.uint8)
        sc.sq_u = (sc.sq_u * (100 - blend_pct) + 128 * blend_pct + 50) // 100
        sc.sq_v = (sc.sq_v * (100 - blend_pct) + 128 * blend_pct + 50) // 100
    return sc


def impostor_at(i):
    """frame i of the gate clip (0 = the init frame) shows the impostor"""
    return i >= 1 and ((i - 1) // SEG) % 2 == 1


def gate_clip():
    """-> (ground-truth box of frame 0, the RGB8 frames of the gate clip)"""
    own, imp = scene(), scene(100)
    return own.gt_box(0), [(imp if impostor_at(i) else own).frame_rgb8(i) for i in range(N_UPDATES + 1)]


def sha256_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.hexdigest()


def check(fx):
    """the conditions the tests rely on; AssertionError names the one that does not hold"""
    tau = float(fx["gate_pm"]) / 1000.0
    act = fx["gate_action"]
    assert int((act == 1).sum()) >= 3 and int((act == 2).sum()) >= 3, "fewer than 3 refreshes or fewer than 3 gated refreshes"
    ev = fx["gate_due"] != 0
    assert np.all(np.abs(fx["gate_sim"][ev] - tau) > TAU_GAP), "an evaluated similarity lies within 0.01 of tau"
    imp = fx["gate_impostor"] != 0
    assert np.all(fx["gate_success"][imp] != 0), "the oracle fails on an impostor frame"
    assert np.all(fx["gate_success"] != 0), "the oracle fails on a frame of the gate clip"
    assert np.all(act[imp] != 1), "a refresh fired on the impostor"
    assert np.all(act[~imp & (act != 0)] == 1), "a refresh was gated on the target's own texture"


def run(out: str):
    from oracle import vit_ref as o
    import template_refresh_util as tu
    weights = vt.weights.ensure_weights("tiny")
    ref = o.VitTrackRef(weights)
    m = ref.m
    T, cols = m.T, 3 * m.patch * m.patch

    def crop(rgb, box):
        return o.preproc(o.Frame.rgb8(rgb), np.asarray(box, np.float32), 2.0, T, m.patch, m.kpad, m.hdr["norm_a"], m.hdr["norm_b"])

    def sim(a, p):
        return float(au.score(a, p, cols)["similarity"])

    # ---- part 1 ----
    sc = scene()
    box0 = sc.gt_box(0)
    f0 = sc.frame_rgb8(0)
    anchor = crop(f0, box0)
    same = [crop(sc.frame_rgb8(t), sc.gt_box(t)) for t in range(1, N_SAME + 1)]
    offs = [crop(f0, (box0[0] + d, box0[1], box0[2], box0[3])) for d in OFFSETS]
    blends = [crop(scene(b).frame_rgb8(0), box0) for b in BLENDS]
    absent = crop(scene(hide=(0, 1 << 30)).frame_rgb8(0), box0)
    same_sim = np.array([sim(anchor, p) for p in same])
    # ---- part 2 ----
    gbox0, frames = gate_clip()
    trk = tu.OracleTracker(weights)
    rule = au.Rule(m.T, m.S, PERIOD, 0.0, GATE_PM)
    trk.init(frames[0], gbox0)
    g_anchor = crop(frames[0], gbox0)
    rows = []
    for i in range(1, N_UPDATES + 1):
        pre = np.array(trk.box(), np.float32)
        last = rule.last_frame
        r = trk.update(frames[i])
        s = sim(g_anchor, crop(frames[i], r.bbox))
        is_due = au.due(rule, r, rule.done + 1, last, 1)
        act = rule.step(r, pre_box=pre, record=(1, s))
        if act == "fire":
            trk.init(frames[i], tuple(int(v) for v in r.bbox))
        rows.append((r.bbox, r.score, int(r.success), s, {None: 0, "fire": 1, "gate": 2, "skip": 3}[act], int(is_due),
                     int(impostor_at(i))))
    fx = dict(config="tiny", frame_w=W, frame_h=H, square=SQ, seed=SEED, weights_sha256=sha256_file(weights),
              box0=np.array(box0, np.int32), cols=cols, anchor=anchor, offsets=np.array(OFFSETS, np.int32),
              offset_rows=np.array(offs), blends=np.array(BLENDS, np.int32), blend_rows=np.array(blends), absent_rows=absent,
              same_last_rows=same[-1], same_sim=same_sim,
              offset_sim=np.array([sim(anchor, p) for p in offs]), blend_sim=np.array([sim(anchor, p) for p in blends]),
              absent_sim=np.float64(sim(anchor, absent)),
              seg=SEG, n_updates=N_UPDATES, period=PERIOD, gate_pm=GATE_PM,
              gate_bbox=np.array([r[0] for r in rows], np.int32), gate_score=np.array([r[1] for r in rows], np.float32),
              gate_success=np.array([r[2] for r in rows], np.int8), gate_sim=np.array([r[3] for r in rows], np.float64),
              gate_action=np.array([r[4] for r in rows], np.int8), gate_due=np.array([r[5] for r in rows], np.int8),
              gate_impostor=np.array([r[6] for r in rows], np.int8))
    check(fx)
    np.savez_compressed(out, **fx)
    imp = fx["gate_impostor"] != 0
    print(f"wrote {out} ({os.path.getsize(out)} bytes); same {same_sim.min():.3f} .. {same_sim.max():.3f}, offsets "
          f"{np.round(fx['offset_sim'], 3)}, blends {np.round(fx['blend_sim'], 3)}, absent {float(fx['absent_sim']):.3f}; gate clip: "
          f"{int((fx['gate_action'] == 1).sum())} refreshed, {int((fx['gate_action'] == 2).sum())} gated, similarity "
          f"{fx['gate_sim'][~imp].min():.3f} .. {fx['gate_sim'][~imp].max():.3f} on the target, "
          f"{fx['gate_sim'][imp].min():.3f} .. {fx['gate_sim'][imp].max():.3f} on the impostor")


if __name__ == "__main__":
    run(OUT)
