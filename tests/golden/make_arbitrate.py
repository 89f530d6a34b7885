"""Generates the committed oracle fixture of the peak-arbitration tests (tests/test_arbitrate_cases.py). CPU oracle only
(oracle/vit_ref.py + oracle/vt_oracle.c, both unchanged), decided by tests/arbitrate_util.py.

  python tests/golden/make_arbitrate.py      -> tests/golden/arbitrate_tiny.npz   (seconds)

The scene, 640 x 360, the `tiny` weights (grid 8, template 64, search 128): the seeded background of
synth.MovingSquare(seed 0); a 48-px target with MovingSquare's texture (u 90, v 200) at (200 + 3 t, 150); the 100 % grey
checkerboard of make_appearance.py (12-px cells, luma 255 / 145, neutral chroma), stationary at LOOKALIKE; the target is absent
on frames HIDE[0] <= t < HIDE[1]. The frames are regenerated from these parameters (frame()), never stored.

Two oracle runs over N frames (frame 0 initialises and is the first update's frame, as in template_refresh_util.drive):
`plain`, the oracle as it is, and `arb`, the oracle with the arbitration rule applied behind every update - the lists of
peaks_util.iterate_oracle under (K, R, min_resp), the template crops at the peaks' integer boxes scored against the frame-0
anchor, arbitrate_util.examine / commit, and on a switch the box the next search crop is cut around set to the chosen peak's
integer box. Recorded per update: both runs' boxes, scores and success, the arbitrated run's record (status, n, chosen, per peak
cell, score, response, similarity, status, float box) and the best response the list did not take.

The conditions that keep the tests from being vacuous are asserted here (check()), and again on the committed file by
tests/test_arbitrate_cases.py. The file records the SHA-256 of the weight blob it was made with.
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
import arbitrate_util as ar  # noqa: E402
import peaks_util as pk  # noqa: E402

W, H, SQ, SEED = 640, 360, 48, 0
TARGET0, SPEED, TARGET_Y = 200, 3, 150
LOOKALIKE = (380, 204)     # at (380, 206) a listed response leads the next cell by 7e-4, below peaks_util.MARGIN
HIDE = (40, 66)
N = 100
POLICY = dict(on=1, max_peaks=3, radius=1, min_resp_pm=50, low_pm=300, high_pm=500)
SIM_GAP = 0.01
OUT = os.path.join(HERE, "arbitrate_tiny.npz")


def checkerboard():
    yy, xx = np.mgrid[0:SQ, 0:SQ]
    return np.where(((yy // 12) + (xx // 12)) % 2 == 0, 255, 145).astype(np.uint8)


def target_box(t, p=None):
    p = p or dict(target0=TARGET0, speed=SPEED, target_y=TARGET_Y, square=SQ)
    return (int(p["target0"]) + int(p["speed"]) * t, int(p["target_y"]), int(p["square"]), int(p["square"]))


def frame(t, p=None):
    """RGB8 frame t of the scene with the parameters p (a fixture's, or this file's)"""
    p = p or dict(frame_w=W, frame_h=H, square=SQ, seed=SEED, target0=TARGET0, speed=SPEED, target_y=TARGET_Y, lookalike=LOOKALIKE, hide=HIDE)
    w, h, sq = int(p["frame_w"]), int(p["frame_h"]), int(p["square"])
    sc = vt.synth.MovingSquare(w, h, sq, seed=int(p["seed"]))
    yy = sc.bg_y.copy()
    uv = np.full(((h + 1) // 2, (w + 1) // 2, 2), 128, np.uint8)
    lx, ly = (int(v) for v in p["lookalike"])
    yy[ly:ly + sq, lx:lx + sq] = checkerboard()
    if not (int(p["hide"][0]) <= t < int(p["hide"][1])):
        x, y, _, _ = target_box(t, p)
        yy[y:y + sq, x:x + sq] = sc.sq_y
        uv[y // 2:(y + sq + 1) // 2, x // 2:(x + sq + 1) // 2, 0] = sc.sq_u
        uv[y // 2:(y + sq + 1) // 2, x // 2:(x + sq + 1) // 2, 1] = sc.sq_v
    return vt.synth.nv12_planes_to_rgb8(yy, uv.reshape(uv.shape[0], -1)[:, :w], w, h)


def iou(a, b):
    ix = max(0, min(a[0] + a[2], b[0] + b[2]) - max(a[0], b[0]))
    iy = max(0, min(a[1] + a[3], b[1] + b[3]) - max(a[1], b[1]))
    u = a[2] * a[3] + b[2] * b[3] - ix * iy
    return ix * iy / u if u > 0 else 0.0


def first_on_target(boxes, p=None):
    """the first frame behind the occlusion whose box has IoU >= 0.5 with the target's (len(boxes) where there is none)"""
    hide1 = HIDE[1] if p is None else int(p["hide"][1])
    for t in range(hide1, len(boxes)):
        if iou(tuple(int(v) for v in boxes[t]), target_box(t, p)) >= 0.5:
            return t
    return len(boxes)


def sha256_file(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    return h.hexdigest()


def check(fx):
    """the conditions the tests rely on; AssertionError names the one that does not hold"""
    st = fx["arb_status"]
    assert int((st == ar.SWITCHED).sum()) >= 1, "no switch in the arbitrated run"
    plain, arb = first_on_target(fx["plain_bbox"], fx), first_on_target(fx["arb_bbox"], fx)
    assert arb < plain, f"the arbitrated run is back on the target at {arb}, the plain run at {plain}"
    assert (int(fx["first_plain"]), int(fx["first_arb"])) == (plain, arb), "the recorded recovery frames"
    low, high = float(ar.threshold(int(fx["low_pm"]))), float(ar.threshold(int(fx["high_pm"])))
    due = (st == ar.KEPT) | (st == ar.SWITCHED)
    cmp0 = fx["arb_sim"][due, 0]
    assert np.all(np.abs(cmp0 - low) >= SIM_GAP), "a similarity of peak 0 lies within 0.01 of low"
    challenged = due & (fx["arb_sim"][:, 0] < low)
    run = fx["arb_peak_status"][challenged, 1:] == ar.P_SCORED
    assert np.all(np.abs(fx["arb_sim"][challenged, 1:][run] - high) >= SIM_GAP), "a runner-up's similarity lies within 0.01 of high"
    assert float(fx["lead_min"]) >= pk.MARGIN and float(fx["thr_min"]) >= pk.MARGIN, "a listed response misses peaks_util.MARGIN"


def run(out: str):
    from oracle import vit_ref as o
    weights = vt.weights.ensure_weights("tiny")
    m = o.Model(weights)
    T, S, cols, grid = m.T, m.S, 3 * m.patch * m.patch, m.gs
    hann = np.ascontiguousarray(m.t["hann"].reshape(-1), np.float32)
    frames = [frame(t) for t in range(N)]
    box0 = target_box(0)

    def crop(rgb, box):
        return o.preproc(o.Frame.rgb8(rgb), np.asarray(box, np.float32), 2.0, T, m.patch, m.kpad, m.hdr["norm_a"], m.hdr["norm_b"])
    anchor = crop(frames[0], box0)

    def drive(arbitrate):
        ref = o.VitTrackRef(weights)
        ref.init(o.Frame.rgb8(frames[0]), box0)
        rows = []
        for t in range(N):
            r = ref.update(o.Frame.rgb8(frames[t]), taps=True)
            rec = dict(bbox=r.bbox, score=r.score, success=int(r.success), status=0, n=0, chosen=0)
            if arbitrate:
                lg = np.ascontiguousarray(ref.last["head_out"], np.float32)[None, :, :5]
                geo = np.asarray(ref.last["geo"], np.float32)
                lst = ar.lists(lg, hann, grid, geo[None], [W], [H], POLICY["max_peaks"], POLICY["radius"], POLICY["min_resp_pm"])
                lead, thr = pk.margins(lg, hann, grid, POLICY["max_peaks"], POLICY["radius"], float(ar.threshold(POLICY["min_resp_pm"])))
                state = dict(frames_done=t + 1, window_miss=0, geo=geo)
                d = ar.decide(lst, 0, lambda k, ib: ar.similarity(anchor, crop(frames[t], ib), cols), state=state, success=int(r.success),
                              frame_wh=(W, H), T=T, S=S, success_threshold=ref.thr, policy=POLICY)
                rec.update(status=d["status"], n=d["n"], chosen=d["chosen"], peak_status=d["peak_status"], sim=[float(v) for v in d["sim"]],
                           cell=lst["cell"][0], pscore=lst["score"][0], resp=lst["resp"][0], fbox=lst["fbox"][0], lead=lead[0], thr=thr[0])
                if d["status"] == ar.SWITCHED:
                    k = d["chosen"]
                    ib = ar.int_box(lst["fbox"][0, k])
                    ref.box = ib.copy()          # what vt_group_set_state_box does: the next search crop is cut around it
                    rec.update(bbox=tuple(int(v) for v in ib), score=float(lst["score"][0, k]), success=1)
            rows.append(rec)
        return rows

    plain, arb = drive(False), drive(True)
    K = ar.KMAX

    def col(name, dtype, width=None):
        a = np.zeros((N,) + ((K,) if width is None else width), dtype)
        for t, r in enumerate(arb):
            if name in r:
                v = np.asarray(r[name])
                a[t, :v.shape[0]] = v
        return a
    fx = dict(config="tiny", frame_w=W, frame_h=H, square=SQ, seed=SEED, weights_sha256=sha256_file(weights), target0=TARGET0, speed=SPEED,
              target_y=TARGET_Y, lookalike=np.array(LOOKALIKE, np.int32), hide=np.array(HIDE, np.int32), n_frames=N,
              box0=np.array(box0, np.int32), **POLICY,
              plain_bbox=np.array([r["bbox"] for r in plain], np.int32), plain_score=np.array([r["score"] for r in plain], np.float32),
              plain_success=np.array([r["success"] for r in plain], np.int8),
              arb_bbox=np.array([r["bbox"] for r in arb], np.int32), arb_score=np.array([r["score"] for r in arb], np.float32),
              arb_success=np.array([r["success"] for r in arb], np.int8), arb_status=np.array([r["status"] for r in arb], np.int8),
              arb_n=np.array([r["n"] for r in arb], np.int8), arb_chosen=np.array([r["chosen"] for r in arb], np.int8),
              arb_peak_status=col("peak_status", np.int8), arb_sim=col("sim", np.float32), arb_cell=col("cell", np.int32),
              arb_peak_score=col("pscore", np.float32), arb_resp=col("resp", np.float32), arb_fbox=col("fbox", np.float32, (K, 4)),
              lead_min=np.float64(min(r["lead"] for r in arb if "lead" in r)), thr_min=np.float64(min(r["thr"] for r in arb if "thr" in r)))
    fx["first_plain"], fx["first_arb"] = first_on_target(fx["plain_bbox"], fx), first_on_target(fx["arb_bbox"], fx)
    for t in np.flatnonzero(fx["arb_status"] >= 1):
        print(t, int(fx["arb_status"][t]), int(fx["arb_chosen"][t]), np.round(fx["arb_sim"][t, :int(fx["arb_n"][t])], 3),
              np.round(fx["arb_peak_score"][t, :int(fx["arb_n"][t])], 3), fx["arb_peak_status"][t])
    print("plain back on the target at", fx["first_plain"], "arbitrated at", fx["first_arb"], "lead", fx["lead_min"], "thr", fx["thr_min"])
    check(fx)
    np.savez_compressed(out, **fx)
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    run(OUT)
