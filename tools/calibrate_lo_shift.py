#!/usr/bin/env python3
"""Choose a weight blob's lo_shift (the residual pair's quantum 2^-s) from what its residual stream
really holds: run a clip through a single-stream engine with taps, print the per-stage range report
(Group.residual_range) and weights.recommend_lo_shift's answer; --write stamps the blob in place.

  python tools/calibrate_lo_shift.py BLOB                          # synth.MovingSquare, 8 frames
  python tools/calibrate_lo_shift.py BLOB --nv12 clip.nv12 --size 1920x1080 --box 900,500,64,64 --write
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import gstreamer_vit_tracker_amd as vt  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("blob")
    ap.add_argument("--nv12", help="raw NV12 frames, back to back (default: a synthetic moving square)")
    ap.add_argument("--size", default="640x480", help="WxH of the frames")
    ap.add_argument("--box", help="x,y,w,h of the target in the first frame (required with --nv12)")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--write", action="store_true", help="stamp the blob with the recommendation")
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    if a.nv12:
        if not a.box:
            ap.error("--nv12 needs --box")
        raw = np.fromfile(a.nv12, np.uint8)
        n = min(a.frames, raw.size // (w * h * 3 // 2))
        if n < 2:
            ap.error("the file holds fewer than two frames of that size")
        frames = [raw[i * (w * h * 3 // 2):(i + 1) * (w * h * 3 // 2)] for i in range(n)]
        box = tuple(int(v) for v in a.box.split(","))
    else:
        sc = vt.synth.MovingSquare(w, h, 64, seed=2)
        frames = [sc.frame_nv12(t) for t in range(a.frames)]
        box = sc.gt_box(0)
    grp = vt.Group(a.blob, n_streams=1)
    grp.enable_taps(True)
    rows = []
    for t, buf in enumerate(frames):
        f = vt.NV12Frame(buf, w, h)
        if t == 0:
            grp.init_host(0, f, vt.BBox.new(*box))
        grp.update_host([f])
        rows.append(grp.residual_range(0))
    stages = [r["stage"] for r in rows[0]]
    worst = []          # per stage, the worst of every frame
    for i, st in enumerate(stages):
        rs = [fr[i] for fr in rows]
        worst.append(dict(stage=st, lo_shift=rs[0]["lo_shift"], max_abs=max(r["max_abs"] for r in rs),
                          n_sat=max(r["n_sat"] for r in rs),
                          n_ge_pow2=[max(r["n_ge_pow2"][k] for r in rs) for k in range(9)]))
    print(f"{a.blob}: lo_shift {worst[0]['lo_shift']}, {len(frames)} frames; per stage, the worst frame")
    print(f"{'stage':>9} {'max |x|':>10} {'|lo8|=127':>10} " + " ".join(f"{'>=2^%d' % k:>7}" for k in range(1, 10)))
    for r in worst:
        print(f"{r['stage']:>9} {r['max_abs']:10.4f} {r['n_sat']:10d} " + " ".join(f"{v:7d}" for v in r["n_ge_pow2"]))
    s = vt.weights.recommend_lo_shift(worst)
    print(f"recommended lo_shift: {s} (exact for |x| < {2 ** (15 - s)})")
    if a.write:
        vt.weights.set_lo_shift(a.blob, 0 if s == vt.weights.LO_SHIFT_DEFAULT else s)
        print(f"stamped {a.blob}")


if __name__ == "__main__":
    main()
