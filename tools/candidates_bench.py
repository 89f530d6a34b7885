"""What a candidate pass costs, and what re-acquisition by scanning costs (run on the GPU box):

    python tools/candidates_bench.py [--repo DIR] [--cfg cfg3] [--group 30] [--n 1,4,8,15,30] [--steps 20] [--reps 3] [--out F.json]

--repo DIR imports the package (and its built library) from another checkout, e.g. the parent commit's: the tool
measures what that checkout has. Everything is synchronous calls (update = enqueue + wait) timed by the wall clock
after a warm-up, median of --reps with every run listed; 1920x1080 NV12, 64-px targets.

  subset_dev / subset_host     vt_group_update_{device,host}_streams over n distinct streams of the group
  cand_dev                     a candidate pass of n slots, all for ONE stream (scan windows of the grid), device frame
  cand_host_shared / _distinct the same on host frames: the n slots name one frame (staged once, as the bounding
                               rectangle of their windows) / n copies of it (every window staged on its own)
  reacquire_*                  Group.reacquire on the jump frame of tests/golden/make_reacquire.py's clip (112 windows,
                               found in the third 30-slot chunk) and on a frame without the target (all four chunks)
  by_hand_*                    the alternative without candidate passes: vt_group_set_state_box + a one-stream
                               update, window by window, until the first success (73 windows) / over all 112

The standalone time of the two candidate kernels comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python tools/candidates_bench.py --n 30 --steps 5 --reps 1 --skip-reacquire)."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--cfg", default="cfg3")
    ap.add_argument("--group", type=int, default=30)
    ap.add_argument("--n", default="1,4,8,15,30")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-reacquire", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    import torch
    import gstreamer_vit_tracker_amd as vt
    have = hasattr(vt.Group, "update_device_candidates")
    ns = [int(v) for v in a.n.split(",")]
    G, w, h = a.group, 1920, 1080
    weights = vt.weights.ensure_weights(a.cfg)
    scs = [vt.synth.MovingSquare(w, h, 64, seed=100 + i) for i in range(G)]
    host = [vt.NV12Frame(sc.frame_nv12(1), w, h) for sc in scs]
    dbuf = [torch.from_numpy(f.buf).cuda() for f in host]
    dev = [vt.frame_nv12(b.data_ptr(), b.data_ptr() + w * h, w, h) for b in dbuf]
    grp = vt.Group(weights, n_streams=G)
    for i, sc in enumerate(scs):
        f0 = torch.from_numpy(sc.frame_nv12(0)).cuda()
        grp.init_device(i, vt.frame_nv12(f0.data_ptr(), f0.data_ptr() + w * h, w, h), vt.BBox.new(*sc.gt_box(0)))
    caps = grp.graph_captures()

    def grid(bw=64.0, bh=64.0):
        if have:
            return vt.scan_windows(w, h, bw, bh)
        side = 4.0 * (bw * bh) ** 0.5

        def axis(L):
            n = int(np.ceil((L - side) / (side / 2))) + 1
            return [side / 2 + i * (L - side) / (n - 1) for i in range(n)]
        return np.array([(cx - bw / 2, cy - bh / 2, bw, bh) for cy in axis(h) for cx in axis(w)], np.float32)

    boxes = grid()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    rows = []
    for n in ns:
        L = list(range(1, n)) + [0] if n > 1 else [0]            # never the identity list: eager launches, like a candidate pass
        kinds = {"subset_dev": lambda: grp.update_device([dev[s] for s in L], streams=L),
                 "subset_host": lambda: grp.update_host([host[s] for s in L], streams=L)}
        if have:
            cands = [(0, b) for b in boxes[40:40 + n]]
            copies = [vt.NV12Frame(host[0].buf.copy(), w, h) for _ in range(n)]
            kinds.update({"cand_dev": lambda: grp.update_device_candidates(cands, [dev[0]] * n),
                          "cand_host_shared": lambda: grp.update_host_candidates(cands, [host[0]] * n),
                          "cand_host_distinct": lambda: grp.update_host_candidates(cands, copies)})
        m = {k: [] for k in kinds}
        for _ in range(a.reps):
            for k, fn in kinds.items():
                m[k].append(timed(fn))
        row = {"n": n}
        for k, v in m.items():
            row[k + "_ms"], row[k + "_ms_all"] = float(np.median(v)), [round(x, 4) for x in v]
        rows.append(row)
        print(f"n {n:3d}: " + "  ".join(f"{k} {row[k + '_ms']:.3f} {row[k + '_ms_all']}" for k in kinds), flush=True)
    res = {"cfg": a.cfg, "group": G, "frame": [w, h], "steps": a.steps, "warmup": a.warmup, "reps": a.reps,
           "candidates": have, "build": vt.build_info(), "rows": rows}

    if not a.skip_reacquire:
        sc_a = vt.synth.MovingSquare(w, h, 64, seed=0)
        sc_b = vt.synth.MovingSquare(w, h, 64, seed=0, center=(0.23 * w, 0.71 * h), amp=0.05 * min(w, h))
        sc_gone = vt.synth.MovingSquare(w, h, 64, seed=0, hide=(1, 1 << 30))
        hf = {"found": vt.NV12Frame(sc_b.frame_nv12(3), w, h), "absent": vt.NV12Frame(sc_gone.frame_nv12(3), w, h)}
        dt = {k: torch.from_numpy(f.buf).cuda() for k, f in hf.items()}
        df = {k: vt.frame_nv12(t.data_ptr(), t.data_ptr() + w * h, w, h) for k, t in dt.items()}
        f0 = torch.from_numpy(sc_a.frame_nv12(0)).cuda()
        init = lambda: grp.init_device(0, vt.frame_nv12(f0.data_ptr(), f0.data_ptr() + w * h, w, h), vt.BBox.new(*sc_a.gt_box(0)))  # noqa: E731
        timing = {}

        def by_hand(frame):
            for i, b in enumerate(boxes):
                grp.set_state_box(0, b)
                r = grp.update_device([frame], streams=[0])[0]
                if r.success:
                    return i + 1, r
            return len(boxes), r

        for case in ("found", "absent"):
            runs = {"by_hand_" + case: []}
            if have:
                runs.update({"reacquire_dev_" + case: [], "reacquire_host_" + case: []})
            for _ in range(a.reps + 1):         # the first repetition warms up and is dropped
                init()
                t0 = time.perf_counter()
                tried, r = by_hand(df[case])
                runs["by_hand_" + case].append((time.perf_counter() - t0) * 1e3)
                timing["by_hand_" + case + "_windows"], timing["by_hand_" + case + "_result"] = tried, repr(r)
                if have:
                    for key, frame, is_host in (("reacquire_dev_", df[case], False), ("reacquire_host_", hf[case], True)):
                        init()
                        t0 = time.perf_counter()
                        r = grp.reacquire(0, frame, box_wh=(64, 64), host=is_host)
                        runs[key + case].append((time.perf_counter() - t0) * 1e3)
                        timing[key + case + "_chunks"], timing[key + case + "_result"] = len(grp.last_scan), repr(r)
            for k, v in runs.items():
                timing[k + "_ms"], timing[k + "_ms_all"] = float(np.median(v[1:])), [round(x, 3) for x in v[1:]]
                print(f"{k}: {timing[k + '_ms']:.2f} ms {timing[k + '_ms_all']}", flush=True)
        print({k: v for k, v in timing.items() if not k.endswith("_ms") and not k.endswith("_all")}, flush=True)
        res["reacquire"] = timing
    assert grp.graph_captures() == caps, "a capture happened inside an update"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    grp.close()


if __name__ == "__main__":
    main()
