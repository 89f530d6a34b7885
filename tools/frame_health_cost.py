"""Frame health: what the four launches of k_health.hip take on 30 device-resident 1080p NV12 frames (the cfg3 x 30 shape
of a pass), alone, through the operator hook; inside a pass: tools/frame_health_engine_cost.py.
usage: rocprofv3 --kernel-trace --output-format csv -d DIR -o health -- python tools/frame_health_cost.py TREE_ROOT run
       python tools/frame_health_cost.py TREE_ROOT report DIR
run: 30 streams, max_cells 65536 (the automatic cell is 8: 240 x 135 = 32,400 cells per stream), in this order: 2 warm-up
calls, then REPS calls each of
  due      every stream measured and compared (status 1; the frames alternate between two pictures)
  period   "health_period" 30 with frames_done = 1: nobody is due
  off      "health" 0
report: reads the kernel trace of such a run; every call dispatches the four launches once, so dispatch k of a kernel
belongs to call k. Prints, per case and launch, the median begin -> end time [and the minimum] and their sum per call."""
import csv
import glob
import os
import sys

REPS = 20
CASES = ("due", "period", "off")
KERNELS = ("health_prepare", "health_thumb", "health_measure", "health_decide")


def run(root):
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import gstreamer_vit_tracker_amd as vt
    B, W, H = 30, 1920, 1080
    scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    keep = [[torch.from_numpy(sc.frame_nv12(k)).cuda() for sc in scs] for k in (0, 1)]
    frames = [[vt.frame_nv12(t.data_ptr(), t.data_ptr() + W * H, W, H) for t in row] for row in keep]
    st = np.zeros(B, vt.snapshot.STATE)
    st["frame_w"], st["frame_h"], st["initialized"] = W, H, 1
    carry = {}
    seen = []

    def call(k, **pol):
        nonlocal carry
        got = vt.op_frame_health(frames[k & 1], st, **pol, **carry)
        carry = {n: got[n] for n in ("thumbs", "hist", "records", "counts")}
        seen.append(sorted(set(got["heads"]["status"].tolist())))
        return got

    for k in range(2):
        call(k)
    for k in range(REPS):
        got = call(k)
    r = got["records"][0]
    print(f"due: stream 0 status {r['status']} c {r['c']} grid {r['Wg']} x {r['Hg']} D {r['D']} HD {r['HD']} flags {r['flags']}", flush=True)
    st["frames_done"] = 1
    for k in range(REPS):
        call(k, period=30)
    for k in range(REPS):
        call(k, on=0)
    print("header statuses per call:", seen[0], seen[1], seen[2], seen[2 + REPS], seen[2 + 2 * REPS], flush=True)


def report(out_dir):
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, f"no kernel trace under {out_dir}"
    per = {k: [] for k in KERNELS}
    for row in csv.DictReader(open(paths[0])):
        for k in KERNELS:
            if k in row["Kernel_Name"]:
                per[k].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for k in KERNELS:
        per[k].sort()
        assert len(per[k]) == 2 + 3 * REPS, (k, len(per[k]))
    import numpy as np
    for c, case in enumerate(CASES):
        lo = 2 + c * REPS
        parts, total = [], np.zeros(REPS)
        for k in KERNELS:
            us = np.array([(e - s) / 1e3 for s, e in per[k][lo:lo + REPS]])
            total += us
            parts.append(f"{k[7:]} {np.median(us):7.2f} [min {us.min():7.2f}]")
        span = np.array([(per[KERNELS[-1]][lo + i][1] - per[KERNELS[0]][lo + i][0]) / 1e3 for i in range(REPS)])
        print(f"{case:7s} {'  '.join(parts)}  sum {np.median(total):7.2f} us  first begin -> last end {np.median(span):7.2f} us")


if __name__ == "__main__":
    if sys.argv[2] == "run":
        run(os.path.abspath(sys.argv[1]))
    else:
        report(sys.argv[3])
