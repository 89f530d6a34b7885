"""Pipelined subset passes (vt_group_enqueue_host_streams + vt_group_wait_next, two deep) against the synchronous
subset pass (vt_group_update_host_streams), and the cost of a stream joining (run on the GPU box):

    python tools/pipelined_subset_bench.py [--cfg cfg3] [--group 30] [--n 1,4,8,15,24,29,30] [--steps 60] [--reps 5]
                                           [--joins 6] [--out F.json] [--table F.txt]

One engine of `--group` streams, 1920x1080 NV12 HOST frames, 64-px moving targets (bench.py's clip, two frames per
stream in turn), every stream its own frames. For every n, ms per pass in steady state of
  (a) update_host over a list of n streams                       - the yardstick: upload, pass and wait inside the period
  (b) enqueue_host over the same list + wait_next, two in flight - the upload of pass t+1 beside pass t
timed by the host clock around `--steps` passes that end in a synchronise (update_host returns after one; the
last wait_next is one), after a warm-up of the same list; (a) and (b) alternate inside one process and the median of
`--reps` is reported with the spread (max - min) of each. n = group is the identity list: the full pass, graph replay.

The join: a group tracking group-1 streams pipelined, one more stream is initialised and tracked from the next frame
on. The duration of the frame period that contains the join - from "frame t is there" to "results of t-1 delivered,
pass t in flight" - for
  (c) drain (wait_next), init_host, enqueue_host       - the only way while every init is refused behind a pass
  (d) enqueue_init_host, enqueue_host, wait_next       - the init queued behind the outstanding pass
and, beside them, the same period without a join. `--joins` of each, alternating, medians and spread."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # repo root

import numpy as np


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cfg", default="cfg3")
    ap.add_argument("--group", type=int, default=30)
    ap.add_argument("--n", default="1,4,8,15,24,29,30")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--joins", type=int, default=6)
    ap.add_argument("--out", default="")
    ap.add_argument("--table", default="")
    a = ap.parse_args()
    import gstreamer_vit_tracker_amd as vt
    G = a.group
    ns = [int(v) for v in a.n.split(",")]
    assert all(1 <= n <= G for n in ns) and G >= 2
    weights = vt.weights.ensure_weights(a.cfg)
    w, h = 1920, 1080
    scs = [vt.synth.MovingSquare(w, h, 64, seed=100 + i) for i in range(G)]
    clip = [[vt.NV12Frame(sc.frame_nv12(t), w, h) for t in range(2)] for sc in scs]     # [stream][t & 1]
    boxes = [vt.BBox.new(*sc.gt_box(0)) for sc in scs]
    grp = vt.Group(weights, n_streams=G)
    for s in range(G):
        grp.init_host(s, clip[s][0], boxes[s])
    caps = grp.graph_captures()
    tick = [0]

    def frames(L):
        tick[0] += 1
        return [clip[s][tick[0] & 1] for s in L]

    def sync_ms(L):
        for _ in range(a.warmup):
            grp.update_host(frames(L), streams=L)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            grp.update_host(frames(L), streams=L)
        return (time.perf_counter() - t0) * 1e3 / a.steps

    def pipe_ms(L):
        grp.enqueue_host(frames(L), streams=L)
        for _ in range(a.warmup):
            grp.enqueue_host(frames(L), streams=L)
            grp.wait_next()
        t0 = time.perf_counter()                  # one pass in flight; every turn of the loop completes one
        for _ in range(a.steps):
            grp.enqueue_host(frames(L), streams=L)
            grp.wait_next()
        dt = (time.perf_counter() - t0) * 1e3 / a.steps
        grp.wait_next()
        return dt

    lines = [f"# {a.cfg}, one engine of {G}, {w}x{h} NV12 host frames; ms per pass, median of {a.reps} x {a.steps} passes "
             f"(spread = max - min of the {a.reps})", f"# build: {vt.build_info()}",
             "#   n   (a) update_host_streams   (b) enqueue_host_streams + wait_next   (b) - (a)    (b) / (a)"]
    rng = np.random.default_rng(0)
    rows = []
    for n in ns:
        L = list(range(G)) if n == G else sorted(int(s) for s in rng.choice(G, n, replace=False))
        if n < G:
            L = [int(s) for s in rng.permutation(L)]
        m = {"sync": [], "pipe": []}
        for _ in range(a.reps):
            m["sync"].append(sync_ms(L))
            m["pipe"].append(pipe_ms(L))
        row = {"n": n, "streams_sample": L[:8]}
        for k, v in m.items():
            row[k + "_ms"] = float(np.median(v))
            row[k + "_spread_ms"] = float(max(v) - min(v))
            row[k + "_ms_all"] = [round(x, 4) for x in v]
        rows.append(row)
        lines.append(f"  {n:3d}   {row['sync_ms']:8.3f} (spread {row['sync_spread_ms']:.3f})      {row['pipe_ms']:8.3f} (spread "
                     f"{row['pipe_spread_ms']:.3f})               {row['pipe_ms'] - row['sync_ms']:+7.3f}      "
                     f"{row['pipe_ms'] / row['sync_ms']:.3f}")
        print(lines[-1], flush=True)
    redos_passes = grp.host_redos()

    # ---- the join: stream G-1 joins a group that tracks the other G-1 ----
    most, every, j = list(range(G - 1)), list(range(G)), G - 1
    period = {"plain_most": [], "plain_every": [], "drain_init": [], "queued_init": []}

    def plain(L, into, turns):
        for _ in range(turns):
            t0 = time.perf_counter()
            grp.enqueue_host(frames(L), streams=L)
            grp.wait_next()
            into.append((time.perf_counter() - t0) * 1e3)

    grp.enqueue_host(frames(most), streams=most)
    plain(most, [], a.warmup)
    for k in range(2 * a.joins):
        plain(most, period["plain_most"], 6)
        f = clip[j][tick[0] & 1]
        t0 = time.perf_counter()
        if k % 2 == 0:                            # (c) drain, synchronous init, restart
            grp.wait_next()
            grp.init_host(j, f, boxes[j])
            grp.enqueue_host(frames(every), streams=every)
            period["drain_init"].append((time.perf_counter() - t0) * 1e3)
        else:                                     # (d) the init queued behind the outstanding pass
            grp.enqueue_init_host(j, f, boxes[j])
            grp.enqueue_host(frames(every), streams=every)
            grp.wait_next()
            period["queued_init"].append((time.perf_counter() - t0) * 1e3)
        plain(every, period["plain_every"], 6)    # stream j tracks ... and leaves again
    grp.wait_next()
    assert grp.graph_captures() == caps, "a capture happened inside a pass"
    join = {k: {"median_ms": float(np.median(v)), "spread_ms": float(max(v) - min(v)), "count": len(v)}
            for k, v in period.items()}
    lines += ["#", f"# the frame period that contains a join (stream {j} joins the other {G - 1}); ms, median (spread), count",
              f"  no join, {G - 1} streams                      {join['plain_most']['median_ms']:8.3f} ({join['plain_most']['spread_ms']:.3f}) {join['plain_most']['count']}",
              f"  no join, {G} streams                      {join['plain_every']['median_ms']:8.3f} ({join['plain_every']['spread_ms']:.3f}) {join['plain_every']['count']}",
              f"  (c) wait_next + init_host + enqueue_host   {join['drain_init']['median_ms']:8.3f} ({join['drain_init']['spread_ms']:.3f}) {join['drain_init']['count']}",
              f"  (d) enqueue_init_host + enqueue + wait_next {join['queued_init']['median_ms']:7.3f} ({join['queued_init']['spread_ms']:.3f}) {join['queued_init']['count']}",
              f"# host_redos: {redos_passes} during the passes, {grp.host_redos()} at the end"]
    print("\n".join(lines[-6:]), flush=True)
    res = {"cfg": a.cfg, "group": G, "frame": [w, h], "target_px": 64, "steps": a.steps, "warmup": a.warmup,
           "reps": a.reps, "build": vt.build_info(), "rows": rows, "join": join, "host_redos": grp.host_redos()}
    for path, text in ((a.out, json.dumps(res, indent=1)), (a.table, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    grp.close()


if __name__ == "__main__":
    main()
