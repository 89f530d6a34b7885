"""Pass time of a subset pass (vt_group_update_device_streams) against engines of the pass's size (run on the GPU box):

    python tools/stream_subset_bench.py [--cfg cfg3] [--group 30] [--n 1,4,10,20,29,30] [--steps 40] [--reps 3] [--out F.json]

For every n: ms per pass of a `--group`-stream engine whose passes list n of its streams (eager launches: the full
identity list at n = group replays the captured graph), and of an engine of exactly n streams, eager (use_graph=0)
and graphed. Device NV12 frames, 1920x1080, 64-px targets (bench.py's clip); every stream has its own frame. A
measurement is `--steps` back-to-back passes (enqueue, then one wait at the end) timed by the wall clock after a
warm-up; the three kinds are interleaved per repetition and the median of `--reps` is reported, with the spread.
A subset pass does the n-stream engine's eager work plus one template-row gather, so it should land within a few
per cent of the eager n-stream engine; the graphed column shows what launch cost the eager path pays at small n."""
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
    ap.add_argument("--n", default="1,4,10,20,29,30")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    import gstreamer_vit_tracker_amd as vt
    ns = [int(v) for v in a.n.split(",")]
    assert all(1 <= n <= a.group for n in ns)
    weights = vt.weights.ensure_weights(a.cfg)
    w, h = 1920, 1080
    scs = [vt.synth.MovingSquare(w, h, 64, seed=100 + i) for i in range(a.group)]
    bufs = [torch.from_numpy(sc.frame_nv12(0)).cuda() for sc in scs]
    frames = [vt.frame_nv12(b.data_ptr(), b.data_ptr() + w * h, w, h) for b in bufs]
    boxes = [vt.BBox.new(*sc.gt_box(0)) for sc in scs]

    def make(n, use_graph):
        g = vt.Group(weights, n_streams=n, use_graph=use_graph)
        for i in range(n):
            g.init_device(i, frames[i], boxes[i])
        return g

    def timed(g, fr, streams):
        for _ in range(a.warmup):
            g.enqueue_device(fr, streams)
        g.wait()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            g.enqueue_device(fr, streams)
        g.wait()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    big = make(a.group, True)
    caps = big.graph_captures()
    rng = np.random.default_rng(0)
    rows = []
    for n in ns:
        # the listed streams: a random choice in random order (n = group: the identity, i.e. the full pass)
        streams = list(range(a.group)) if n == a.group else [int(s) for s in rng.choice(a.group, n, replace=False)]
        eager, graphed = make(n, False), make(n, True)
        m = {"subset": [], "eager": [], "graph": []}
        for _ in range(a.reps):
            m["subset"].append(timed(big, [frames[s] for s in streams], streams))
            m["eager"].append(timed(eager, frames[:n], None))
            m["graph"].append(timed(graphed, frames[:n], None))
        eager.close()
        graphed.close()
        row = {"n": n, "streams_sample": streams[:8]}
        for k, v in m.items():
            row[k + "_ms"] = float(np.median(v))
            row[k + "_ms_all"] = [round(x, 4) for x in v]
        row["subset_vs_eager"] = row["subset_ms"] / row["eager_ms"]
        row["eager_vs_graph"] = row["eager_ms"] / row["graph_ms"]
        rows.append(row)
        print(f"n {n:3d}: subset of {a.group} {row['subset_ms']:7.3f} ms  (eager {n}-stream engine {row['eager_ms']:7.3f} ms, "
              f"ratio {row['subset_vs_eager']:.3f};  graphed {row['graph_ms']:7.3f} ms, eager / graph "
              f"{row['eager_vs_graph']:.3f})  spreads {m['subset']!r} {m['eager']!r} {m['graph']!r}", flush=True)
    assert big.graph_captures() == caps, "a capture happened inside an update"
    res = {"cfg": a.cfg, "group": a.group, "frame": [w, h], "target_px": 64, "steps": a.steps, "warmup": a.warmup,
           "reps": a.reps, "build": vt.build_info(), "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    big.close()


if __name__ == "__main__":
    main()
