"""Same-process A/B of the "last_rows" tuning key: E engines of B streams run PASSES device-frame
passes each, from one thread per engine, in alternating blocks - the last block on search rows only (default) / on all
rows ("last_rows" = 0) - and the wall time per block is printed. One binary, one process, one set of buffers: what
differs between the blocks is the tuning key alone.

   python tools/last_rows_ab.py [--engines 2] [--streams 30] [--passes 300] [--blocks 6] [--workload cfg3]   (on the GPU box)"""
import argparse
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engines", type=int, default=2)
    ap.add_argument("--streams", type=int, default=30)
    ap.add_argument("--passes", type=int, default=300)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--workload", default="cfg3")
    a = ap.parse_args()
    import torch
    import gstreamer_vit_tracker_amd as vt
    w, h = 1920, 1080
    weights = vt.weights.ensure_weights(a.workload)
    sc = vt.synth.MovingSquare(w, h, 64, seed=1)
    bufs = [torch.from_numpy(sc.frame_nv12(t)).cuda() for t in range(8)]
    frames = [vt.frame_nv12(b.data_ptr(), b.data_ptr() + w * h, w, h) for b in bufs]
    groups = [vt.Group(weights, n_streams=a.streams) for _ in range(a.engines)]
    for g in groups:
        for i in range(a.streams):
            g.init_device(i, frames[0], vt.BBox.new(*sc.gt_box(0)))

    def run(g, n):
        for t in range(n):
            g.update_device([frames[t % 8]] * a.streams)

    def block(n):
        th = [threading.Thread(target=run, args=(g, n)) for g in groups]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join()
        return (time.perf_counter() - t0) / n * 1e3

    out = {1: [], 0: []}
    for b in range(a.blocks):
        for mode in ((1, 0) if b % 2 == 0 else (0, 1)):
            for g in groups:
                g.set_tuning("last_rows", mode)
            block(30)       # warm-up of the recaptured passes
            ms = block(a.passes)
            rows = int(groups[0].read_tensor("last_block_rows")[0])
            out[mode].append(ms)
            print(f"block {b} last_rows={mode} (last block on {rows} rows per stream): {ms:.4f} ms per step of {a.engines} x {a.streams} streams", flush=True)
    m1, m0 = float(np.median(out[1])), float(np.median(out[0]))
    print(f"median ms per step: search rows {m1:.4f} (min {min(out[1]):.4f} max {max(out[1]):.4f}), all rows {m0:.4f} "
          f"(min {min(out[0]):.4f} max {max(out[0]):.4f}); all rows / search rows = {m0 / m1:.4f}")


if __name__ == "__main__":
    main()
