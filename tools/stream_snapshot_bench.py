"""What moving a stream costs (run on the GPU box):

    python tools/stream_snapshot_bench.py [--cfg cfg3] [--group 30] [--calls 30] [--periods 40] [--out F.json]

Two engines of --group streams on one GPU, 1920x1080 NV12, 64-px targets. Host wall clock around the synchronous calls,
median of --calls after a warm-up, every figure with its minimum and maximum:

  export_ms / import_ms / copy_ms   vt_group_export_stream(A, 7) into a caller buffer, vt_group_import_stream(B, 0) of
                                    those bytes, vt_group_copy_stream(A, 7, B, 0) - nothing else on the device
  period_ms                         one period of the pipelined host loop of B over its streams 1 .. group - 1
                                    (vt_group_wait_next of the oldest pass + vt_group_enqueue_host_streams of the next,
                                    two passes in flight), without and WITH a vt_group_import_stream into stream 0
                                    queued in every period beside the two outstanding passes; the two variants alternate
                                    in blocks of ten periods so that both see the same machine"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np


def _stats(v):
    v = np.asarray(v, np.float64) * 1e3
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4), n=len(v))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--cfg", default="cfg3")
    ap.add_argument("--group", type=int, default=30)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--periods", type=int, default=40)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo))
    import torch
    import gstreamer_vit_tracker_amd as vt
    G, w, h = a.group, 1920, 1080
    weights = vt.weights.ensure_weights(a.cfg)
    scs = [vt.synth.MovingSquare(w, h, 64, seed=100 + i) for i in range(3)]
    ring = 4
    host = [[vt.NV12Frame(np.ascontiguousarray(sc.frame_nv12(t)), w, h) for t in range(ring)] for sc in scs]
    A, B = vt.Group(weights, n_streams=G), vt.Group(weights, n_streams=G)
    for g in (A, B):
        for s in range(G):
            sc = scs[s % 3]
            f0 = torch.from_numpy(host[s % 3][0].buf).cuda()
            g.init_device(s, vt.frame_nv12(f0.data_ptr(), f0.data_ptr() + w * h, w, h), vt.BBox.new(*sc.gt_box(0)))
    for g in (A, B):
        for t in (1, 2, 3):
            g.update_host([host[s % 3][t % ring] for s in range(G)])
    caps = (A.graph_captures(), B.graph_captures())
    L = vt.lib()
    need = A.snapshot_bytes()
    buf, n = ctypes.create_string_buffer(need), ctypes.c_size_t(0)

    def timed(fn, calls):
        for _ in range(5):
            fn()
        out = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t0)
        return out

    def export():
        vt._check(L.vt_group_export_stream(A._h, 7, buf, need, ctypes.byref(n)))

    def imp():
        vt._check(L.vt_group_import_stream(B._h, 0, buf, need))

    def copy():
        vt._check(L.vt_group_copy_stream(A._h, 7, B._h, 0))

    res = {"cfg": a.cfg, "group": G, "frame": [w, h], "snapshot_bytes": need, "build": vt.build_info(),
           "export": _stats(timed(export, a.calls)), "import": _stats(timed(imp, a.calls)), "copy": _stats(timed(copy, a.calls))}
    for k in ("export", "import", "copy"):
        print(f"{k:7s} {res[k]}", flush=True)

    # a period of the pipelined loop over streams 1 .. G-1, with and without an import queued into stream 0
    lst = list(range(1, G))

    def frames(t):
        return [host[s % 3][t % ring] for s in lst]

    t = 4
    B.enqueue_host(frames(t), streams=lst); t += 1
    B.enqueue_host(frames(t), streams=lst); t += 1
    per = {False: [], True: []}
    for p in range(2 * a.periods + 20):
        with_import = (p // 10) % 2 == 1
        t0 = time.perf_counter()
        if with_import:
            imp()
        B.wait_next()
        B.enqueue_host(frames(t), streams=lst)
        dt = time.perf_counter() - t0
        t += 1
        if p >= 20:
            per[with_import].append(dt)
    B.wait_next(), B.wait_next()
    res["period_plain"], res["period_with_import"] = _stats(per[False]), _stats(per[True])
    res["host_redos"] = B.host_redos()
    print(f"period without import {res['period_plain']}\nperiod with import    {res['period_with_import']}  (redos {res['host_redos']})", flush=True)
    assert (A.graph_captures(), B.graph_captures()) == caps, "a snapshot call captured a graph"
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    A.close(), B.close()


if __name__ == "__main__":
    main()
