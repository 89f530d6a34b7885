"""Result overlay: what a never-enabled engine pays (nothing), what an enabled one pays per pass, and what the route it
replaces costs. cfg3 x 30 streams, device-resident 1080p NV12 frames.
usage: python tools/result_overlay_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE:
  never        no overlay key ever set: ms per device pass (vt_group_enqueue_device + vt_group_wait), three runs of 40
  F:S[:one]    flags F (1, 3, 7) on 30 streams with S-px targets, gate score > 0 (":one": the other 29 targets are absent from
               their frames and the gate is the default 25, so that stream 7 alone draws; the line says how many streams
               the last pass drew): ms per device pass as above, and from vt_group_profile_device
               (one pass at a time, medians over 20) the result_overlay launch's own begin -> end time
  today:S      the route the feature replaces, on the same engine without the overlay: after vt_group_wait, per camera one
               vt_overlay_nv12_device call with the equivalent list (rectangle, crosshair, label; gate score > 0) - wall time from the
               first call to the device being idle again, and the device's own time between two events around the 30 calls
The frames stay on the device and are drawn into pass after pass (the shapes land where they were: the targets do not move
between the passes of one case)."""
import ctypes
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt
import result_overlay_util as ro

B, W, H = 30, 1920, 1080
w = vt.weights.ensure_weights("cfg3")


def engine(square, one=False):
    scs = [vt.synth.MovingSquare(W, H, square, seed=s, hide=(1, 1 << 30) if one and s != 7 else None) for s in range(B)]
    g = vt.Group(w, n_streams=B)
    for s, sc in enumerate(scs):
        d = torch.from_numpy(sc.frame_nv12(0)).cuda()
        g.init_device(s, vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H), vt.BBox.new(*sc.gt_box(0)))
    keep = [torch.from_numpy(sc.frame_nv12(1)).cuda() for sc in scs]
    dev = [vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H) for d in keep]
    return g, dev, keep


def pass_ms(g, dev, runs=3, n=40):
    out = []
    for _ in range(runs):
        for _ in range(5):
            g.enqueue_device(dev)
            g.wait()
        t0 = time.perf_counter()
        for _ in range(n):
            g.enqueue_device(dev)
            g.wait()
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def launch_us(g, dev):
    rows = []
    for _ in range(20):
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        rows.append((sum(d.values()), d.get("result_overlay", 0.0)))
    a = np.array(rows)
    return np.median(a, axis=0), a[:, 1].min()


def today(g, dev, keep, n=40):
    """wait, then one vt_overlay_nv12_device per camera with the list the overlay would draw"""
    L = vt.lib()
    wall, devt = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(n + 5):
        g.enqueue_device(dev)
        res = g.wait()
        t0 = time.perf_counter()
        e0.record()
        for s, r in enumerate(res):
            if not ro.draws(r.success, r.score, 0):
                continue
            cmds = ro.commands(r.bbox, r.score, "luma")
            arr = (vt.CDrawCmd * len(cmds))()
            for c, (kind, x, y, cw, ch, p, value, text) in zip(arr, cmds):
                c.type, c.x, c.y, c.w, c.h, c.p, c.value, c.text = kind, x, y, cw, ch, p, value, text.encode()
            rc = L.vt_overlay_nv12_device(0, ctypes.c_void_p(keep[s].data_ptr()), W, H, W, arr, len(cmds), None)
            assert rc == 0
        e1.record()
        torch.cuda.synchronize()
        if it >= 5:
            wall.append((time.perf_counter() - t0) * 1e6)
            devt.append(e0.elapsed_time(e1) * 1e3)
    return np.median(wall), np.min(wall), np.median(devt), np.min(devt)


for case in sys.argv[2:] or ["never"]:
    p = case.split(":")
    if case == "never":
        g, dev, keep = engine(64)
        ms = pass_ms(g, dev)
        med, _ = launch_us(g, dev)
        print(f"{'never enabled':24s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {med[0]:8.1f} us", flush=True)
    elif p[0] == "today":
        g, dev, keep = engine(int(p[1]))
        wm, wn, dm, dn = today(g, dev, keep)
        print(f"{'today, ' + p[1] + '-px boxes':24s} 30 x vt_overlay_nv12_device after wait: wall {wm:7.1f} us [min {wn:7.1f}]  "
              f"device {dm:7.1f} us [min {dn:7.1f}]", flush=True)
    else:
        flags, square, one = int(p[0]), int(p[1]), len(p) > 2 and p[2] == "one"
        g, dev, keep = engine(square, one)
        g.set_result_overlay(rect=bool(flags & 1), crosshair=bool(flags & 2), score=bool(flags & 4), min_score_pct=25 if one else 0)
        ms = pass_ms(g, dev)
        med, mn = launch_us(g, dev)
        drawn = sum(g.result_overlay_stats(s)["drawn"] for s in range(B))
        tag = f"flags {flags}, {square}-px, {'stream 7 only' if one else 'all 30'}"
        print(f"{tag:32s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {med[0]:8.1f} us  "
              f"result_overlay {med[1]:5.2f} us [min {mn:5.2f}]  streams drawn in the last pass {drawn}", flush=True)
    g.close()
