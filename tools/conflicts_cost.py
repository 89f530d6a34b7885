"""Stream conflicts: what a never-enabled engine pays (nothing), and what the one launch of an enabled one takes per pass.
usage: python tools/conflicts_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE:
  never       cfg3 x 30 streams, device-resident 1080p NV12, no conflicts key ever set: ms per device pass
              (vt_group_enqueue_device + vt_group_wait), three runs of 40, and the sum of the kernel times of
              vt_group_profile_device
  scene1      the same engine, "conflicts" 1, every stream in scene 1: every stream is compared with the 29 others
  scene0      every stream in scene 0: 30 records with status 3, nobody compared
  off         enabled once, then "conflicts" 0: a launch that leaves at once
  tiny1       a 1024-stream tiny engine on one shared 640 x 480 frame, all streams started on the same box and in scene 1:
              every lane walks 1,024 entries, every pair overlaps - the one case where the walk is work and not latency
  tiny0       the same engine, every stream in scene 0
For each enabled case: the conflicts_check launch's own begin -> end time, median over the profiled passes [and the minimum]."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt


def engine(cfg, B, W, H, shared):
    w = vt.weights.ensure_weights(cfg)
    scs = [vt.synth.MovingSquare(W, H, 64, seed=0 if shared else s) for s in range(1 if shared else B)]
    g = vt.Group(w, n_streams=B)
    first = [torch.from_numpy(sc.frame_nv12(0)).cuda() for sc in scs]
    for s in range(B):
        d, sc = first[0 if shared else s], scs[0 if shared else s]
        g.init_device(s, vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H), vt.BBox.new(*sc.gt_box(0)))
    keep = [torch.from_numpy(sc.frame_nv12(1)).cuda() for sc in scs]
    dev = [vt.frame_nv12(keep[0 if shared else s].data_ptr(), keep[0 if shared else s].data_ptr() + W * H, W, H) for s in range(B)]
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


def launch_us(g, dev, passes):
    """per profiled pass: (sum of all kernels, the conflicts launch)"""
    rows = []
    for _ in range(passes):
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        rows.append([sum(d.values()), d.get("conflicts_check", 0.0)])
    return np.array(rows)


for case in sys.argv[2:] or ["never"]:
    tiny = case.startswith("tiny")
    g, dev, keep = engine("tiny", 1024, 640, 480, True) if tiny else engine("cfg3", 30, 1920, 1080, False)
    if case != "never":
        g.set_conflicts(True)
        g.set_scene(None, 1 if case in ("scene1", "tiny1", "off") else 0)
        if case == "off":
            g.set_conflicts(False)
    ms = pass_ms(g, dev, n=10 if tiny else 40)
    a = launch_us(g, dev, 20)
    print(f"{case:8s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {np.median(a[:, 0]):8.1f} us", flush=True)
    if case != "never":
        c = g.conflicts(0)
        print(f"         conflicts_check {np.median(a[:, 1]):6.2f} us [min {a[:, 1].min():6.2f}]   (stream 0: status {c['status']}, "
              f"n_over {c['n_over']}, evaluated {c['evaluated']})", flush=True)
    g.close()
