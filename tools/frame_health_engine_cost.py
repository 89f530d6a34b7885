"""Frame health: what a never-enabled engine pays (nothing), and what the four launches of an enabled one take per pass.
usage: python tools/frame_health_engine_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE, all on cfg3 x 30 streams, device-resident 1080p NV12:
  never     no health key ever set: ms per device pass (vt_group_enqueue_device + vt_group_wait), three runs of 40, and the
            sum of the kernel times of vt_group_profile_device
  due       "health" 1, every stream due in every pass
  period    "health_period" 30
  off       enabled once, then "health" 0: four launches that leave at once
For each enabled case: the four launches' own begin -> end times, medians over the profiled passes, and their sum."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt

NAMES = ("health_prepare", "health_thumb", "health_measure", "health_decide")


def engine(B=30, W=1920, H=1080):
    w = vt.weights.ensure_weights("cfg3")
    scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    g = vt.Group(w, n_streams=B)
    first = [torch.from_numpy(sc.frame_nv12(0)).cuda() for sc in scs]
    for s in range(B):
        g.init_device(s, vt.frame_nv12(first[s].data_ptr(), first[s].data_ptr() + W * H, W, H), vt.BBox.new(*scs[s].gt_box(0)))
    keep = [torch.from_numpy(sc.frame_nv12(1)).cuda() for sc in scs]
    return g, [vt.frame_nv12(k.data_ptr(), k.data_ptr() + W * H, W, H) for k in keep], keep


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
    rows = []
    for _ in range(passes):
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        rows.append([sum(d.values())] + [d.get(k, 0.0) for k in NAMES])
    return np.array(rows)


for case in sys.argv[2:] or ["never"]:
    g, dev, keep = engine()
    if case != "never":
        g.set_health(True, period=30 if case == "period" else 1)
        if case == "off":
            g.set_health(False)
    ms = pass_ms(g, dev)
    a = launch_us(g, dev, 20)
    print(f"{case:7s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {np.median(a[:, 0]):8.1f} us", flush=True)
    if case != "never":
        m = np.median(a[:, 1:], axis=0)
        h = g.frame_health(0)
        print("        " + "  ".join(f"{k[7:]} {v:6.2f}" for k, v in zip(NAMES, m)) + f"  sum {m.sum():6.2f} us   (stream 0: status "
              f"{h['status']}, c {h['c']}, {h['Wg']} x {h['Hg']}, flags {h['flags']}, evaluated {h['evaluated']})", flush=True)
    g.close()
