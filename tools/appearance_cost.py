"""Appearance check: what a never-enabled engine pays (nothing), and what the two launches of an enabled one take per pass
at period 1, at period 30 and with every stream due. cfg3 x 30 streams, device-resident 1080p NV12.
usage: python tools/appearance_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE:
  never          no appearance key ever set: ms per device pass (vt_group_enqueue_device + vt_group_wait), three runs of 40,
                 and the sum of the kernel times of vt_group_profile_device
  p1             "appearance" 1, period 1: every stream is due in every pass (the streams' frames_done run in step)
  p30            period 30: the streams are due in every 30th pass only - the launches' times over passes that are not due
                 and over the due ones, apart
  off            enabled once, then "appearance" 0: two launches that leave at once
  refresh        period 1 beside a template refresh of period 2 with the gate at 500 per mille: the refresh launch next to it
For each enabled case: the appearance_probe / appearance_score / refresh_template launches' own begin -> end times, medians
over the profiled passes [and the minimum]."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt

B, W, H = 30, 1920, 1080
w = vt.weights.ensure_weights("cfg3")
NAMES = ("appearance_probe", "appearance_score", "refresh_template")


def engine(square=64):
    scs = [vt.synth.MovingSquare(W, H, square, seed=s) for s in range(B)]
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


def launch_us(g, dev, passes):
    """per profiled pass: (sum of all kernels, the three launches, was stream 0 evaluated in it)"""
    rows = []
    for _ in range(passes):
        before = g.appearance(0)["evaluated"] if g_enabled else 0
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        due = (g.appearance(0)["evaluated"] - before) if g_enabled else 0
        rows.append([sum(d.values())] + [d.get(n, 0.0) for n in NAMES] + [due])
    return np.array(rows)


def fmt(a):
    return "  ".join(f"{n} {np.median(a[:, 1 + i]):6.2f} us [min {a[:, 1 + i].min():6.2f}]" for i, n in enumerate(NAMES) if a[:, 1 + i].any())


for case in sys.argv[2:] or ["never"]:
    g, dev, keep = engine()
    g_enabled = case != "never"
    if case == "p1":
        g.set_appearance(True, period=1)
    elif case == "p30":
        g.set_appearance(True, period=30)
    elif case == "off":
        g.set_appearance(True)
        g.set_appearance(False)
    elif case == "refresh":
        g.set_template_refresh(2, 0.0)
        g.set_appearance(True, period=1, gate=0.5)
    ms = pass_ms(g, dev)
    a = launch_us(g, dev, 60 if case == "p30" else 20)
    line = f"{case:8s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {np.median(a[:, 0]):8.1f} us"
    print(line, flush=True)
    if case == "p30":
        due, idle = a[a[:, 4] > 0], a[a[:, 4] == 0]
        print(f"         {len(idle)} passes not due: {fmt(idle)}", flush=True)
        print(f"         {len(due)} passes due:     {fmt(due)}", flush=True)
    elif g_enabled:
        ap = g.appearance(0)
        print(f"         {fmt(a)}   (stream 0: evaluated {ap['evaluated']}, gated {ap['gated']}, similarity {ap['similarity']:.4f})", flush=True)
    g.close()
