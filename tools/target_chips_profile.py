"""Target chips: what an enabled engine pays per pass. cfg3 x 30 streams, 1080p NV12 device frames, 64-px targets, per-pass
times of vt_group_profile_device (medians over 20 passes): sum of kernels, target_chips, refresh_template.
usage: python tools/target_chips_profile.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("." or a parent-commit tree built beside it). CASE: "never" (no feature
enabled: the only case a parent tree can run), "refresh" (template refresh, period 2: the passes in which all 30 streams
fire), or SIZE:KIND:PERIOD[:FACTOR] such as 192:bf16:1, 192:bf16:30, 224:u8:1. Every case runs on an engine of its own.
VITTRACK_HIP_LIB selects a tuning build of the library (python build.py --variant NAME -DMACRO)."""
import os
import sys

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt

B, W, H = 30, 1920, 1080
w = vt.weights.ensure_weights("cfg3")
scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]


def frames(t):
    keep = [torch.from_numpy(sc.frame_nv12(t)).cuda() for sc in scs]
    return [vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H) for d in keep], keep


f0, k0 = frames(0)
f1, k1 = frames(1)


def engine():
    g = vt.Group(w, n_streams=B)
    for s in range(B):
        g.init_device(s, f0[s], vt.BBox.new(*scs[s].gt_box(0)))
    return g


def one(g):
    d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(f1, iters=1)}
    return sum(d.values()), d.get("target_chips", 0.0), d.get("refresh_template", 0.0), d.get("preproc_search", 0.0)


def stats(rows, tag):
    a = np.array(rows)
    print(f"{tag:36s} n={len(rows):2d}  pass(sum of kernels) {np.median(a[:, 0]):8.1f} us  target_chips {np.median(a[:, 1]):6.2f} us "
          f"[min {a[:, 1].min():6.2f}]  refresh {np.median(a[:, 2]):6.2f} us  preproc_search {np.median(a[:, 3]):6.2f} us", flush=True)


for case in sys.argv[2:] or ["never"]:
    g = engine()
    for _ in range(6):
        g.update_device(f1)         # warm
    if case == "never":
        stats([one(g) for _ in range(20)], "never enabled")
    elif case == "refresh":
        g.set_template_refresh(2, 0.0)
        fire = []
        for _ in range(44):
            g0 = [g.template_refresh_stats(s)["generation"] for s in range(B)]
            r = one(g)
            if sum(g.template_refresh_stats(s)["generation"] - g0[s] for s in range(B)) == B:
                fire.append(r)
        stats(fire, "refresh, period 2, all 30 fire")
    else:
        p = case.split(":")
        size, kind, period = int(p[0]), {"bf16": vt.CHIP_NORM_BF16, "u8": vt.CHIP_RGB8}[p[1]], int(p[2])
        factor = float(p[3]) if len(p) > 3 else 2.0
        g.enable_chips(size, kind, (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044))
        g.set_chips(factor, period, 0)
        cut, idle = [], []
        for _ in range(20 if period == 1 else 2 * period + 2):
            r = one(g)
            n = sum(i["status"] == 1 for i in g.read_chips()[1])
            (cut if n == B else idle if n == 0 else []).append(r)
        if cut:
            stats(cut, f"chips {case}, all 30 cut")
        if idle:
            stats(idle, f"chips {case}, pass w/o a chip")
    g.close()
