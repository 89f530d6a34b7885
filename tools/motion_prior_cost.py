"""Motion prior: what a never-enabled engine pays (nothing), what the two launches of an enabled one take per pass, and what
the prior does to the redo count of pipelined host passes. cfg3 x 30 streams, 1080p NV12.
usage: python tools/motion_prior_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE:
  never          no motion key ever set: ms per device pass (vt_group_enqueue_device + vt_group_wait) on device-resident
                 frames, three runs of 40, and the sum of the kernel times of vt_group_profile_device
  on             "motion_prior" 1 with the default policy: the same, and the motion_place / motion_settle launches' own
                 begin -> end times (medians over 20 profiled passes [and the minimum])
  redos:K:M:on|off[:PERIOD:AMP]
                 300 pipelined host passes (vt_group_enqueue_host two deep / vt_group_wait_next), all 30 streams on the
                 clip MovingSquare(seed 0, 64-px target[, period PERIOD, amplitude AMP px]) sampled every K-th frame,
                 vt_config.host_window_margin_pct = M, with / without the prior: vt_group_host_redos, successes, ms per pass"""
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


def launch_us(g, dev):
    rows = []
    for _ in range(20):
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        rows.append((sum(d.values()), d.get("motion_place", 0.0), d.get("motion_settle", 0.0)))
    a = np.array(rows)
    return np.median(a, axis=0), a.min(axis=0)


def redos(step, margin, on, passes=300, **path):
    sc = vt.synth.MovingSquare(W, H, 64, seed=0, **path)
    g = vt.Group(w, n_streams=B, host_window_margin_pct=margin)
    f0 = vt.NV12Frame(sc.frame_nv12(0), W, H)
    for s in range(B):
        g.init_host(s, f0, vt.BBox.new(*sc.gt_box(0)))
    if on:
        g.set_motion_prior(True)
    ok = 0
    t0 = time.perf_counter()
    for k in range(1, passes + 1):
        fr = vt.NV12Frame(sc.frame_nv12(k * step), W, H)
        g.enqueue_host([fr] * B)
        if k > 1:
            ok += sum(int(r.success) for r in g.wait_next())
    ok += sum(int(r.success) for r in g.wait_next())
    ms = (time.perf_counter() - t0) * 1e3 / passes
    n = g.host_redos()
    g.close()
    return n, ok, ms


for case in sys.argv[2:] or ["never"]:
    p = case.split(":")
    if p[0] == "redos":
        step, margin, on = int(p[1]), int(p[2]), len(p) > 3 and p[3] == "on"
        path = dict(period=int(p[4]), amp=float(p[5])) if len(p) > 5 else {}
        n, ok, ms = redos(step, margin, on, **path)
        print(f"pipelined host, {'period %d amp %d, ' % (path['period'], path['amp']) if path else ''}every {step}th frame, margin {margin} %, prior {'on ' if on else 'off'}: host_redos {n:3d} per 300 passes, "
              f"{ok} of {300 * B} updates succeeded, {ms:.2f} ms per pass (frame synthesis included)", flush=True)
        continue
    g, dev, keep = engine()
    if case == "on":
        g.set_motion_prior(True)
    ms = pass_ms(g, dev)
    med, mn = launch_us(g, dev)
    line = f"{'never enabled' if case == 'never' else 'motion prior on':16s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {med[0]:8.1f} us"
    if case == "on":
        line += f"  motion_place {med[1]:5.2f} us [min {mn[1]:5.2f}]  motion_settle {med[2]:5.2f} us [min {mn[2]:5.2f}]"
    print(line, flush=True)
    g.close()
