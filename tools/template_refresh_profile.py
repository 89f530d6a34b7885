"""Template refresh: what an enabled engine pays per pass. cfg3 x 30 streams, 1080p NV12 device frames, per-pass times of
vt_group_profile_device (medians over 20 passes): sum of kernels, gather_template, refresh_template, preproc_search.
usage: python tools/template_refresh_profile.py TREE_ROOT [refresh]   (TREE_ROOT: the checkout whose package is loaded, "." or
a parent-commit tree built beside it; "refresh": also the enabled cases)"""
import sys, os
root = os.path.abspath(sys.argv[1]); sys.path.insert(0, root)
import numpy as np, torch
import gstreamer_vit_tracker_amd as vt
refresh = len(sys.argv) > 2
B, W, H = 30, 1920, 1080
w = vt.weights.ensure_weights("cfg3")
scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
def frames(t):
    keep = [torch.from_numpy(sc.frame_nv12(t)).cuda() for sc in scs]
    return [vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H) for d in keep], keep
g = vt.Group(w, n_streams=B)
f0, k0 = frames(0)
for s in range(B):
    g.init_device(s, f0[s], vt.BBox.new(*scs[s].gt_box(0)))
def one(fr):
    fams = g.profile_device(fr, iters=1)
    d = {f["name"]: f["ms"] * 1e3 for f in fams}
    return sum(d.values()), d.get("gather_template", 0.0), d.get("refresh_template", 0.0), d.get("preproc_search", 0.0)
f1, k1 = frames(1)
for _ in range(6): g.update_device(f1)          # warm
def stats(rows, tag):
    a = np.array(rows)
    print(f"{tag:34s} n={len(rows):2d}  pass(sum of kernels) {np.median(a[:,0]):8.1f} us  gather {np.median(a[:,1]):6.2f} us  refresh {np.median(a[:,2]):6.2f} us  preproc_search {np.median(a[:,3]):6.2f} us   [medians; min pass {a[:,0].min():.1f}]")
rows = [one(f1) for _ in range(20)]
stats(rows, "never enabled")
if refresh:
    g.set_template_refresh(1000000, 0.0)
    rows = [one(f1) for _ in range(20)]
    stats(rows, "enabled, period 1e6 (none fire)")
    g.set_template_refresh(2, 0.0)
    fire, idle = [], []
    for _ in range(40):
        g0 = [g.template_refresh_stats(s)["generation"] for s in range(B)]
        r = one(f1)
        n = sum(g.template_refresh_stats(s)["generation"] - g0[s] for s in range(B))
        (fire if n == B else idle if n == 0 else []).append(r)
    stats(idle, "enabled, period 2, pass w/o refresh")
    stats(fire, "enabled, period 2, all 30 fire")
    print("skipped_geometry", sum(g.template_refresh_stats(s)["skipped_geometry"] for s in range(B)))
g.close()
