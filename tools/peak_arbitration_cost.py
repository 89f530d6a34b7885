"""Peak arbitration: what a never-enabled engine pays (nothing), and what the four launches of an enabled one take per pass.
usage: python tools/peak_arbitration_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE, all on cfg3 x 30 streams, device-resident 1080p NV12:
  never     no arbitrate key ever set: ms per device pass (vt_group_enqueue_device + vt_group_wait), three runs of 40, and the
            sum of the kernel times of vt_group_profile_device
  idle      "arbitrate" 1 with min_resp 1000 per mille: no runner-up is ever listed, nothing is due
  all       K = 4, min_resp 0 and an engine whose success threshold is 1e-6: every listed runner-up that passes rule 6 is cut and
            scored; the records say how many streams were due and how many peaks were scored
  one       as `all`, but "arbitrate_min_resp_pm" placed between the largest and the second-largest runner-up response of the
            thirty streams (read from the records of a pass under `all`): one stream lists a runner-up, the others list none.
            The records must say "1 of 30 streams due"; if no per-mille value separates the two responses on a frame, the next
            frame of the clip is tried
  off       enabled once, then "arbitrate" 0: four launches that leave at once
For each enabled case: the four launches' own begin -> end times, medians over the profiled passes, and their sum."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt

NAMES = ("arbitrate_list", "arbitrate_probe", "arbitrate_score", "arbitrate_commit")


def engine(B=30, W=1920, H=1080, frame=1, **kw):
    w = vt.weights.ensure_weights("cfg3")
    scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    g = vt.Group(w, n_streams=B, **kw)
    first = [torch.from_numpy(sc.frame_nv12(0)).cuda() for sc in scs]
    for s in range(B):
        g.init_device(s, vt.frame_nv12(first[s].data_ptr(), first[s].data_ptr() + W * H, W, H), vt.BBox.new(*scs[s].gt_box(0)))
    keep = [torch.from_numpy(sc.frame_nv12(frame)).cuda() for sc in scs]
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


def settle(g, dev, n=10):
    for _ in range(n):
        g.enqueue_device(dev)
        g.wait()
    return [g.arbitration(s) for s in range(g.streams)]


def one_due():
    """-> (engine, frames, keep-alive tensors) with exactly one stream due, or None"""
    for frame in range(1, 9):
        g, dev, keep = engine(frame=frame, success_threshold=1e-6)
        g.set_appearance(True)
        g.set_arbitration(True, max=4, radius=1, min_resp_pm=0)
        recs = settle(g, dev)
        # the runner-up response of every stream that is due under `all` (peak 1 leads the later ones)
        resp = sorted((float(r["peaks"][1]["resp"]) for r in recs if r["status"] in (1, 2) and r["n"] >= 2), reverse=True)
        pm = int(np.floor(resp[0] * 1000.0)) if resp else 0
        if len(resp) >= 2 and pm >= 1 and np.float32(pm) / np.float32(1000.0) > np.float32(resp[1]):
            g.set_tuning("arbitrate_min_resp_pm", pm)
            recs = settle(g, dev)
            if sum(r["status"] in (1, 2) for r in recs) == 1:
                print(f"one     frame {frame}: runner-up responses {resp[0]:.4f}, {resp[1]:.4f}, ...; min_resp {pm} per mille", flush=True)
                return g, dev, keep
        print(f"one     frame {frame}: not separable (runner-up responses {[round(v, 4) for v in resp[:3]]}, {pm} per mille)", flush=True)
        g.close()
    return None


for case in sys.argv[2:] or ["never"]:
    if case == "one":
        found = one_due()
        if found is None:
            print("one     no frame of the clip separates one stream's runner-up from the others'", flush=True)
            continue
        g, dev, keep = found
    else:
        g, dev, keep = engine(**({"success_threshold": 1e-6} if case == "all" else {}))
    if case not in ("never", "one"):
        g.set_appearance(True)
        if case == "all":
            g.set_arbitration(True, max=4, radius=1, min_resp_pm=0)
        else:
            g.set_arbitration(True, min_resp_pm=1000)
        if case == "off":
            g.set_arbitration(False)
    ms = pass_ms(g, dev)
    a = launch_us(g, dev, 20)
    print(f"{case:7s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {np.median(a[:, 0]):8.1f} us", flush=True)
    if case != "never":
        m = np.median(a[:, 1:], axis=0)
        recs = [g.arbitration(s) for s in range(g.streams)]
        due = sum(r["status"] in (1, 2) for r in recs)
        scored = sum(sum(p["status"] in (1, 3) for p in r["peaks"]) for r in recs if r["status"] in (1, 2))
        print("        " + "  ".join(f"{k[10:]} {v:6.2f}" for k, v in zip(NAMES, m)) + f"  sum {m.sum():6.2f} us   ({due} of {g.streams} streams "
              f"due, {scored} peaks scored, {sum(r['status'] == 2 for r in recs)} switched in the last pass)", flush=True)
    g.close()
