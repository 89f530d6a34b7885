"""Reacquire proposals: what a never-enabled engine pays (nothing), what the four launches of an enabled one take per pass
with 0, 1 and 30 streams due, and what Group.reacquire takes on the fixture's jump frame with and without them.
cfg3 x 30 streams, device-resident 1080p NV12 (the `reacquire` case: cfg2 x 30, the committed clip).
usage: python tools/proposals_cost.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("."); VITTRACK_HIP_LIB selects another build of the library (the parent
commit's, for case `never`). CASE:
  never          no proposals key ever set: ms per device pass (vt_group_enqueue_device + vt_group_wait), three runs of 40,
                 and the sum of the kernel times of vt_group_profile_device
  due0           "proposals" 1 and every update succeeds: four launches that leave at once
  due1           "proposals" 1 and stream 0 is shown a frame without its target where it looks: one stream due in every pass
  due30          "proposals" 2: every stream due in every pass
  reacquire      the jump frame of tests/golden/make_reacquire.py on stream 0 of a cfg2 x 30 engine: wall time of
                 Group.reacquire by the scan and with proposals=True, the target present (found) and painted out (absent)
For each enabled case: the four launches' own begin -> end times, medians over 20 profiled passes [and the minimum]."""
import os
import sys
import time

root = os.path.abspath(sys.argv[1])
sys.path.insert(0, root)
import numpy as np
import torch
import gstreamer_vit_tracker_amd as vt

B, W, H = 30, 1920, 1080
NAMES = ("proposals_prepare", "proposals_thumb", "proposals_match", "proposals_list")


def dev_frame(buf):
    d = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    return vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H), d


def engine(cfg="cfg3", square=64):
    scs = [vt.synth.MovingSquare(W, H, square, seed=s) for s in range(B)]
    g = vt.Group(vt.weights.ensure_weights(cfg), n_streams=B)
    for s, sc in enumerate(scs):
        f, d = dev_frame(sc.frame_nv12(0))
        g.init_device(s, f, vt.BBox.new(*sc.gt_box(0)))
    pairs = [dev_frame(sc.frame_nv12(1)) for sc in scs]
    return g, [p[0] for p in pairs], pairs, scs


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


def launch_us(g, dev, passes=20):
    rows = []
    for _ in range(passes):
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        rows.append([sum(d.values())] + [d.get(n, 0.0) for n in NAMES])
    return np.array(rows)


def fmt(a):
    return "  ".join(f"{n[10:]} {np.median(a[:, 1 + i]):7.2f} us [min {a[:, 1 + i].min():7.2f}]" for i, n in enumerate(NAMES))


def reacquire_case():
    sys.path.insert(0, os.path.join(root, "tests", "golden"))
    import make_reacquire as mr
    frame, gt = mr.clip()
    absent = vt.synth.MovingSquare(W, H, mr.SQ, seed=0, center=(0.23 * W, 0.71 * H), amp=0.05 * min(W, H), hide=(0, 1000))
    for what, jump_buf in (("found", frame(mr.JUMP_AT)), ("absent", absent.frame_nv12(mr.JUMP_AT))):
        for use in (False, True):
            others = [vt.synth.MovingSquare(W, H, 56 + 2 * (i % 9), seed=100 + i) for i in range(1, B)]
            g = vt.Group(vt.weights.ensure_weights("cfg2"), n_streams=B)
            if use:
                g.set_proposals(1)
            for t in range(mr.JUMP_AT + 1):
                bufs = [frame(t) if t < mr.JUMP_AT else jump_buf] + [sc.frame_nv12(t) for sc in others]
                pairs = [dev_frame(b) for b in bufs]
                if t == 0:
                    g.init_device(0, pairs[0][0], vt.BBox.new(*gt(0)))
                    for i, sc in enumerate(others, start=1):
                        g.init_device(i, pairs[i][0], vt.BBox.new(*sc.gt_box(0)))
                res = g.update_device([p[0] for p in pairs])
            assert not res[0].success
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            best = g.reacquire(0, pairs[0][0], proposals=use)
            ms = (time.perf_counter() - t0) * 1e3
            n_prop = len(g.last_proposal_pass[0]) if g.last_proposal_pass else 0
            print(f"reacquire {what:6s} {'proposals' if use else 'scan     '} {ms:8.2f} ms   proposal slots {n_prop}, scan chunks "
                  f"{len(g.last_scan)} ({sum(len(r) for r, _ in g.last_scan)} windows)   -> success {int(best.success)} "
                  f"score {best.score:.4f} box {list(best.bbox)}", flush=True)
            g.close()


for case in sys.argv[2:] or ["never"]:
    if case == "reacquire":
        reacquire_case()
        continue
    g, dev, keep, scs = engine()
    if case in ("due0", "due1"):
        g.set_proposals(1)
    elif case == "due30":
        g.set_proposals(2)
    if case == "due1":      # stream 0: the scene with its target far from where the stream looks
        far = vt.synth.MovingSquare(W, H, 64, seed=0, center=(0.23 * W, 0.71 * H), amp=0.05 * min(W, H))
        keep.append(dev_frame(far.frame_nv12(1)))
        dev[0] = keep[-1][0]
    ms = pass_ms(g, dev)
    a = launch_us(g, dev)
    print(f"{case:8s} device pass ms {' '.join(f'{v:.4f}' for v in ms)}   kernels/pass {np.median(a[:, 0]):8.1f} us", flush=True)
    if case != "never":
        recs = [g.proposals(s) for s in range(B)]
        print(f"         {fmt(a)}   (last pass: {sum(r['status'] == 1 for r in recs)} streams evaluated; stream 0: n {recs[0]['n']}, "
              f"grid {recs[0]['grid']}, best {recs[0]['proposals'][0]['sim'] if recs[0]['n'] else 0:.4f})", flush=True)
    g.close()
