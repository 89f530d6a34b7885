"""Response peaks: what a never-enabled engine pays (nothing) and what an enabled one pays per pass. cfg3 x 30 streams,
1080p NV12 HOST frames, 64-px targets.
usage: python tools/response_peaks_profile.py TREE_ROOT [CASE ...]
TREE_ROOT: the checkout whose package is loaded ("." or a parent-commit tree built beside it). CASE:
  never       no policy ever set (the only case a parent tree can run): ms per synchronous host pass, three runs of 40
  K:R[:one]   max_peaks K at radius R on all 30 streams (":one": on stream 7 of 30): ms per host pass as above, and from
              vt_group_profile_device (device frames, one pass at a time, medians over 20) the response_peaks launch's own
              event time beside the decode tail's
  lookalike   a 1080p clip whose frames carry a pixel copy of the 96-px target 1.5 box sides to its right, one stream with
              the fitted cfg3 head, K 8 at R 2, min_resp 0.05: per frame the peaks listed, how far peak 1's box centre lies
              from the copy's, and whether a candidate slot placed at peak 1's box locks on to the copy in the next frame
VITTRACK_HIP_LIB selects a tuning build of the library."""
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


def engine(scs):
    g = vt.Group(w, n_streams=len(scs))
    for s, sc in enumerate(scs):
        g.init_host(s, vt.NV12Frame(sc.frame_nv12(0), W, H), vt.BBox.new(*sc.gt_box(0)))
    return g


def host_ms(g, frames, runs=3, n=40):
    out = []
    for _ in range(runs):
        for _ in range(5):
            g.update_host(frames)
        t0 = time.perf_counter()
        for _ in range(n):
            g.update_host(frames)
        out.append((time.perf_counter() - t0) * 1e3 / n)
    return out


def launch_us(g, dev):
    rows = []
    for _ in range(20):
        d = {f["name"]: f["ms"] * 1e3 for f in g.profile_device(dev, iters=1)}
        tail = d.get("head_conv3x3_logits_decode", d.get("decode", 0.0))
        rows.append((sum(d.values()), d.get("response_peaks", 0.0), tail))
    a = np.array(rows)
    return np.median(a, axis=0), a[:, 1].min()


def lookalike():
    sq = 96
    sc = vt.synth.MovingSquare(W, H, sq, seed=3)
    off = int(1.5 * sq)

    def frame(t):
        rgb = sc.frame_rgb8(t)
        x, y, s, _ = sc.gt_box(t)
        x2 = min(x + off, W - s)
        rgb[y:y + s, x2:x2 + s] = rgb[y:y + s, x:x + s].copy()
        return rgb, (x2, y, s, s)

    g = vt.Group(w, n_streams=2)
    rgb0, _ = frame(0)
    g.init_host(0, rgb0, vt.BBox.new(*sc.gt_box(0)))
    g.set_peaks(8, 2, 0.05, stream=0)
    print("lookalike: t  result(success score box)  n  resp[0..n)  |peak1 - copy| px  candidate at peak 1 -> box, IoU with the copy", flush=True)
    for t in range(1, 13):
        rgb, copy = frame(t)
        r = g.update_host([rgb], streams=[0])[0]
        rec = g.last_peaks(1)[0]
        n = int(rec["n"])
        line = f"  t={t:2d}  {int(r.success)} {r.score:.3f} {tuple(r.bbox)}  n={n}  resp {np.round(rec['peak']['resp'][:n], 3).tolist()}"
        if n >= 2:
            b = rec["peak"]["box"][1]
            d = float(np.hypot(b[0] + b[2] / 2 - (copy[0] + copy[2] / 2), b[1] + b[3] / 2 - (copy[1] + copy[3] / 2)))
            line += f"  peak1 box {np.round(b, 1).tolist()} dist {d:.1f}"
            # the next frame, two candidate slots of stream 0: its own box, and peak 1's box. A twin engine keeps the clip's
            # own track untouched: the probe runs on a copy of the stream
            probe = vt.Group(w, n_streams=2)
            g.copy_stream(0, probe, 0)
            rgb2, copy2 = frame(t + 1)
            res, win = probe.update_host_candidates([(0, None), (0, [float(v) for v in b])], [rgb2, rgb2])
            cb = tuple(res[1].bbox)
            ix = max(0, min(cb[0] + cb[2], copy2[0] + copy2[2]) - max(cb[0], copy2[0]))
            iy = max(0, min(cb[1] + cb[3], copy2[1] + copy2[3]) - max(cb[1], copy2[1]))
            iou = ix * iy / float(cb[2] * cb[3] + copy2[2] * copy2[3] - ix * iy)
            line += f"  cand {int(res[1].success)} {res[1].score:.3f} {cb} IoU {iou:.2f} winner slot {win[0]}"
            probe.close()
        print(line, flush=True)
    g.close()


for case in sys.argv[2:] or ["never"]:
    if case == "lookalike":
        lookalike()
        continue
    scs = [vt.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    g = engine(scs)
    bufs = [sc.frame_nv12(1) for sc in scs]
    frames = [vt.NV12Frame(b, W, H) for b in bufs]
    tag = "never enabled"
    if case != "never":
        p = case.split(":")
        K, R = int(p[0]), int(p[1])
        one = len(p) > 2 and p[2] == "one"
        g.set_peaks(K, R, 0.0, stream=7 if one else None)
        tag = f"K {K} R {R} on {'stream 7 of 30' if one else 'all 30'}"
    ms = host_ms(g, frames)
    line = f"{tag:28s} host pass ms {' '.join(f'{v:.4f}' for v in ms)}"
    keep = [torch.from_numpy(b).cuda() for b in bufs]
    dev = [vt.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H) for d in keep]
    med, mn = launch_us(g, dev)
    line += f"   kernels/pass {med[0]:8.1f} us  decode tail {med[2]:6.2f} us"
    if case != "never":
        rec = g.last_peaks()
        line += f"  response_peaks {med[1]:5.2f} us [min {mn:5.2f}]  peaks listed {rec['n'].min()}..{rec['n'].max()}"
    print(line, flush=True)
    g.close()
