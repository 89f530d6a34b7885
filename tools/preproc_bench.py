"""Crop / resize kernel time by target size (rectangles that do not fit the tile kernel's LDS buffer).
python tools/preproc_bench.py cfg3|cfg2 [streams] [--format nv12|nv21|rgb8|bgr8|rgbx|bgrx|yuy2|uyvy|i420|yv12|p010|nv16|gray8|xrgb|xbgr] [--sizes 64,160]
(run on the GPU box; VITTRACK_HIP_LIB selects the build). --format: whole 1080p device frames of that vt_pixfmt /
vt_pixfmt2, made from the clip's NV12 frame by the byte re-arrangements of tests/test_gpu_pixel_formats.py and
tests/planar_formats_util.py (default nv12); --sizes: only these targets, no mixed-size runs."""
import sys
sys.path.insert(0, str(__import__('pathlib').Path(__file__).resolve().parents[1]))   # repo root
import numpy as np
import gstreamer_vit_tracker_amd as vt

opts = {}
args = []
it = iter(sys.argv[1:])
for a in it:
    if a in ("--format", "--sizes"):
        opts[a] = next(it)
    else:
        args.append(a)
cfg = {"cfg3": "vitb16_t192_s384", "cfg2": "vitb16_t128_s256"}[args[0] if args else "cfg3"]
B = int(args[1]) if len(args) > 1 else 30
FMT = opts.get("--format", "nv12")
SIZES = [int(v) for v in opts["--sizes"].split(",")] if "--sizes" in opts else (48, 64, 96, 128, 160, 200, 256)
w, h = 1920, 1080
weights = vt.weights.ensure_weights(cfg)
import torch


def device_frame(sc):
    """(CFrame of format FMT on the device, keep-alive tensor) from the clip's frame 0"""
    nv12 = sc.frame_nv12(0)
    if FMT in ("nv12", "nv21"):
        b = nv12.copy()
        if FMT == "nv21":
            b[w * h:] = nv12[w * h:].reshape(-1, 2)[:, ::-1].reshape(-1)
        d = torch.from_numpy(b).cuda()
        return (vt.frame_nv12 if FMT == "nv12" else vt.frame_nv21)(d.data_ptr(), d.data_ptr() + w * h, w, h), d
    if FMT in ("i420", "yv12"):
        uv = nv12[w * h:].reshape(h // 2, w // 2, 2)
        first, second = (uv[..., 0], uv[..., 1]) if FMT == "i420" else (uv[..., 1], uv[..., 0])
        d = torch.from_numpy(np.concatenate([nv12[:w * h], first.reshape(-1), second.reshape(-1)])).cuda()
        return (vt.frame_i420 if FMT == "i420" else vt.frame_yv12)(d.data_ptr(), d.data_ptr() + w * h, w, h), d
    if FMT == "p010":
        d = torch.from_numpy((nv12.astype(np.uint16) << 8).astype("<u2").view(np.uint8)).cuda()
        return vt.frame_p010(d.data_ptr(), d.data_ptr() + 2 * w * h, w, h), d
    if FMT == "nv16":
        uv = nv12[w * h:].reshape(h // 2, w)[np.arange(h) // 2]
        d = torch.from_numpy(np.concatenate([nv12[:w * h], uv.reshape(-1)])).cuda()
        return vt.frame_nv16(d.data_ptr(), d.data_ptr() + w * h, w, h), d
    if FMT == "gray8":
        d = torch.from_numpy(nv12[:w * h].copy()).cuda()
        return vt.frame_gray8(d.data_ptr(), w, h), d
    if FMT in ("yuy2", "uyvy"):
        y = nv12[:w * h].reshape(h, w)
        uv = nv12[w * h:].reshape(h // 2, w // 2, 2)[np.arange(h) // 2]
        p = np.stack([y[:, 0::2], uv[..., 0], y[:, 1::2], uv[..., 1]], axis=2)
        if FMT == "uyvy":
            p = p[..., [1, 0, 3, 2]]
        d = torch.from_numpy(np.ascontiguousarray(p).reshape(-1)).cuda()
        return vt.CFrame(d.data_ptr(), None, w, h, 2 * w, 0, vt.PIX_YUY2 if FMT == "yuy2" else vt.PIX_UYVY,
                         0, 0, 0, 0, 0), d
    rgb = vt.nv12_full_to_rgb(nv12, w, h)
    c = rgb[..., ::-1] if FMT in ("bgr8", "bgrx", "xbgr") else rgb
    if FMT in ("rgbx", "bgrx"):
        c = np.concatenate([c, np.zeros((h, w, 1), np.uint8)], axis=2)
    if FMT in ("xrgb", "xbgr"):
        c = np.concatenate([np.zeros((h, w, 1), np.uint8), c], axis=2)
    d = torch.from_numpy(np.ascontiguousarray(c)).cuda()
    helper = {"rgb8": vt.frame_rgb8, "bgr8": vt.frame_bgr8, "rgbx": vt.frame_rgbx, "bgrx": vt.frame_bgrx,
              "xrgb": vt.frame_xrgb, "xbgr": vt.frame_xbgr}[FMT]
    return helper(d.data_ptr(), w, h), d


for sq in SIZES:
    sc = vt.synth.MovingSquare(w, h, sq, seed=1)
    fr, buf = device_frame(sc)
    grp = vt.Group(weights, n_streams=B)
    for i in range(B):
        grp.init_device(i, fr, vt.BBox.new(*sc.gt_box(0)))
    us = []
    for _ in range(3):
        for i in range(B):
            grp.set_state_box(i, [float(v) for v in sc.gt_box(0)])     # the crop is cut around THIS box every time
        prof = grp.profile_device([fr] * B, iters=1)
        us.append([p["ms"] * 1e3 for p in prof if p["name"] == "preproc_search"][0])
    print(f"{cfg} {B} streams, {FMT}, target {sq:3d} px (crop side {4 * sq} px): preproc {np.median(us):6.1f} us (min {min(us):6.1f})", flush=True)
    del grp

# mixed target sizes in ONE engine: the tier of a pass is the largest any stream needs, so one large target puts every stream's
# tiles on the big buffer (2 blocks per CU at 64 KiB instead of 8 at 16 KiB)
for big in ((160, 200, 256) if "--sizes" not in opts else ()):
    scs = [vt.synth.MovingSquare(w, h, 64, seed=1)] * (B - 1) + [vt.synth.MovingSquare(w, h, big, seed=1)]
    bufs = {id(s): torch.from_numpy(s.frame_nv12(0)).cuda() for s in scs}
    frs = [vt.frame_nv12(bufs[id(s)].data_ptr(), bufs[id(s)].data_ptr() + w * h, w, h) for s in scs]
    grp = vt.Group(weights, n_streams=B)
    for i in range(B):
        grp.init_device(i, frs[i], vt.BBox.new(*scs[i].gt_box(0)))
    us = []
    for _ in range(3):
        for i in range(B):
            grp.set_state_box(i, [float(v) for v in scs[i].gt_box(0)])
        prof = grp.profile_device(frs, iters=1)
        us.append([p["ms"] * 1e3 for p in prof if p["name"] == "preproc_search"][0])
    print(f"{cfg} {B} streams, {B - 1} targets of 64 px + ONE of {big} px: preproc {np.median(us):6.1f} us (min {min(us):6.1f})", flush=True)
    del grp
