"""BGR8, RGBX, BGRX, NV21 and UYVY frames (vt_pixfmt 3-7) on the MI355X.

Every new format is a byte permutation or padding of RGB8, NV12 or YUY2 (its sibling), so every frame here is built from
a frame of the sibling by permuting or padding bytes, and every check is exact:
  * the patch matrix equals the sibling's HIP patch matrix and the oracle's on the sibling frame, for the boxes that take
    every path of the crop kernel, with every crop tier forced, for host and device frames, padded strides, a windowed
    device frame with an origin and an odd frame width where the family allows one;
  * 300 frames of traj_cfg3_300's clip in closed loop give the NV12 run's boxes, scores and flags bit for bit, through
    VitTrack and through vt_update_frame on device frames;
  * groups (synchronous host passes, pipelined passes with the redo path, subset passes, a registered zero-copy frame)
    give each stream what its sibling format gives it;
  * bad frames of the new formats are refused and change nothing."""
import ctypes
import struct

import numpy as np
import pytest

from test_gpu_trajectories import _clip, _fixture

pytestmark = pytest.mark.gpu

NEW = ["bgr8", "rgbx", "bgrx", "nv21", "uyvy"]
SIBLING = {"bgr8": "rgb8", "rgbx": "rgb8", "bgrx": "rgb8", "nv21": "nv12", "uyvy": "yuy2"}
BOXES = [(288, 208, 64, 64), (300, 200, 41, 77), (5, 3, 50, 40), (600, 440, 30, 30), (100, 100, 333, 201),
         (200, 150, 80, 80), (250, 180, 100, 70)]          # test_patch_matrix_bit_exact_nv12's: every crop path
INVALID = -1


def _nv12_to_yuy2(buf, w, h):
    """a YUY2 frame with the NV12 frame's luma and, per row, its chroma row (w even)"""
    y = buf[:w * h].reshape(h, w)
    uv = buf[w * h:w * h + w * ((h + 1) // 2)].reshape((h + 1) // 2, w // 2, 2)
    out = np.empty((h, w // 2, 4), np.uint8)
    out[..., 0], out[..., 2] = y[:, 0::2], y[:, 1::2]
    out[..., 1], out[..., 3] = uv[np.arange(h) // 2, :, 0], uv[np.arange(h) // 2, :, 1]
    return out.reshape(-1)


def _permute(fmt, sib, w, h, xbyte=0):
    """the new format's bytes from the sibling's: (H,W,3) RGB -> BGR / RGBX / BGRX, NV12 buffer -> NV21, YUY2 buffer ->
    UYVY. The x byte of the 4-byte formats is `xbyte` (never read)."""
    if fmt == "bgr8":
        return np.ascontiguousarray(sib[..., ::-1])
    if fmt in ("rgbx", "bgrx"):
        rgb = sib if fmt == "rgbx" else sib[..., ::-1]
        return np.concatenate([rgb, np.full(sib.shape[:2] + (1,), xbyte, np.uint8)], axis=2)
    if fmt == "nv21":
        out = sib.copy()
        n = ((w + 1) & ~1) * ((h + 1) // 2)
        out[w * h:w * h + n] = sib[w * h:w * h + n].reshape(-1, 2)[:, ::-1].reshape(-1)
        return out
    assert fmt == "uyvy"
    return np.ascontiguousarray(sib.reshape(-1, 4)[:, [1, 0, 3, 2]]).reshape(-1)


def _sibling_frame(gpu, sib, sc, t, w, h):
    """(sibling bytes, host frame object, oracle frame builder args)"""
    if sib == "rgb8":
        a = sc.frame_rgb8(t)
        return a, a
    buf = sc.frame_nv12(t)
    if sib == "nv12":
        return buf, gpu.NV12Frame(buf, w, h)
    y = _nv12_to_yuy2(buf, w, h)
    return y, gpu.YUY2Frame(y, w, h)


def _host(gpu, fmt, data, w, h, stride=None):
    cls = {"bgr8": gpu.BGR8Frame, "rgbx": gpu.RGBXFrame, "bgrx": gpu.BGRXFrame}
    if fmt in cls:
        return cls[fmt](data, stride)
    return (gpu.NV21Frame if fmt == "nv21" else gpu.UYVYFrame)(data, w, h)


def _oracle_frame(oracle, sib, data, w, h):
    return {"rgb8": lambda: oracle.Frame.rgb8(data), "nv12": lambda: oracle.Frame.nv12(data, w, h),
            "yuy2": lambda: oracle.Frame.yuy2(data, w, h)}[sib]()


def _device(gpu, fmt, data, w, h, stride=None):
    """(CFrame on the device, keep-alive tensor); packed formats with `stride` get rows that far apart"""
    import torch
    fmt_code = {"rgb8": gpu.PIX_RGB8, "bgr8": gpu.PIX_BGR8, "rgbx": gpu.PIX_RGBX, "bgrx": gpu.PIX_BGRX,
                "nv12": gpu.PIX_NV12, "nv21": gpu.PIX_NV21, "yuy2": gpu.PIX_YUY2, "uyvy": gpu.PIX_UYVY}[fmt]
    if fmt in ("nv12", "nv21"):
        d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        return gpu.CFrame(d.data_ptr(), d.data_ptr() + w * h, w, h, w, (w + 1) & ~1, fmt_code, 0, 0, 0, 0, 0), d
    row = data.reshape(h, -1)
    s = stride or row.shape[1]
    buf = np.zeros((h, s), np.uint8)
    buf[:, :row.shape[1]] = row
    d = torch.from_numpy(buf).cuda()
    return gpu.CFrame(d.data_ptr(), None, w, h, s, 0, fmt_code, 0, 0, 0, 0, 0), d


def _patches(trk):
    mi = trk.model_info()
    return trk.as_group().read_tensor("patches").reshape(mi.tokens_template + mi.tokens_search, mi.kpad)


def _res(r):
    return tuple(r.bbox), int(r.success), struct.unpack("<I", struct.pack("<f", r.score))[0]


# ---- 1. patch matrix, bit-exact -------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", NEW)
def test_patch_matrix_equals_the_sibling_and_the_oracle(gpu, oracle, weights_tiny, fmt):
    """host frames (and, for the packed RGB formats, rows padded to an unaligned stride) on every box of the NV12 test:
    the same patch matrix as the sibling's HIP run and the oracle's on the sibling frame"""
    w, h = 640, 480
    sib = SIBLING[fmt]
    sc = gpu.synth.MovingSquare(w, h, 64, seed=1)
    data, sib_host = _sibling_frame(gpu, sib, sc, 0, w, h)
    new = _permute(fmt, data, w, h, xbyte=77)
    variants = [_host(gpu, fmt, new, w, h)]
    if sib == "rgb8":
        variants.append(_host(gpu, fmt, new, w, h, stride=new.shape[2] * w + 5))
    of = _oracle_frame(oracle, sib, data, w, h)
    for box in BOXES:
        ref = oracle.VitTrackRef(weights_tiny)
        ref.init(of, box)
        ref.update(of, taps=True)
        want = oracle.bf16_bits_to_f32(ref.last["patches"])
        ts = gpu.VitTrack.new(weights_tiny)
        ts.init(sib_host, gpu.BBox.new(*box))
        rs = ts.update(sib_host)
        assert np.array_equal(_patches(ts), want), box
        for v in variants:
            tn = gpu.VitTrack.new(weights_tiny)
            tn.init(v, gpu.BBox.new(*box))
            rn = tn.update(v)
            assert np.array_equal(_patches(tn), want), (box, getattr(v, "stride", None))
            assert _res(rn) == _res(rs)


@pytest.mark.parametrize("fmt", NEW)
def test_every_crop_tier_device_frames_windows_and_odd_widths(gpu, weights_tiny, fmt):
    """forced crop tiers (graph replay and eager), device frames through vt_update_frame, a windowed device frame with
    an origin, and an odd frame width (packed RGB and NV21): patch matrix and result equal the sibling's"""
    sib = SIBLING[fmt]
    for (w, h) in ([(640, 480), (637, 479)] if sib != "yuy2" else [(640, 480)]):
        sc = gpu.synth.MovingSquare(w + (w & 1), h + (h & 1), 64, seed=1)
        if sib == "rgb8":
            data = sc.frame_rgb8(0)[:h, :w].copy()
        else:
            full = sc.frame_nv12(0)
            W2, H2 = w + (w & 1), h + (h & 1)
            if (W2, H2) == (w, h):
                data = full
            else:       # crop the even clip to the odd size: Y rows, then the chroma rows of (w + 1) bytes
                yy = full[:W2 * H2].reshape(H2, W2)[:h, :w]
                uv = full[W2 * H2:].reshape(H2 // 2, W2)[:(h + 1) // 2, :(w + 1) & ~1]
                data = np.concatenate([yy.reshape(-1), uv.reshape(-1)])
            if sib == "yuy2":
                data = _nv12_to_yuy2(data, w, h)
        new = _permute(fmt, data, w, h, xbyte=200)
        for box in [(288, 208, 64, 64), (200, 150, 80, 80), (600, 440, 30, 30), (100, 100, 333, 201)]:
            out = {}
            for name, d_ in ((sib, data), (fmt, new)):
                runs = []
                for tier in (-1, 0, 1, 2):
                    for use_graph in (True, False):
                        g = gpu.Group(weights_tiny, n_streams=2, use_graph=use_graph)
                        g.set_tuning("crop_tier", tier)
                        f, keep = _device(gpu, name, d_, w, h)
                        for i in range(2):
                            g.init_device(i, f, gpu.BBox.new(*box))
                        r = [g.update_device([f, f]) for _ in range(2)][-1]
                        runs.append((g.read_tensor("patches", 1).tobytes(), [_res(x) for x in r]))
                        del g
                assert all(x == runs[0] for x in runs), (name, box)
                # the single tracker on the device frame through vt_update_frame
                trk = gpu.VitTrack.new(weights_tiny)
                f, keep = _device(gpu, name, d_, w, h, stride=None)
                trk.init_device(f, gpu.BBox.new(*box))
                r1 = trk.update_device(f)
                runs.append((_patches(trk).tobytes(), [_res(r1)]))
                out[name] = runs
            assert out[fmt][0][0] == out[sib][0][0] and out[fmt][0][1] == out[sib][0][1], (fmt, w, h, box)
            assert out[fmt][-1] == out[sib][-1], (fmt, w, h, box)
            if sib == "rgb8":
                # device frames with padded rows: 16-byte aligned (the 4-byte formats' staging path with a gap after
                # every row) and unaligned (the per-pixel path)
                bpp = new.shape[2]
                for stride in (bpp * w + 16 - (bpp * w) % 16, bpp * w + 16 - (bpp * w) % 16 + 16, bpp * w + 4, bpp * w + 5):
                    trk = gpu.VitTrack.new(weights_tiny)
                    f, keep = _device(gpu, fmt, new, w, h, stride=stride)
                    trk.init_device(f, gpu.BBox.new(*box))
                    r1 = trk.update_device(f)
                    assert (_patches(trk).tobytes(), [_res(r1)]) == out[sib][-1], (fmt, w, h, box, stride)
    # a windowed device frame with an origin: the window around the box, the rest of the frame never stored
    w, h = 640, 480
    sc = gpu.synth.MovingSquare(w, h, 64, seed=1)
    data, _ = _sibling_frame(gpu, sib, sc, 0, w, h)
    new = _permute(fmt, data, w, h)
    x0, y0, ww, wh = 160, 96, 384, 320          # even, as NV12 / YUY2 windows must be
    results = {}
    for name, d_ in ((sib, data), (fmt, new)):
        import torch
        if sib == "nv12":
            yy = d_[:w * h].reshape(h, w)[y0:y0 + wh, x0:x0 + ww]
            uv = d_[w * h:].reshape(h // 2, w)[y0 // 2:(y0 + wh) // 2, x0:x0 + ww]
            buf = torch.from_numpy(np.concatenate([yy.reshape(-1), uv.reshape(-1)])).cuda()
            cf = gpu.CFrame(buf.data_ptr(), buf.data_ptr() + ww * wh, w, h, ww, ww,
                            gpu.PIX_NV12 if name == "nv12" else gpu.PIX_NV21, x0, y0, 1, ww, wh)
        else:
            bpp = {"rgb8": 3, "bgr8": 3, "rgbx": 4, "bgrx": 4, "yuy2": 2, "uyvy": 2}[name]
            rows = d_.reshape(h, -1)[y0:y0 + wh, x0 * bpp:(x0 + ww) * bpp]
            buf = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
            code = {"rgb8": gpu.PIX_RGB8, "bgr8": gpu.PIX_BGR8, "rgbx": gpu.PIX_RGBX, "bgrx": gpu.PIX_BGRX,
                    "yuy2": gpu.PIX_YUY2, "uyvy": gpu.PIX_UYVY}[name]
            cf = gpu.CFrame(buf.data_ptr(), None, w, h, ww * bpp, 0, code, x0, y0, 1, ww, wh)
        trk = gpu.VitTrack.new(weights_tiny)
        trk.init_device(cf, gpu.BBox.new(288, 208, 64, 64))
        r = trk.update_device(cf)
        results[name] = (_patches(trk).tobytes(), _res(r))
        del buf
    assert results[fmt] == results[sib]


# ---- 2. closed loop, bit-exact --------------------------------------------------------------------------------------

def test_closed_loop_cfg3_is_the_nv12_run(gpu, capsys):
    """traj_cfg3_300's clip, 300 frames, single tracker: NV21 (from the NV12 frames) and BGRX / BGR8 (from the GPU's
    nv12_to_rgb8 of them) through VitTrack, and NV21 / BGRX device frames through vt_update_frame, give the NV12 run's
    results bit for bit; the NV12 run itself stays within the committed oracle trajectory's +-1 px"""
    import torch
    name = "traj_cfg3_300.npz"
    fx = _fixture(name)
    weights = gpu.weights.ensure_weights(str(fx["config"]))
    sc = _clip(gpu, fx)
    w, h, n = sc.w, sc.h, int(fx["frames"])
    runs = ["nv12", "nv21", "bgrx", "bgr8", "nv21_dev", "bgrx_dev"]
    trk = {k: gpu.VitTrack(weights) for k in runs}
    out = {k: [] for k in runs}
    for t in range(n):
        buf = sc.frame_nv12(t)
        rgb = gpu.nv12_full_to_rgb(buf, w, h)
        nv21 = _permute("nv21", buf, w, h)
        bgrx = _permute("bgrx", rgb, w, h, xbyte=255)
        frames = {"nv12": gpu.NV12Frame(buf, w, h), "nv21": gpu.NV21Frame(nv21, w, h),
                  "bgrx": gpu.BGRXFrame(bgrx), "bgr8": gpu.BGR8Frame(rgb[..., ::-1])}
        d21, k21 = _device(gpu, "nv21", nv21, w, h)
        dbx, kbx = _device(gpu, "bgrx", bgrx, w, h)
        frames["nv21_dev"], frames["bgrx_dev"] = d21, dbx
        for k in runs:
            if t == 0:
                b = gpu.BBox.new(*sc.gt_box(0))
                trk[k].init_device(frames[k], b) if k.endswith("_dev") else trk[k].init(frames[k], b)
            r = trk[k].update_device(frames[k]) if k.endswith("_dev") else trk[k].update(frames[k])
            out[k].append(_res(r))
        torch.cuda.synchronize()
    for k in runs[1:]:
        diff = [t for t in range(n) if out[k][t] != out["nv12"][t]]
        assert not diff, f"{k}: {len(diff)} frames differ from NV12, first {diff[0]}"
    boxes = np.array([r[0] for r in out["nv12"]])
    succ = np.array([r[1] for r in out["nv12"]])
    d = np.abs(boxes - fx["bbox"])
    with capsys.disabled():
        print(f"\n[{name}, pixel formats] {n} frames: NV21, BGRX, BGR8 host and NV21, BGRX device runs bit-identical to "
              f"NV12; NV12 vs oracle max |delta| {d.max()} px, identical boxes {(d.max(axis=1) == 0).sum()}")
    assert d.max() <= 1 and np.array_equal(succ, fx["success"].astype(int))


# ---- 3. engines -----------------------------------------------------------------------------------------------------

GROUP_FMTS = ["nv12", "bgrx", "uyvy", "bgr8"]


def _group_frames(gpu, scs, t, w, h, sibling):
    """host frame objects of the four streams: the listed formats, or (sibling=True) each one's sibling"""
    out, raw = [], []
    for i, fmt in enumerate(GROUP_FMTS):
        sib = SIBLING.get(fmt, fmt)
        data, sib_host = _sibling_frame(gpu, sib, scs[i], t, w, h)
        if sibling or fmt == sib:
            out.append(sib_host)
            raw.append((sib, data))
        else:
            new = _permute(fmt, data, w, h, xbyte=13)
            out.append(_host(gpu, fmt, new, w, h))
            raw.append((fmt, new))
    return out, raw


def test_group_passes_give_each_stream_its_sibling_formats_results(gpu, weights_tiny):
    """a group of four streams (NV12, BGRX, UYVY, BGR8): synchronous host passes against device frames of the same
    formats and against a group fed the siblings; pipelined passes with the redo path forced; a subset pass"""
    w, h, B = 640, 480, 4
    scs = [gpu.synth.MovingSquare(w, h, 64, seed=60 + i) for i in range(B)]     # the clips of the pipelined NV12 test
    g_new, g_dev, g_sib = (gpu.Group(weights_tiny, n_streams=B) for _ in range(3))
    g_pipe = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1)
    g_pipe_sib = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1)
    T = 24
    new_frames = [_group_frames(gpu, scs, t, w, h, False) for t in range(T)]
    sib_frames = [_group_frames(gpu, scs, t, w, h, True) for t in range(T)]
    for i in range(B):
        b = gpu.BBox.new(*scs[i].gt_box(0))
        g_new.init_host(i, new_frames[0][0][i], b)
        g_sib.init_host(i, sib_frames[0][0][i], b)
        g_pipe.init_host(i, new_frames[0][0][i], b)
        g_pipe_sib.init_host(i, sib_frames[0][0][i], b)
        f, k = _device(gpu, *new_frames[0][1][i], w, h)
        g_dev.init_device(i, f, b)
    pipe, pipe_sib = [], []
    for t in range(1, T):
        rn = g_new.update_host(new_frames[t][0])
        rs = g_sib.update_host(sib_frames[t][0])
        dev = [_device(gpu, *new_frames[t][1][i], w, h) for i in range(B)]
        rd = g_dev.update_device([d[0] for d in dev])
        assert [_res(r) for r in rn] == [_res(r) for r in rs] == [_res(r) for r in rd], t
    # pipelined: the upload of t overlaps the pass of t - 1 (speculative windows, no enlargement: redone passes)
    g_pipe.enqueue_host(new_frames[1][0])
    g_pipe_sib.enqueue_host(sib_frames[1][0])
    for t in range(2, T):
        g_pipe.enqueue_host(new_frames[t][0])
        g_pipe_sib.enqueue_host(sib_frames[t][0])
        pipe.append([_res(r) for r in g_pipe.wait_next()])
        pipe_sib.append([_res(r) for r in g_pipe_sib.wait_next()])
    pipe.append([_res(r) for r in g_pipe.wait_next()])
    pipe_sib.append([_res(r) for r in g_pipe_sib.wait_next()])
    assert pipe == pipe_sib
    assert g_pipe.host_redos() > 0 and g_pipe.host_redos() == g_pipe_sib.host_redos()
    # a subset pass over streams 3 and 1 (BGR8, BGRX) on host and device frames
    L = [3, 1]
    rh = g_new.update_host([new_frames[T - 1][0][s] for s in L], streams=L)
    rs = g_sib.update_host([sib_frames[T - 1][0][s] for s in L], streams=L)
    dev = [_device(gpu, *new_frames[T - 1][1][s], w, h) for s in L]
    rd = g_dev.update_device([d[0] for d in dev], streams=L)
    assert [_res(r) for r in rh] == [_res(r) for r in rs] == [_res(r) for r in rd]


def test_registered_bgrx_frame_takes_the_zero_copy_route(gpu, weights_tiny):
    """a BGRX clip in registered host memory (vt_host_register) gives, single tracker and zero-copy group, what the
    same frames give from unregistered memory and what RGB8 gives; the registered frames really go to the kernels in
    place: read through the mapping as device frames they give the same results, and pipelined passes on them with
    speculative windows switched off redo nothing (a whole mapped frame cannot miss its window), where the same
    passes on unregistered memory redo"""
    w, h, n = 640, 480, 6
    sc = gpu.synth.MovingSquare(w, h, 64, seed=23)
    rgb = [sc.frame_rgb8(t) for t in range(n)]
    clip = np.stack([_permute("bgrx", a, w, h, xbyte=9) for a in rgb])
    plain = clip.copy()
    B, m = 3, 24                # the clips of the pipelined NV12 test: their targets leave unenlarged windows
    scs = [gpu.synth.MovingSquare(w, h, 64, seed=60 + i) for i in range(B)]
    pclip = np.stack([np.stack([_permute("bgrx", s.frame_rgb8(t), w, h, xbyte=5) for t in range(m)]) for s in scs])
    pplain = pclip.copy()

    def pipelined(buf):
        g = gpu.Group(weights_tiny, n_streams=B, host_zero_copy=1, host_window_margin_pct=-1)
        for i in range(B):
            g.init_host(i, gpu.BGRXFrame(buf[i, 0]), gpu.BBox.new(*scs[i].gt_box(0)))
        out = []
        g.enqueue_host([gpu.BGRXFrame(buf[i, 1]) for i in range(B)])
        for t in range(2, m):
            g.enqueue_host([gpu.BGRXFrame(buf[i, t]) for i in range(B)])
            out.append([_res(r) for r in g.wait_next()])
        out.append([_res(r) for r in g.wait_next()])
        return out, g.host_redos()

    def run(frames, zc=None):
        if zc is None:
            trk = gpu.VitTrack.new(weights_tiny)
            trk.init(frames[0], gpu.BBox.new(*sc.gt_box(0)))
            return [_res(trk.update(f)) for f in frames]
        g = gpu.Group(weights_tiny, n_streams=2, host_zero_copy=zc)
        for i in range(2):
            g.init_host(i, frames[0], gpu.BBox.new(*sc.gt_box(0)))
        return [[_res(r) for r in g.update_host([f, f])] for f in frames]

    want = (run(rgb), run(rgb, 1))
    want_pipe, redos_plain = pipelined(pplain)
    hm, hp = gpu.HostMapping(clip), gpu.HostMapping(pclip)
    try:
        got = (run([gpu.BGRXFrame(clip[t]) for t in range(n)]), run([gpu.BGRXFrame(clip[t]) for t in range(n)], 1))
        got_pipe, redos_mapped = pipelined(pclip)
        # the mapping itself: device frames at hm.d_ptr
        trk = gpu.VitTrack.new(weights_tiny)
        fb = 4 * w * h
        trk.init_device(gpu.frame_bgrx(hm.d_ptr, w, h), gpu.BBox.new(*sc.gt_box(0)))
        via_map = [_res(trk.update_device(gpu.frame_bgrx(hm.d_ptr + t * fb, w, h))) for t in range(n)]
    finally:
        hm.close()
        hp.close()
    unreg = run([gpu.BGRXFrame(plain[t]) for t in range(n)])
    assert got == want and unreg == want[0] and via_map == want[0]
    assert got_pipe == want_pipe
    assert redos_plain > 0 and redos_mapped == 0, (redos_plain, redos_mapped)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------

def test_bad_frames_of_the_new_formats_are_refused_and_change_nothing(gpu, weights_tiny):
    import torch
    L_ = gpu.lib()
    w, h = 640, 480
    sc = gpu.synth.MovingSquare(w, h, 64, seed=3)
    buf = sc.frame_nv12(0)
    d = torch.from_numpy(np.concatenate([buf, np.zeros(4 * w * h, np.uint8)])).cuda()
    p = d.data_ptr()
    trk = gpu.VitTrack.new(weights_tiny)
    trk.init_device(gpu.frame_nv12(p, p + w * h, w, h), gpu.BBox.new(*sc.gt_box(0)))
    trk.update_device(gpu.frame_nv12(p, p + w * h, w, h))
    g = trk.as_group()
    before = g.read_tensor("state").tobytes()
    F = gpu.CFrame
    bad = [F(p, None, w, h, 2 * w, 0, gpu.PIX_UYVY, 3, 0, 1, 64, 64),             # odd origin_x, UYVY
           F(p, p + w * h, w, h, w, w, gpu.PIX_NV21, 2, 3, 1, 64, 64),         # odd origin_y, NV21
           F(p, p + w * h, w, h, w, w, gpu.PIX_NV21, 3, 2, 1, 64, 64),         # odd origin_x, NV21
           F(p, None, w, h, 4 * w - 1, 0, gpu.PIX_BGRX, 0, 0, 0, 0, 0),        # stride < 4w
           F(p, None, w, h, w, w, gpu.PIX_NV21, 0, 0, 0, 0, 0),                # NV21 without a UV plane
           F(p, p + w * h, w, h, w, w, 8, 0, 0, 0, 0, 0)]                       # format 8
    r = gpu.CResult()
    for f in bad:
        assert L_.vt_update_frame(trk._h, ctypes.byref(f), 1, ctypes.byref(r)) == INVALID, (f.format, f.origin_x)
        assert L_.vt_init_frame(trk._h, ctypes.byref(f), 1, gpu.BBox.new(10, 10, 40, 40)._c()) == INVALID
        hf = gpu.CFrame(*[getattr(f, n) for n, _ in gpu.CFrame._fields_])
        if f.format != gpu.PIX_UYVY and f.origin_x == 0:      # host frames: no origin fields
            host = np.zeros(4 * w * h * 2, np.uint8)
            hf.plane0 = host.ctypes.data
            hf.plane1 = host.ctypes.data + w * h if f.plane1 else None
            assert L_.vt_update_frame(trk._h, ctypes.byref(hf), 0, ctypes.byref(r)) == INVALID
    assert L_.vt_update_frame(trk._h, ctypes.byref(gpu.frame_nv12(p, p + w * h, w, h)), 2, ctypes.byref(r)) == INVALID
    assert g.read_tensor("state").tobytes() == before
    # group entry points refuse the same frames
    grp = gpu.Group(weights_tiny, n_streams=1)
    for f in bad:
        with pytest.raises(gpu.VtError) as ei:
            grp.init_device(0, f, gpu.BBox.new(10, 10, 40, 40))
        assert ei.value.code == INVALID


# ---- 5. graphs: captured at init, never inside an update ------------------------------------------------------------

def test_no_graph_capture_inside_an_update_of_a_bgrx_stream(gpu, weights_cfg3):
    """the tier-crossing test of test_gpu_pipeline.py with a BGRX stream: the graphs of the crop kernels that read the
    byte layout are captured, all three tiers, inside the init on the first such frame; the target then grows
    through both tier boundaries and no update captures - all three tiers' graphs replay. A stream initialised on
    NV12 and then fed BGRX frames runs such passes eagerly: no capture either, and the results of a BGRX-initialised
    stream. A tuning change re-captures both sets at once."""
    import time
    import torch
    w, h = 1920, 1080
    sc = gpu.synth.MovingSquare(w, h, 64, seed=2)
    nv12 = sc.frame_nv12(0)
    rgb = gpu.nv12_full_to_rgb(nv12, w, h)
    bgrx = torch.from_numpy(_permute("bgrx", rgb, w, h, xbyte=1)).cuda()
    dnv = torch.from_numpy(nv12).cuda()
    fb = gpu.frame_bgrx(bgrx.data_ptr(), w, h)
    fn = gpu.frame_nv12(dnv.data_ptr(), dnv.data_ptr() + w * h, w, h)
    trk = gpu.VitTrack.new(weights_cfg3)
    g = trk.as_group()
    assert g.graph_captures() == 3
    trk.init_device(fb, gpu.BBox.new(900, 480, 100, 100))
    assert g.graph_captures() == 6                      # the second set, inside the init
    sizes = [100] * 20 + list(range(100, 282, 2))
    lat, res = [], []
    for s in sizes:
        g.set_state_box(0, [960 - s / 2, 540 - s / 2, s, s])
        a = time.perf_counter()
        res.append(_res(trk.update_device(fb)))
        lat.append(time.perf_counter() - a)
    assert g.graph_captures() == 6, "a pass captured a graph on the hot path"
    rep = g.read_tensor("graph_replays")
    assert rep.sum() == len(sizes) and (rep > 0).all(), rep
    steady = np.array(lat[20:])
    p50, p99 = np.median(steady), np.percentile(steady, 99)
    print(f"BGRX tier crossing: replays per tier {rep.tolist()}, update p50 {p50 * 1e3:.3f} ms, p99 {p99 * 1e3:.3f} ms")
    # the capture counter above is the exact check; a capture + instantiate costs several updates, so a stall would
    # also show here (bar wider than the NV12 test's 1.2: measured p99 / p50 = 1.19 with no capture at all)
    assert p99 <= 1.5 * p50, (p50, p99)
    g.set_tuning("head_band", 1)
    assert g.graph_captures() == 12
    g.set_tuning("head_band", -1)
    # initialised on NV12, then BGRX frames: eager passes, nothing captured, same results
    t2 = gpu.VitTrack.new(weights_cfg3)
    g2 = t2.as_group()
    t2.init_device(fn, gpu.BBox.new(900, 480, 100, 100))
    assert g2.graph_captures() == 3
    res2 = []
    for s in sizes[:30]:
        g2.set_state_box(0, [960 - s / 2, 540 - s / 2, s, s])
        res2.append(_res(t2.update_device(fb)))
    assert g2.graph_captures() == 3 and g2.read_tensor("graph_replays").sum() == 0
    t3 = gpu.VitTrack.new(weights_cfg3)
    g3 = t3.as_group()
    t3.init_device(fb, gpu.BBox.new(900, 480, 100, 100))
    res3 = []
    for s in sizes[:30]:
        g3.set_state_box(0, [960 - s / 2, 540 - s / 2, s, s])
        res3.append(_res(t3.update_device(fb)))
    assert res2 == res3 == res[:30]
