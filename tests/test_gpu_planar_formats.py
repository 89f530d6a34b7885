"""I420, YV12, P010, NV16, GRAY8, XRGB and XBGR frames (vt_pixfmt2) on the MI355X.

Every new format is DEFINED as a byte re-arrangement of RGB8, NV12 or YUY2 (its sibling; planar_formats_util.py builds
one from the other), so every check is exact:
  1. the patch matrix equals the sibling's HIP patch matrix and the oracle's on the sibling frame: every crop path and
     forced tier, host and device frames, aligned strides (the wide staging paths) and unaligned padded ones (the
     per-pixel path), packed windows and pointer-offset views with an origin, odd frame sizes;
  2. bytes that are not sampled do not matter: P010 low bytes, the x byte, row padding, bytes beyond a stored window,
     the bytes between planes;
  3. 60 frames of traj_cfg2_300's clip in closed loop give the sibling run's boxes, score bits and flags;
  4. groups - synchronous, pipelined with the redo path, subsets, a registered zero-copy frame, a candidate pass sharing
     one host frame - give every stream what its sibling format gives it in a twin engine;
  5. template refresh and target chips give the sibling's template rows and chip bytes;
  6. graphs are captured at the first init on such a format, never inside an update;
  7. bad frames are refused and change nothing."""
import ctypes
import struct

import numpy as np
import pytest

import planar_formats_util as U
from test_gpu_pixel_formats import BOXES, _nv12_to_yuy2
from test_gpu_trajectories import _clip, _fixture

pytestmark = pytest.mark.gpu

NEW = U.NEW
SIBLING = U.SIBLING
INVALID = -1
ODD_OK = [f for f in NEW if f != "nv16"]


def _code(gpu, fmt):
    return getattr(gpu, "PIX_" + fmt.upper())


def _res(r):
    return tuple(r.bbox), int(r.success), struct.unpack("<I", struct.pack("<f", r.score))[0]


def _patches(trk):
    mi = trk.model_info()
    return trk.as_group().read_tensor("patches").reshape(mi.tokens_template + mi.tokens_search, mi.kpad)


def _crop_nv12(full, W2, H2, w, h):
    """the packed NV12 frame of the top-left w x h pixels of an even-sized one"""
    if (W2, H2) == (w, h):
        return full
    cw, ch = U.chroma_dims(w, h)
    yy = full[:W2 * H2].reshape(H2, W2)[:h, :w]
    uv = full[W2 * H2:].reshape(H2 // 2, W2)[:ch, :2 * cw]
    return np.concatenate([yy.reshape(-1), uv.reshape(-1)])


def _sibling_data(gpu, fmt, sc, t, w, h):
    """the sibling format's packed bytes of frame t, cut to w x h: an NV12 / YUY2 buffer, or an (H,W,3) array - for GRAY8 the
    grey image of the clip's luma"""
    W2, H2 = sc.w, sc.h
    nv12 = _crop_nv12(sc.frame_nv12(t), W2, H2, w, h)
    sib = SIBLING[fmt]
    if sib == "nv12":
        return nv12
    if sib == "yuy2":
        return _nv12_to_yuy2(nv12, w, h)
    if fmt == "gray8":
        return U.gray8_to_rgb8(nv12[:w * h].reshape(h, w))
    return sc.frame_rgb8(t)[:h, :w].copy()


def _host(gpu, fmt, data, w, h):
    """host frame object of any format from its packed bytes"""
    cls = {"nv12": gpu.NV12Frame, "yuy2": gpu.YUY2Frame, "i420": gpu.I420Frame, "yv12": gpu.YV12Frame, "p010": gpu.P010Frame,
           "nv16": gpu.NV16Frame}
    if fmt in cls:
        return cls[fmt](data, w, h)
    if fmt == "rgb8":
        return data
    return {"gray8": gpu.Gray8Frame, "xrgb": gpu.XRGBFrame, "xbgr": gpu.XBGRFrame}[fmt](data)


def _oracle_frame(oracle, sib, data, w, h):
    if sib == "nv12":       # Frame.nv12 takes the chroma stride for the width: an odd width needs it said
        buf = np.ascontiguousarray(data, np.uint8).reshape(-1)
        return oracle.Frame(1, buf[:w * h], buf[w * h:], w, h, w, (w + 1) & ~1)
    return {"rgb8": lambda: oracle.Frame.rgb8(data), "yuy2": lambda: oracle.Frame.yuy2(data, w, h)}[sib]()


def _planes(fmt, data, w, h):
    """(plane 0, plane 1 or None) of a packed frame as 2-D byte arrays [rows][row bytes]; the two chroma planes of I420 /
    YV12 are ONE array of 2 * ceil(h/2) rows (the second plane lies stride1 * ceil(h/2) bytes behind the first)"""
    cw, ch = U.chroma_dims(w, h)
    d = np.asarray(data, np.uint8).reshape(-1)
    if fmt in ("nv12", "nv21"):
        return d[:w * h].reshape(h, w), d[w * h:w * h + 2 * cw * ch].reshape(ch, 2 * cw)
    if fmt in ("i420", "yv12"):
        return d[:w * h].reshape(h, w), d[w * h:w * h + 2 * cw * ch].reshape(2 * ch, cw)
    if fmt == "p010":
        return d[:2 * w * h].reshape(h, 2 * w), d[2 * w * h:2 * w * h + 4 * cw * ch].reshape(ch, 4 * cw)
    if fmt == "nv16":
        return d[:w * h].reshape(h, w), d[w * h:2 * w * h].reshape(h, w)
    return d.reshape(h, -1), None


def _window_planes(fmt, p0, p1, w, h, x0, y0, ww, wh):
    """the planes of the window (x0, y0, ww, wh) of a frame's planes: x0, y0 even where the format has chroma"""
    bpp = p0.shape[1] // w
    q0 = p0[y0:y0 + wh, x0 * bpp:(x0 + ww) * bpp]
    if p1 is None:
        return q0, None
    if fmt in ("i420", "yv12"):
        ch = (h + 1) // 2
        r0, r1, c0, c1 = y0 // 2, (y0 + wh + 1) // 2, x0 // 2, (x0 + ww + 1) // 2
        return q0, np.concatenate([p1[r0:r1, c0:c1], p1[ch + r0:ch + r1, c0:c1]])
    if fmt == "nv16":
        return q0, p1[y0:y0 + wh, x0:x0 + ww]
    return q0, p1[y0 // 2:(y0 + wh + 1) // 2, x0 * bpp:((x0 + ww + 1) & ~1) * bpp]


def _device(gpu, fmt, data, w, h, aligned=True, fill=0, window=None, view=None):
    """(CFrame of device memory, keep-alive tensor) from a frame's packed bytes.
    aligned: every plane starts on a 256-byte boundary with a stride that is a multiple of 16 (the wide staging paths);
    else odd strides with 5-13 bytes of padding and odd plane starts (the per-pixel path). fill: the byte (or a Generator
    for random bytes) of everything that is not a sample of the frame - padding, gaps between the planes.
    window = (x0, y0, ww, wh): only that window is stored (windowed = 1); view = (x0, y0, ww, wh): the whole frame is
    stored and the pointers are offset to the window's first pixel (windowed = 0)"""
    import torch
    p0, p1 = _planes(fmt, data, w, h)
    bpp = p0.shape[1] // w
    x0 = y0 = ww = wh = 0
    if window:
        x0, y0, ww, wh = window
        p0, p1 = _window_planes(fmt, p0, p1, w, h, x0, y0, ww, wh)

    def pitch(n, extra):
        return (n + 15) // 16 * 16 + (16 if extra else 0) if aligned else n + extra

    s0 = pitch(p0.shape[1], 5)
    s1 = pitch(p1.shape[1], 13) if p1 is not None else 0
    off0 = 0 if aligned else 3
    off1 = (off0 + s0 * p0.shape[0] + 255) // 256 * 256 + (0 if aligned else 7)
    total = off1 + (s1 * p1.shape[0] if p1 is not None else 0) + 64
    if isinstance(fill, np.random.Generator):
        buf = fill.integers(0, 256, total, dtype=np.uint8)
    else:
        buf = np.full(total, fill, np.uint8)
    buf[off0:off0 + s0 * p0.shape[0]].reshape(-1, s0)[:, :p0.shape[1]] = p0
    if p1 is not None:
        buf[off1:off1 + s1 * p1.shape[0]].reshape(-1, s1)[:, :p1.shape[1]] = p1
    d = torch.from_numpy(buf).cuda()
    a0, a1 = d.data_ptr() + off0, (d.data_ptr() + off1 if p1 is not None else None)
    if view:
        x0, y0, ww, wh = view
        a0 += y0 * s0 + x0 * bpp
        if p1 is not None:
            a1 += {"i420": (y0 // 2) * s1 + x0 // 2, "yv12": (y0 // 2) * s1 + x0 // 2, "nv16": y0 * s1 + x0}.get(
                fmt, (y0 // 2) * s1 + x0 * bpp)
    return gpu.CFrame(a0, a1, w, h, s0, s1, _code(gpu, fmt), x0, y0, 1 if window else 0, ww, wh), d


def _frames_of(gpu, fmt, sc, t, w, h, rng=None, xbyte=0):
    """(sibling name, sibling bytes, new bytes) of frame t"""
    sib = _sibling_data(gpu, fmt, sc, t, w, h)
    return SIBLING[fmt], sib, U.from_sibling(fmt, sib, w, h, rng=rng, xbyte=xbyte)


# ---- 1. patch matrix, bit-exact -------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", NEW)
def test_patch_matrix_equals_the_sibling_and_the_oracle(gpu, oracle, weights_tiny, fmt):
    """every box of the NV12 test (every crop path) with every crop tier forced: host frames, device frames with aligned
    strides (the wide groups) and with unaligned padded strides (pixel by pixel) give the sibling's HIP patch matrix, the
    oracle's on the sibling frame, and the sibling's result"""
    w, h = 640, 480
    sc = gpu.synth.MovingSquare(w, h, 64, seed=1)
    sib, sdata, ndata = _frames_of(gpu, fmt, sc, 0, w, h, rng=np.random.default_rng(5), xbyte=77)
    of = _oracle_frame(oracle, sib, sdata, w, h)
    trk = {k: gpu.VitTrack.new(weights_tiny, use_graph=False) for k in ("sib", "host", "wide", "pixel")}
    fr = {"sib": _host(gpu, sib, sdata, w, h), "host": _host(gpu, fmt, ndata, w, h)}
    fr["wide"], k1 = _device(gpu, fmt, ndata, w, h, aligned=True, fill=0xA5)
    fr["pixel"], k2 = _device(gpu, fmt, ndata, w, h, aligned=False, fill=0x5A)
    for box in BOXES:
        ref = oracle.VitTrackRef(weights_tiny)
        ref.init(of, box)
        ref.update(of, taps=True)
        want = oracle.bf16_bits_to_f32(ref.last["patches"])
        for tier in (0, 1, 2):
            res = {}
            for k, t in trk.items():
                t.as_group().set_tuning("crop_tier", tier)
                if k in ("wide", "pixel"):
                    t.init_device(fr[k], gpu.BBox.new(*box))
                    res[k] = _res(t.update_device(fr[k]))
                else:
                    t.init(fr[k], gpu.BBox.new(*box))
                    res[k] = _res(t.update(fr[k]))
                assert np.array_equal(_patches(t), want), (fmt, k, box, tier)
            assert all(v == res["sib"] for v in res.values()), (fmt, box, tier, res)


@pytest.mark.parametrize("fmt", NEW)
def test_windows_views_graphs_and_odd_sizes(gpu, oracle, weights_tiny, fmt):
    """a packed window (windowed = 1) and a pointer-offset view into the whole frame (origin set, windowed = 0), aligned
    and not, give the whole sibling frame's patch matrix and result; so do the graph replays of a group with every tier
    forced; and an odd width and height (all but NV16) on host and device frames, with a window that ends at the
    frame's odd edge, against the sibling and the oracle"""
    for (w, h) in ([(640, 480), (637, 479)] if fmt in ODD_OK else [(640, 480)]):
        sc = gpu.synth.MovingSquare(w + (w & 1), h + (h & 1), 64, seed=1)
        sib, sdata, ndata = _frames_of(gpu, fmt, sc, 0, w, h, rng=np.random.default_rng(6), xbyte=200)
        of = _oracle_frame(oracle, sib, sdata, w, h)
        ts = gpu.VitTrack.new(weights_tiny, use_graph=False)
        tn = gpu.VitTrack.new(weights_tiny, use_graph=False)
        # (box, window): the window holds the box's search crop; the second one ends at the frame's right and bottom edge
        cases = [((288, 208, 64, 64), (160, 96, 384, 320)), ((440, 330, 40, 40), (320, 240, w - 320, h - 240))]
        for box, win in cases:
            ref = oracle.VitTrackRef(weights_tiny)
            ref.init(of, box)
            ref.update(of, taps=True)
            want = oracle.bf16_bits_to_f32(ref.last["patches"])
            ts.init(_host(gpu, sib, sdata, w, h), gpu.BBox.new(*box))
            rs = _res(ts.update(_host(gpu, sib, sdata, w, h)))
            assert np.array_equal(_patches(ts), want)
            tn.init(_host(gpu, fmt, ndata, w, h), gpu.BBox.new(*box))
            assert _res(tn.update(_host(gpu, fmt, ndata, w, h))) == rs and np.array_equal(_patches(tn), want), (fmt, w, h, box)
            for aligned in (True, False):
                for kw in ({}, {"window": win}, {"view": win}):
                    f, keep = _device(gpu, fmt, ndata, w, h, aligned=aligned, fill=0x33, **kw)
                    for tier in (0, 2):
                        tn.as_group().set_tuning("crop_tier", tier)
                        tn.init_device(f, gpu.BBox.new(*box))
                        r = _res(tn.update_device(f))
                        assert np.array_equal(_patches(tn), want) and r == rs, (fmt, w, h, box, aligned, kw, tier)
                    tn.as_group().set_tuning("crop_tier", -1)
        # graph replays: a group of two streams, every tier forced, replays what the eager tracker computed
        box = cases[0][0]
        for tier in (-1, 0, 1, 2):
            g = gpu.Group(weights_tiny, n_streams=2, use_graph=True)
            g.set_tuning("crop_tier", tier)
            f, keep = _device(gpu, fmt, ndata, w, h, aligned=True)
            for i in range(2):
                g.init_device(i, f, gpu.BBox.new(*box))
            r = g.update_device([f, f])
            ts.init(_host(gpu, sib, sdata, w, h), gpu.BBox.new(*box))
            rs = _res(ts.update(_host(gpu, sib, sdata, w, h)))
            assert [_res(x) for x in r] == [rs, rs] and g.read_tensor("graph_replays").sum() == 1, (fmt, tier)
            assert g.read_tensor("patches", 1).tobytes() == _patches(ts).tobytes()
            del g


# ---- 2. bytes that must not matter ----------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", NEW)
def test_bytes_that_are_not_sampled_do_not_matter(gpu, weights_tiny, fmt):
    """two device buffers equal in every sampled byte and different everywhere else - the low bytes of P010, the x byte,
    the row padding, the gap between the planes, and, in a pointer-offset view, every pixel outside the stored window -
    give identical patch matrices and results, on the wide and on the per-pixel path, for crops inside the window and
    for one that leaves it (which reads black there, from either buffer)"""
    w, h = 640, 480
    sc = gpu.synth.MovingSquare(w, h, 64, seed=1)
    sdata = _sibling_data(gpu, fmt, sc, 0, w, h)
    other = _sibling_data(gpu, fmt, gpu.synth.MovingSquare(w, h, 64, seed=9), 3, w, h)
    win = (160, 96, 384, 320)
    x0, y0, ww, wh = win
    # frame B: frame A inside the window, another clip's pixels outside it
    inside = np.zeros((h, w), bool)
    inside[y0:y0 + wh, x0:x0 + ww] = True

    def mix(a, b):
        sib = SIBLING[fmt]
        if sib == "rgb8":
            return np.where(inside[:, :, None], a, b)
        if sib == "yuy2":
            m = np.repeat(inside, 2, axis=1).reshape(-1)
            return np.where(m, a, b)
        cw, ch = U.chroma_dims(w, h)
        m = np.concatenate([inside.reshape(-1), np.repeat(inside[::2, ::2], 2, axis=1).reshape(-1)])
        return np.where(m, a, b)

    a_new = U.from_sibling(fmt, sdata, w, h, rng=np.random.default_rng(1), xbyte=0)
    xb = np.random.default_rng(2).integers(0, 256, (h, w), dtype=np.uint8)
    b_new = U.from_sibling(fmt, mix(sdata, other), w, h, rng=np.random.default_rng(3), xbyte=xb)
    if fmt in ("p010", "xrgb", "xbgr"):
        assert not np.array_equal(a_new, U.from_sibling(fmt, sdata, w, h, rng=np.random.default_rng(3), xbyte=xb))
    trk = gpu.VitTrack.new(weights_tiny, use_graph=False)
    for aligned in (True, False):
        fa, ka = _device(gpu, fmt, a_new, w, h, aligned=aligned, fill=0, view=win)
        fb, kb = _device(gpu, fmt, b_new, w, h, aligned=aligned, fill=np.random.default_rng(4), view=win)
        assert not np.array_equal(ka.cpu().numpy(), kb.cpu().numpy())
        for box in ((288, 208, 64, 64), (200, 150, 80, 80), (150, 100, 120, 90)):     # the last crop leaves the window
            for tier in (0, 2):
                trk.as_group().set_tuning("crop_tier", tier)
                out = []
                for f in (fa, fb):
                    trk.init_device(f, gpu.BBox.new(*box))
                    r = _res(trk.update_device(f))
                    out.append((_patches(trk).tobytes(), r))
                assert out[0] == out[1], (fmt, aligned, box, tier)


# ---- 3. closed loop, bit-exact --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", NEW)
def test_closed_loop_cfg2_is_the_siblings_run(gpu, fmt):
    """60 frames of traj_cfg2_300's clip: the new format through VitTrack on host frames and through vt_update_frame on
    device frames gives the sibling format's boxes, score bits and flags (GRAY8: against RGB8 on the grey clip)"""
    fx = _fixture("traj_cfg2_300.npz")
    weights = gpu.weights.ensure_weights(str(fx["config"]))
    sc = _clip(gpu, fx)
    w, h, n = sc.w, sc.h, 60
    runs = ["sib", "host", "dev"]
    trk = {k: gpu.VitTrack(weights) for k in runs}
    out = {k: [] for k in runs}
    rng = np.random.default_rng(11)
    for t in range(n):
        sib, sdata, ndata = _frames_of(gpu, fmt, sc, t, w, h, rng=rng, xbyte=t & 255)
        frames = {"sib": _host(gpu, sib, sdata, w, h), "host": _host(gpu, fmt, ndata, w, h)}
        frames["dev"], keep = _device(gpu, fmt, ndata, w, h)
        for k in runs:
            if t == 0:
                b = gpu.BBox.new(*sc.gt_box(0))
                trk[k].init_device(frames[k], b) if k == "dev" else trk[k].init(frames[k], b)
            r = trk[k].update_device(frames[k]) if k == "dev" else trk[k].update(frames[k])
            out[k].append(_res(r))
    for k in runs[1:]:
        diff = [t for t in range(n) if out[k][t] != out["sib"][t]]
        assert not diff, f"{fmt} {k}: {len(diff)} frames differ from {SIBLING[fmt]}, first {diff[0]}"
    assert len(set(r[0] for r in out["sib"])) > n // 4, "the sibling run's box hardly moves: the comparison shows little"


# ---- 4. engines -----------------------------------------------------------------------------------------------------

GROUPS = [["i420", "p010", "nv12", "gray8", "rgb8"], ["yv12", "nv16", "nv12", "xbgr", "xrgb"]]


def _group_frames(gpu, fmts, scs, t, w, h, sibling, rng):
    """(host frame objects, (format name, packed bytes)) of the streams: the listed formats, or (sibling) each one's sibling"""
    out, raw = [], []
    for i, fmt in enumerate(fmts):
        if fmt in SIBLING:
            sib, sdata, ndata = _frames_of(gpu, fmt, scs[i], t, w, h, rng=rng, xbyte=13)
        else:
            sib = fmt
            sdata = ndata = scs[i].frame_nv12(t) if fmt == "nv12" else scs[i].frame_rgb8(t)
        name, data = (sib, sdata) if sibling else (fmt, ndata)
        out.append(_host(gpu, name, data, w, h))
        raw.append((name, data))
    return out, raw


@pytest.mark.parametrize("fmts", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_group_passes_give_each_stream_its_sibling_formats_results(gpu, weights_tiny, fmts):
    """five streams, one format each: synchronous host passes against device frames of the same formats and against a
    twin engine fed the siblings; pipelined passes with the redo path forced; subset passes; a stream re-initialised
    behind outstanding passes; a candidate pass whose slots share one host frame"""
    w, h, B = 640, 480, 5
    scs = [gpu.synth.MovingSquare(w, h, 64, seed=60 + i) for i in range(B)]     # the clips of the pipelined NV12 test
    g_new, g_dev, g_sib = (gpu.Group(weights_tiny, n_streams=B) for _ in range(3))
    g_pipe = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1)
    g_pipe_sib = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1)
    T = 24          # as the pipelined NV12 test: by then the targets have left their unenlarged windows
    rng = np.random.default_rng(21)
    new_frames = [_group_frames(gpu, fmts, scs, t, w, h, False, rng) for t in range(T)]
    sib_frames = [_group_frames(gpu, fmts, scs, t, w, h, True, rng) for t in range(T)]
    for i in range(B):
        b = gpu.BBox.new(*scs[i].gt_box(0))
        g_new.init_host(i, new_frames[0][0][i], b)
        g_sib.init_host(i, sib_frames[0][0][i], b)
        g_pipe.init_host(i, new_frames[0][0][i], b)
        g_pipe_sib.init_host(i, sib_frames[0][0][i], b)
        f, k = _device(gpu, *new_frames[0][1][i], w, h)
        g_dev.init_device(i, f, b)
    for t in range(1, T):
        rn = g_new.update_host(new_frames[t][0])
        rs = g_sib.update_host(sib_frames[t][0])
        dev = [_device(gpu, *new_frames[t][1][i], w, h) for i in range(B)]
        rd = g_dev.update_device([d[0] for d in dev])
        assert [_res(r) for r in rn] == [_res(r) for r in rs] == [_res(r) for r in rd], t
    # pipelined: the upload of t overlaps the pass of t - 1 (speculative windows, no enlargement: redone passes)
    pipe, pipe_sib = [], []
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
    # a pipelined subset pass and a subset pass on host and device frames
    L = [3, 0, 1]
    g_pipe.enqueue_host([new_frames[T - 1][0][s] for s in L], streams=L)
    g_pipe_sib.enqueue_host([sib_frames[T - 1][0][s] for s in L], streams=L)
    assert [_res(r) for r in g_pipe.wait_next()] == [_res(r) for r in g_pipe_sib.wait_next()]
    # stream 0 (I420 / YV12) joins again behind an outstanding pass of other streams (vt_group_enqueue_init_host)
    L2, b0 = [1, 2], gpu.BBox.new(*scs[0].gt_box(T - 2))
    for g, fr in ((g_pipe, new_frames), (g_pipe_sib, sib_frames)):
        g.enqueue_host([fr[T - 2][0][s] for s in L2], streams=L2)
        g.enqueue_init_host(0, fr[T - 2][0][0], b0)
        g.enqueue_host(fr[T - 1][0])
    for _ in range(2):
        assert [_res(r) for r in g_pipe.wait_next()] == [_res(r) for r in g_pipe_sib.wait_next()]
    assert g_pipe.read_tensor("state", 0).tobytes() == g_pipe_sib.read_tensor("state", 0).tobytes()
    rh = g_new.update_host([new_frames[T - 1][0][s] for s in L], streams=L)
    rs = g_sib.update_host([sib_frames[T - 1][0][s] for s in L], streams=L)
    dev = [_device(gpu, *new_frames[T - 1][1][s], w, h) for s in L]
    rd = g_dev.update_device([d[0] for d in dev], streams=L)
    assert [_res(r) for r in rh] == [_res(r) for r in rs] == [_res(r) for r in rd]
    # a candidate pass: three slots of stream 0 and two of stream 1, each stream's slots on ONE host frame (staged once)
    b0, b1 = g_new.read_state(0)["box"], g_new.read_state(1)["box"]
    cands = [(0, None), (0, [b0[0] + 24, b0[1] - 10, b0[2], b0[3]]), (1, None), (0, [b0[0] - 40, b0[1] + 16, b0[2], b0[3]]),
             (1, [b1[0] + 30, b1[1] + 30, b1[2], b1[3]])]
    fn, fs = new_frames[T - 1][0], sib_frames[T - 1][0]
    rn, wn = g_new.update_host_candidates(cands, [fn[0], fn[0], fn[1], fn[0], fn[1]])
    rs, ws = g_sib.update_host_candidates(cands, [fs[0], fs[0], fs[1], fs[0], fs[1]])
    assert [_res(r) for r in rn] == [_res(r) for r in rs] and wn == ws
    for i in range(B):
        assert g_new.read_tensor("state", i).tobytes() == g_sib.read_tensor("state", i).tobytes(), i


@pytest.mark.parametrize("fmt", ["i420", "p010", "gray8"])
def test_registered_frame_takes_the_zero_copy_route(gpu, weights_tiny, fmt):
    """a clip in registered host memory (vt_host_register) gives, single tracker and zero-copy group, what the same
    frames give from unregistered memory and what the sibling gives; read through the mapping as device frames the
    registered frames give the same results"""
    w, h, n = 640, 480, 5
    sc = gpu.synth.MovingSquare(w, h, 64, seed=23)
    rng = np.random.default_rng(8)
    sibs, news = [], []
    for t in range(n):
        sib, sdata, ndata = _frames_of(gpu, fmt, sc, t, w, h, rng=rng)
        sibs.append(_host(gpu, sib, sdata, w, h))
        news.append(np.asarray(ndata, np.uint8).reshape(-1))
    clip = np.stack(news)
    plain = clip.copy()

    def frames(buf):
        return [_host(gpu, fmt, buf[t].reshape(h, w) if fmt == "gray8" else buf[t], w, h) for t in range(n)]

    def run(fr, zc=None):
        if zc is None:
            trk = gpu.VitTrack.new(weights_tiny)
            trk.init(fr[0], gpu.BBox.new(*sc.gt_box(0)))
            return [_res(trk.update(f)) for f in fr]
        g = gpu.Group(weights_tiny, n_streams=2, host_zero_copy=zc)
        for i in range(2):
            g.init_host(i, fr[0], gpu.BBox.new(*sc.gt_box(0)))
        return [[_res(r) for r in g.update_host([f, f])] for f in fr]

    want = (run(sibs), run(sibs, 1))
    hm = gpu.HostMapping(clip)
    try:
        got = (run(frames(clip)), run(frames(clip), 1))
        trk = gpu.VitTrack.new(weights_tiny)
        fb = clip.shape[1]
        helper = {"i420": lambda p: gpu.frame_i420(p, p + w * h, w, h), "p010": lambda p: gpu.frame_p010(p, p + 2 * w * h, w, h),
                  "gray8": lambda p: gpu.frame_gray8(p, w, h)}[fmt]
        trk.init_device(helper(hm.d_ptr), gpu.BBox.new(*sc.gt_box(0)))
        via_map = [_res(trk.update_device(helper(hm.d_ptr + t * fb))) for t in range(n)]
    finally:
        hm.close()
    unreg = run(frames(plain))
    assert got == want and unreg == want[0] and via_map == want[0]


# ---- 5. template refresh and target chips -----------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["bf16", "rgb8"])
def test_refresh_and_chips_give_the_siblings_rows_and_bytes(gpu, weights_tiny, kind):
    """streams on I420, P010 and GRAY8 with a template-refresh policy and chips enabled: after every pass the template
    rows and the chip bytes are those of the sibling formats in a twin engine (device frames, graph replays)"""
    w, h = 640, 480
    fmts = ["i420", "p010", "gray8"]
    scs = [gpu.synth.MovingSquare(w, h, 64, seed=40 + i) for i in range(3)]
    ck = gpu.CHIP_NORM_BF16 if kind == "bf16" else gpu.CHIP_RGB8
    g_new, g_sib = gpu.Group(weights_tiny, n_streams=3), gpu.Group(weights_tiny, n_streams=3)
    for g in (g_new, g_sib):
        g.set_template_refresh(2, 0.0)
        g.enable_chips(64, ck)
        g.set_chips(2.0, 1, 0)
    rng = np.random.default_rng(2)
    for t in range(7):
        fn, fs, keep = [], [], []
        for i, fmt in enumerate(fmts):
            sib, sdata, ndata = _frames_of(gpu, fmt, scs[i], t, w, h, rng=rng)
            for lst, name, data in ((fn, fmt, ndata), (fs, sib, sdata)):
                f, k = _device(gpu, name, data, w, h)
                lst.append(f)
                keep.append(k)
        if t == 0:
            for i in range(3):
                g_new.init_device(i, fn[i], gpu.BBox.new(*scs[i].gt_box(0)))
                g_sib.init_device(i, fs[i], gpu.BBox.new(*scs[i].gt_box(0)))
            continue
        rn, rs = g_new.update_device(fn), g_sib.update_device(fs)
        assert [_res(r) for r in rn] == [_res(r) for r in rs], t
        cn, infn = g_new.read_chips()
        cs, infs = g_sib.read_chips()
        assert cn.tobytes() == cs.tobytes() and infn == infs, t
        for i in range(3):
            assert g_new.read_tensor("template", i).tobytes() == g_sib.read_tensor("template", i).tobytes(), (t, i)
    assert g_new.template_refresh_stats(0)["generation"] > 0 and cn.any()


# ---- 6. graphs: captured at init, never inside an update ------------------------------------------------------------

def test_graphs_are_captured_at_the_first_init_never_in_an_update(gpu, weights_tiny):
    """the first init on a vt_pixfmt2 format captures one graph set (the tier count), later inits and updates none, and
    the passes replay; an engine that only ever sees NV12 captures what it did at creation"""
    w, h = 640, 480
    sc = gpu.synth.MovingSquare(w, h, 64, seed=2)
    g = gpu.Group(weights_tiny, n_streams=2)
    tiers = g.graph_captures()
    assert tiers == 3
    frames = {}
    for fmt in ("nv12", "i420", "gray8"):
        data = sc.frame_nv12(0) if fmt == "nv12" else _frames_of(gpu, fmt, sc, 0, w, h)[2]
        frames[fmt] = _device(gpu, fmt, data, w, h)
    box = gpu.BBox.new(*sc.gt_box(0))
    g.init_device(0, frames["nv12"][0], box)
    g.init_device(1, frames["nv12"][0], box)
    g.update_device([frames["nv12"][0]] * 2)
    assert g.graph_captures() == tiers, "an NV12-only engine captured more than its creation did"
    g.init_device(1, frames["i420"][0], box)
    assert g.graph_captures() == 2 * tiers
    g.init_device(0, frames["gray8"][0], box)
    assert g.graph_captures() == 2 * tiers
    before = int(g.read_tensor("graph_replays").sum())
    for s in (40, 64, 100, 160, 230):           # through the tier boundaries of the tiny model's crop
        for i in range(2):
            g.set_state_box(i, [320 - s / 2, 240 - s / 2, s, s])
        g.update_device([frames["gray8"][0], frames["i420"][0]])
        g.update_device([frames["nv12"][0], frames["i420"][0]])
    assert g.graph_captures() == 2 * tiers, "a pass captured a graph on the hot path"
    assert int(g.read_tensor("graph_replays").sum()) == before + 10


def test_a_snapshot_of_an_i420_stream_continues_in_another_engine(gpu, weights_tiny):
    """a stream initialised on I420 is exported, imported into an engine that has only seen NV12, and fed I420 frames
    there: the results of the twin that never moved; the import is the only call that captures"""
    w, h = 640, 480
    sc = gpu.synth.MovingSquare(w, h, 64, seed=5)

    def frames(t):
        sib, sdata, ndata = _frames_of(gpu, "i420", sc, t, w, h)
        return _device(gpu, "nv12", sdata, w, h), _device(gpu, "i420", ndata, w, h)

    a, b, twin = (gpu.Group(weights_tiny, n_streams=2) for _ in range(3))
    nv, yu = frames(0)
    box = gpu.BBox.new(*sc.gt_box(0))
    for i in range(2):
        a.init_device(i, yu[0], box)
        twin.init_device(i, yu[0], box)
        b.init_device(i, nv[0], box)
    for t in range(1, 4):
        nv, yu = frames(t)
        ra, rt, rb = a.update_device([yu[0]] * 2), twin.update_device([yu[0]] * 2), b.update_device([nv[0]] * 2)
        assert [_res(r) for r in ra] == [_res(r) for r in rt] == [_res(r) for r in rb]
    blob = a.export_stream(1)
    assert gpu.snapshot_info(blob)["flags"] == 1
    caps = b.graph_captures()
    b.import_stream(1, blob)
    caps_after = b.graph_captures()
    assert caps_after >= caps
    for t in range(4, 8):
        nv, yu = frames(t)
        rb, rt = b.update_device([nv[0], yu[0]]), twin.update_device([yu[0]] * 2)
        assert [_res(r) for r in rb] == [_res(r) for r in rt], t
    assert b.graph_captures() == caps_after, "an update captured a graph"
    assert b.read_tensor("state", 1).tobytes() == twin.read_tensor("state", 1).tobytes()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------

def test_bad_frames_are_refused_and_change_nothing(gpu, weights_tiny):
    import torch
    L_ = gpu.lib()
    w, h = 640, 480
    cw, ch = U.chroma_dims(w, h)
    sc = gpu.synth.MovingSquare(w, h, 64, seed=3)
    buf = sc.frame_nv12(0)
    d = torch.from_numpy(np.concatenate([buf, np.zeros(4 * w * h, np.uint8)])).cuda()
    p = d.data_ptr()
    q = p + w * h
    good = gpu.frame_nv12(p, q, w, h)
    trk, twin = gpu.VitTrack.new(weights_tiny), gpu.VitTrack.new(weights_tiny)
    for t_ in (trk, twin):
        t_.init_device(good, gpu.BBox.new(*sc.gt_box(0)))
        t_.update_device(good)
    g = trk.as_group()
    before = g.read_tensor("state").tobytes()
    F, P = gpu.CFrame, gpu
    bad = [F(p, None, w, h, w, cw, P.PIX_I420, 0, 0, 0, 0, 0),                 # no chroma plane
           F(p, None, w, h, w, cw, P.PIX_YV12, 0, 0, 0, 0, 0),
           F(p, None, w, h, 2 * w, 2 * w, P.PIX_P010, 0, 0, 0, 0, 0),
           F(p, None, w, h, w, w, P.PIX_NV16, 0, 0, 0, 0, 0),
           F(p, q, w, h, w - 1, cw, P.PIX_I420, 0, 0, 0, 0, 0),                # small strides
           F(p, q, w, h, w, cw - 1, P.PIX_I420, 0, 0, 0, 0, 0),
           F(p, q, w, h, w, cw - 1, P.PIX_YV12, 0, 0, 0, 0, 0),
           F(p, q, w, h, 2 * w - 1, 2 * w, P.PIX_P010, 0, 0, 0, 0, 0),
           F(p, q, w, h, 2 * w, 2 * w - 1, P.PIX_P010, 0, 0, 0, 0, 0),
           F(p, q, w, h, w, w, P.PIX_P010, 0, 0, 0, 0, 0),                     # NV12's strides: samples are two bytes
           F(p, q, w, h, w - 1, w, P.PIX_NV16, 0, 0, 0, 0, 0),
           F(p, q, w, h, w, w - 1, P.PIX_NV16, 0, 0, 0, 0, 0),
           F(p, None, w, h, w - 1, 0, P.PIX_GRAY8, 0, 0, 0, 0, 0),
           F(p, None, w, h, 4 * w - 1, 0, P.PIX_XRGB, 0, 0, 0, 0, 0),
           F(p, None, w, h, 4 * w - 1, 0, P.PIX_XBGR, 0, 0, 0, 0, 0),
           F(p, q, w - 1, h, w, w, P.PIX_NV16, 0, 0, 0, 0, 0),                 # odd NV16 width
           F(p, q, w, h, w, cw, P.PIX_I420, 3, 2, 1, 64, 64),                  # odd origins
           F(p, q, w, h, w, cw, P.PIX_YV12, 2, 3, 1, 64, 64),
           F(p, q, w, h, 2 * w, 2 * w, P.PIX_P010, 3, 2, 1, 64, 64),
           F(p, q, w, h, 2 * w, 2 * w, P.PIX_P010, 2, 3, 1, 64, 64),
           F(p, q, w, h, w, w, P.PIX_NV16, 3, 2, 1, 64, 64),
           F(p, q, w, h, w, cw, P.PIX_I420, 2, 2, 1, 63, 64),                  # odd extents that do not end at the edge
           F(p, q, w, h, w, cw, P.PIX_I420, 2, 2, 1, 64, 63),
           F(p, q, w, h, 2 * w, 2 * w, P.PIX_P010, 2, 2, 1, 64, 63),
           F(p, q, w, h, w, w, P.PIX_NV16, 2, 2, 1, 63, 64)]
    named = len(bad)        # every rule of a format above names it in the error text
    bad += [F(p, None, w, h, w, 0, P.PIX_GRAY8, 2, 2, 1, 0, 0),                 # a window without an extent
           F(p, None, w, h, 4 * w, 0, P.PIX_XRGB, 0, 0, 1, w + 1, h)]          # a window larger than the frame
    bad += [F(p, q, w, h, 4 * w, 4 * w, v, 0, 0, 0, 0, 0) for v in list(range(8, 16)) + [23, 24, 255, -1]]
    r = gpu.CResult()
    for i, f in enumerate(bad):
        tag = (f.format, f.stride0, f.stride1, f.origin_x, f.origin_y, f.window_w, f.window_h, f.width)
        assert L_.vt_update_frame(trk._h, ctypes.byref(f), 1, ctypes.byref(r)) == INVALID, tag
        text = L_.vt_last_error().decode()
        if i < named:
            assert U.NEW[f.format - 16] in text, (tag, text)      # the text names the format
        assert L_.vt_init_frame(trk._h, ctypes.byref(f), 1, gpu.BBox.new(10, 10, 40, 40)._c()) == INVALID, tag
        if f.origin_x == 0 and f.windowed == 0:      # host frames: no origin fields
            host = np.zeros(8 * w * h, np.uint8)
            hf = gpu.CFrame(*[getattr(f, n) for n, _ in gpu.CFrame._fields_])
            hf.plane0 = host.ctypes.data
            hf.plane1 = host.ctypes.data + 2 * w * h if f.plane1 else None
            assert L_.vt_update_frame(trk._h, ctypes.byref(hf), 0, ctypes.byref(r)) == INVALID, tag
            assert L_.vt_init_frame(trk._h, ctypes.byref(hf), 0, gpu.BBox.new(10, 10, 40, 40)._c()) == INVALID, tag
    assert g.read_tensor("state").tobytes() == before
    # a following valid update gives the result it would have given
    assert _res(trk.update_device(good)) == _res(twin.update_device(good))
    # group entry points refuse the same frames
    grp = gpu.Group(weights_tiny, n_streams=1)
    grp.init_device(0, good, gpu.BBox.new(*sc.gt_box(0)))
    st = grp.read_tensor("state").tobytes()
    for f in bad:
        with pytest.raises(gpu.VtError) as ei:
            grp.init_device(0, f, gpu.BBox.new(10, 10, 40, 40))
        assert ei.value.code == INVALID
        with pytest.raises(gpu.VtError) as ei:
            grp.update_device([f])
        assert ei.value.code == INVALID
    assert grp.read_tensor("state").tobytes() == st
