"""Result overlay, operator level (vt_op_result_overlay: the launch of csrc/k_result_overlay.hip alone), on the MI355X.

Every comparison is np.array_equal on EVERY byte of the frame - chroma, pad bytes and row padding included - against
result_overlay_util.expected, which draws the specification's command list with the existing oracle.vit_ref.draw / draw_rgb.
Frames are 96x64 and 160x120; a launch carries many slots, each with a frame of its own unless the case is about sharing."""
import numpy as np
import pytest

import result_overlay_util as ro

pytestmark = pytest.mark.gpu

SIZES = ((96, 64), (160, 120))
NEXT = float(np.nextafter(np.float32(0.25), np.float32(1)))


def boxes(W, H):
    """(name, bbox): flush with every edge and corner, thinner than twice the thickness, 1x1, crosshair on a border, a label
    past the right edge, boxes partly and wholly outside (the luma rectangle's x + w < 0 wrap included), one larger than the frame"""
    return [("interior", (30, 24, 30, 20)), ("top-left", (0, 0, 30, 20)), ("top-right", (W - 30, 0, 30, 20)),
            ("bottom-left", (0, H - 20, 30, 20)), ("bottom-right", (W - 30, H - 20, 30, 20)), ("left edge", (0, 20, 12, 30)),
            ("top edge", (40, 0, 30, 12)), ("thin", (40, 30, 4, 4)), ("thin row", (20, 30, 40, 2)), ("1x1", (50, 40, 1, 1)),
            ("centre on x = 0", (-10, 20, 20, 20)), ("centre on the last column", (W - 11, 20, 20, 20)),
            ("centre on the last row", (30, H - 11, 20, 20)), ("label past the right edge", (W - 40, 30, 30, 20)),
            ("x + w < 0", (-50, -40, 20, 10)), ("beyond the corner", (W + 5, H + 5, 10, 10)), ("half outside", (-15, -9, 40, 30)),
            ("larger than the frame", (-10, -10, W + 20, H + 20)), ("ends at the frame", (W - 20, H - 16, 20, 16)),
            ("ends one before", (W - 21, H - 17, 20, 16))]


class Dev:
    """a packed frame of `fmt` in device memory (optionally with padded rows) and its vt_frame"""

    def __init__(self, gpu, fmt, buf, w, h, pad=0, canary=0xC3):
        import torch
        self.fmt, self.w, self.h, self.pad = fmt, w, h, pad
        self.planes = self._planes(fmt, w, h)       # (row bytes, rows) of every plane, in buffer order
        host = np.asarray(buf, np.uint8).reshape(-1)
        rows = []
        off = 0
        for rb, nr in self.planes:
            p = np.full((nr, rb + pad), canary, np.uint8)
            p[:, :rb] = host[off:off + rb * nr].reshape(nr, rb)
            rows.append(p.reshape(-1))
            off += rb * nr
        assert off == host.size
        self.host = np.concatenate(rows)
        self.t = torch.from_numpy(self.host.copy()).cuda()
        base = self.t.data_ptr()
        s0 = self.planes[0][0] + pad
        p1 = base + s0 * self.planes[0][1] if len(self.planes) > 1 else None
        s1 = self.planes[1][0] + pad if len(self.planes) > 1 else 0
        self.frame = gpu.CFrame(base, p1, w, h, s0, s1, getattr(gpu, "PIX_" + fmt.upper()), 0, 0, 0, 0, 0)

    @staticmethod
    def _planes(fmt, w, h):
        cw, ch = (w + 1) // 2, (h + 1) // 2
        if fmt in ("nv12", "nv21"):
            return [(w, h), (2 * cw, ch)]
        if fmt in ("i420", "yv12"):
            return [(w, h), (cw, ch), (cw, ch)]
        if fmt == "p010":
            return [(2 * w, h), (4 * cw, ch)]
        if fmt == "nv16":
            return [(w, h), (w, h)]
        return [(ro.frame_bytes(fmt, w, h) // h, h)]

    def padded(self, packed):
        """a packed buffer laid out like the device copy (row padding = the canary the device copy started with)"""
        out = self.host.copy()
        src, off, o = np.asarray(packed, np.uint8).reshape(-1), 0, 0
        for rb, nr in self.planes:
            out[o:o + (rb + self.pad) * nr].reshape(nr, rb + self.pad)[:, :rb] = src[off:off + rb * nr].reshape(nr, rb)
            off += rb * nr
            o += (rb + self.pad) * nr
        return out

    def read(self):
        return self.t.cpu().numpy()


def _results(gpu, slots):
    r = np.zeros(len(slots), gpu.RESULT_DTYPE)
    for i, (success, score, bbox) in enumerate(slots):
        r[i] = (success, score, bbox)
    return r


def _check_stats(st, slots, pol, drawable=True):
    want = ro.stats_after(slots, drawable=drawable, **pol)
    for i, (drawn, nd, ng, nu, last) in enumerate(want):
        got = st[i]
        assert (got["drawn"], got["n_drawn"], got["n_gated"], got["n_unsupported"]) == (drawn, nd, ng, nu), (i, slots[i], got)
        assert got["last_n"] == (last if last is not None else 0), (i, slots[i], got)
        assert not got["reserved"].any()


def _content(fmt, w, h, seed):
    return np.random.default_rng(seed).integers(0, 200, ro.frame_bytes(fmt, w, h), dtype=np.uint8)


POLICIES = [dict(), dict(flags=1), dict(flags=2), dict(flags=4), dict(flags=3, thickness=1, size=1),
            dict(thickness=16, size=64, scale=4, luma=128, rgb=0x1080F0), dict(flags=5, scale=1, thickness=2, luma=0, rgb=0)]


@pytest.mark.parametrize("fmt", ["nv12", "rgb8"])
@pytest.mark.parametrize("W,H", SIZES)
def test_boxes_at_every_edge(gpu, oracle, fmt, W, H):
    """one slot per box case, each on a frame of its own, under every policy of POLICIES"""
    cases = boxes(W, H)
    slots = [(1, 0.5 + 0.01 * i, b) for i, (_, b) in enumerate(cases)]
    for k, pol in enumerate(POLICIES):
        bufs = [_content(fmt, W, H, 100 + i) for i in range(len(cases))]
        devs = [Dev(gpu, fmt, b, W, H) for b in bufs]
        st = gpu.op_result_overlay([d.frame for d in devs], _results(gpu, slots), **pol)
        for i, (name, _) in enumerate(cases):
            want = ro.expected(oracle, fmt, bufs[i], W, H, [slots[i]], **pol)
            assert np.array_equal(devs[i].read(), want), f"{fmt} {W}x{H}, policy {k}, box '{name}' {cases[i][1]}"
        _check_stats(st, slots, dict(ro.DEFAULTS, **pol))
    # something was drawn at all, and the wrap case lit the last column (the reference's usize quirk)
    if fmt == "nv12":
        i = [n for n, _ in cases].index("x + w < 0")
        assert (devs[i].read() != bufs[i]).any()


@pytest.mark.parametrize("fmt", ["nv12", "bgrx"])
def test_gate_scores_and_success(gpu, oracle, fmt):
    """scores on both sides of and exactly at the gate, a NaN, success = 0 - at the default 25 and at 0, 60 and 100"""
    W, H = SIZES[0]
    box = (20, 24, 30, 20)
    slots = [(1, 0.25, box), (1, NEXT, box), (1, 0.2, box), (1, 0.9, box), (1, float("nan"), box), (0, 0.9, box), (1, 0.6, box),
             (1, 1.0, box), (1, 0.0, box), (1, -0.5, box), (1, float("inf"), box), (1, 0.125, box), (1, 0.375, box), (1, 0.995, box)]
    for pct in (25, 0, 60, 100):
        bufs = [_content(fmt, W, H, 7 + i) for i in range(len(slots))]
        devs = [Dev(gpu, fmt, b, W, H) for b in bufs]
        st = gpu.op_result_overlay([d.frame for d in devs], _results(gpu, slots), min_score_pct=pct)
        n_drawn = 0
        for i, s in enumerate(slots):
            want = ro.expected(oracle, fmt, bufs[i], W, H, [s], min_score_pct=pct)
            n_drawn += int((want != bufs[i]).any())
            assert np.array_equal(devs[i].read(), want), f"{fmt}, gate {pct}, slot {i} {s[:2]}"
        _check_stats(st, slots, dict(ro.DEFAULTS, min_score_pct=pct))
        assert n_drawn == {25: 7, 0: 10, 60: 4, 100: 1}[pct], (pct, n_drawn)
    assert [int(v) for v in st["last_n"][-3:]] == [0, 0, 0]     # gate 100: none of the three drew
    st = gpu.op_result_overlay([d.frame for d in devs], _results(gpu, slots))
    assert [int(v) for v in st["last_n"][-3:]] == [0, 38, 100] and st["drawn"][-3:].tolist() == [0, 1, 1]   # 0.125 is gated at 25


@pytest.mark.parametrize("fmt", ro.DRAWABLE + ("p010",))
def test_every_format(gpu, oracle, fmt):
    """three slots, three frames; P010 is left untouched and counted"""
    W, H = SIZES[0]
    slots = [(1, 0.8, (30, 24, 30, 20)), (1, 0.31, (W - 30, H - 20, 30, 20)), (1, 0.66, (-15, -9, 40, 30))]
    pol = dict(luma=231, rgb=0xF02010)
    bufs = [_content(fmt, W, H, 40 + i) for i in range(3)]
    devs = [Dev(gpu, fmt, b, W, H) for b in bufs]
    st = gpu.op_result_overlay([d.frame for d in devs], _results(gpu, slots), **pol)
    for i in range(3):
        want = ro.expected(oracle, fmt, bufs[i], W, H, [slots[i]], **pol)
        assert np.array_equal(devs[i].read(), want), f"{fmt}, slot {i}"
        assert (want != bufs[i]).any() == (fmt != "p010")
    _check_stats(st, slots, dict(ro.DEFAULTS, **pol), drawable=fmt != "p010")


@pytest.mark.parametrize("fmt,pad", [("nv12", 13), ("rgb8", 7), ("rgbx", 8), ("uyvy", 6), ("i420", 5), ("gray8", 3)])
def test_padded_strides(gpu, oracle, fmt, pad):
    W, H = SIZES[1]
    slots = [(1, 0.8, (W - 40, 30, 36, 50)), (1, 0.5, (-4, H - 30, 50, 40))]
    bufs = [_content(fmt, W, H, 60 + i) for i in range(2)]
    devs = [Dev(gpu, fmt, b, W, H, pad=pad) for b in bufs]
    gpu.op_result_overlay([d.frame for d in devs], _results(gpu, slots))
    for i in range(2):
        want = devs[i].padded(ro.expected(oracle, fmt, bufs[i], W, H, [slots[i]]))
        assert np.array_equal(devs[i].read(), want), f"{fmt} stride + {pad}, slot {i}: a frame byte or the row padding differs"


@pytest.mark.parametrize("fmt", ["nv12", "rgb8", "yuy2", "xbgr"])
@pytest.mark.parametrize("packed", [True, False])
def test_window_cuts_through_the_rectangle(gpu, oracle, fmt, packed):
    """a stored window 64x48 at (32, 20) of a 160x120 frame. packed: the planes hold the window only (windowed = 1), inside a
    buffer with a canary margin on both sides; else plane0 points into a whole frame (origin set, full strides) and every byte
    of the frame outside the window is the guard. The rectangle, the crosshair and the label all cross the window's border."""
    import torch
    W, H = SIZES[1]
    ox, oy, ww, wh = 32, 20, 64, 48
    slots = [(1, 0.8, (20, 10, 60, 40)), (1, 0.7, (80, 50, 40, 40))]
    full = _content(fmt, W, H, 77)
    want_full = ro.expected(oracle, fmt, full, W, H, slots)
    bpp = {"nv12": 1, "rgb8": 3, "yuy2": 2, "xbgr": 4}[fmt]
    MARGIN = 4096

    def crop(buf):      # the window's bytes, packed, plane after plane
        y = buf[:W * H * bpp].reshape(H, W * bpp)[oy:oy + wh, ox * bpp:(ox + ww) * bpp].reshape(-1)
        if fmt != "nv12":
            return y
        uv = buf[W * H:].reshape(H // 2, W)[oy // 2:(oy + wh) // 2, ox:ox + ww].reshape(-1)
        return np.concatenate([y, uv])

    if packed:
        host = np.concatenate([np.full(MARGIN, 0xC3, np.uint8), crop(full), np.full(MARGIN, 0xC3, np.uint8)])
        t = torch.from_numpy(host.copy()).cuda()
        p0 = t.data_ptr() + MARGIN
        fr = gpu.CFrame(p0, p0 + ww * wh if fmt == "nv12" else None, W, H, ww * bpp, ww if fmt == "nv12" else 0,
                        getattr(gpu, "PIX_" + fmt.upper()), ox, oy, 1, ww, wh)
        want = np.concatenate([host[:MARGIN], crop(want_full), host[-MARGIN:]])
    else:
        t = torch.from_numpy(full.copy()).cuda()
        p0 = t.data_ptr() + oy * W * bpp + ox * bpp
        p1 = t.data_ptr() + W * H + (oy // 2) * W + ox if fmt == "nv12" else None
        fr = gpu.CFrame(p0, p1, W, H, W * bpp, W if fmt == "nv12" else 0, getattr(gpu, "PIX_" + fmt.upper()), ox, oy, 0, ww, wh)
        want = full.copy()
        m = np.zeros(W * H * bpp, bool).reshape(H, W * bpp)
        m[oy:oy + wh, ox * bpp:(ox + ww) * bpp] = True
        want[:W * H * bpp][m.reshape(-1)] = want_full[:W * H * bpp][m.reshape(-1)]
    st = gpu.op_result_overlay([fr, fr], _results(gpu, slots))
    got = t.cpu().numpy()
    assert np.array_equal(got, want), f"{fmt}, packed {packed}: the window or its guard differs"
    assert (crop(want_full) != crop(full)).any() and (want_full != full).sum() > (crop(want_full) != crop(full)).sum()
    assert st["drawn"].tolist() == [1, 1]


@pytest.mark.parametrize("fmt", ["rgb8", "nv12", "bgrx"])
def test_slots_that_share_a_frame(gpu, oracle, fmt):
    """two and three slots on ONE frame, overlapping shapes, different results: the lists concatenate in slot order (on RGB
    the label's grey and the shapes' colour tell who is on top). A slot that is gated draws nothing and hides nothing; a slot
    on another frame between them is not taken for a sharer."""
    W, H = SIZES[1]
    pol = dict(luma=200, rgb=0x20E040)
    a = (1, 0.9, (30, 40, 70, 40))         # its label lies across b's rectangle, its rectangle across c's label
    b = (1, 0.6, (20, 8, 60, 30))
    c = (1, 0.45, (40, 60, 50, 40))
    gated = (1, 0.1, (25, 20, 80, 60))
    for order in ([a, b], [b, a], [a, b, c], [c, a, b], [a, gated, b], [b, c, a]):
        buf = _content(fmt, W, H, 5)
        other = _content(fmt, W, H, 6)
        d, o = Dev(gpu, fmt, buf, W, H), Dev(gpu, fmt, other, W, H)
        frames = [d.frame] * len(order)
        slots = list(order)
        frames.insert(1, o.frame)
        slots.insert(1, (1, 0.77, (35, 30, 60, 50)))
        st = gpu.op_result_overlay(frames, _results(gpu, slots), **pol)
        assert np.array_equal(d.read(), ro.expected(oracle, fmt, buf, W, H, order, **pol)), f"{fmt}: {len(order)} slots {[s[1] for s in order]}"
        assert np.array_equal(o.read(), ro.expected(oracle, fmt, other, W, H, [slots[1]], **pol))
        _check_stats(st, slots, dict(ro.DEFAULTS, **pol))
    if fmt == "rgb8":     # the order matters in these pictures: the test shows something
        assert not np.array_equal(ro.expected(oracle, fmt, buf, W, H, [a, b], **pol), ro.expected(oracle, fmt, buf, W, H, [b, a], **pol))


def test_many_slots_on_one_frame(gpu, oracle):
    """forty slots on one frame: more sharers than one LDS chunk of the kernel holds"""
    W, H = SIZES[1]
    rng = np.random.default_rng(9)
    slots = [(1, float(rng.uniform(0.3, 1.0)), (int(rng.integers(-10, W - 20)), int(rng.integers(-10, H - 20)), int(rng.integers(8, 60)),
                                               int(rng.integers(8, 50)))) for _ in range(40)]
    buf = _content("rgb8", W, H, 12)
    d = Dev(gpu, "rgb8", buf, W, H)
    pol = dict(luma=90, rgb=0xE01030, thickness=2, scale=1)
    gpu.op_result_overlay([d.frame] * 40, _results(gpu, slots), **pol)
    assert np.array_equal(d.read(), ro.expected(oracle, "rgb8", buf, W, H, slots, **pol))


def test_candidate_losers_and_stream_map(gpu, oracle):
    """slots 0, 1 work for stream 3 (slot 1 wins), slots 2, 3 for stream 0 (slot 2 wins), slot 4 alone for stream 1: losers
    draw nothing, write no record, and do not hide the winner's pixels; the records are by STREAM"""
    W, H = SIZES[0]
    fmt = "nv12"
    bufs = [_content(fmt, W, H, 20 + i) for i in range(3)]
    devs = [Dev(gpu, fmt, b, W, H) for b in bufs]
    frames = [devs[0].frame, devs[0].frame, devs[1].frame, devs[1].frame, devs[2].frame]
    slots = [(1, 0.95, (10, 10, 40, 30)), (1, 0.7, (30, 20, 40, 30)), (1, 0.8, (5, 5, 30, 30)), (1, 0.9, (40, 20, 30, 30)),
             (1, 0.1, (20, 20, 30, 30))]
    smap, winner = [3, 3, 0, 0, 1], [1, 1, 2, 2, 4]
    start = np.zeros(4, gpu.OVERLAY_STATS_DTYPE)
    start["n_drawn"], start["n_gated"], start["drawn"], start["last_n"] = 10, 20, 1, 55
    st = gpu.op_result_overlay(frames, _results(gpu, slots), slot_stream=smap, winner=winner, stats=start)
    assert np.array_equal(devs[0].read(), ro.expected(oracle, fmt, bufs[0], W, H, [slots[1]]))
    assert np.array_equal(devs[1].read(), ro.expected(oracle, fmt, bufs[1], W, H, [slots[2]]))
    assert np.array_equal(devs[2].read(), bufs[2])
    assert [tuple(int(v) for v in (s["drawn"], s["n_drawn"], s["n_gated"], s["last_n"])) for s in st] == \
        [(1, 11, 20, 80), (0, 10, 21, 55), (1, 10, 20, 55), (1, 11, 20, 70)]       # stream 2 was not in the pass: untouched


def test_host_pass_and_flags_zero_draw_nothing(gpu):
    W, H = SIZES[0]
    slots = [(1, 0.9, (10, 10, 40, 30)), (1, 0.1, (10, 10, 40, 30))]
    for fmt in ("nv12", "rgb8"):
        for kw in (dict(device_frames=False), dict(flags=0)):
            bufs = [_content(fmt, W, H, i) for i in range(2)]
            devs = [Dev(gpu, fmt, b, W, H) for b in bufs]
            start = np.zeros(2, gpu.OVERLAY_STATS_DTYPE)
            start["drawn"], start["n_drawn"] = 1, 4
            st = gpu.op_result_overlay([d.frame for d in devs], _results(gpu, slots), stats=start, **kw)
            for d, b in zip(devs, bufs):
                assert np.array_equal(d.read(), b), (fmt, kw)
            assert st["drawn"].tolist() == [0, 0] and st["n_drawn"].tolist() == [4, 4] and not st["n_gated"].any(), (fmt, kw)


def test_bad_operands_are_refused(gpu):
    W, H = SIZES[0]
    d = Dev(gpu, "nv12", _content("nv12", W, H, 1), W, H)
    res = _results(gpu, [(1, 0.9, (10, 10, 40, 30))])
    for bad in (dict(flags=8), dict(flags=-1), dict(thickness=0), dict(thickness=17), dict(size=0), dict(size=65), dict(scale=0),
                dict(scale=5), dict(luma=256), dict(luma=-1), dict(rgb=0x1000000), dict(min_score_pct=101), dict(min_score_pct=-1),
                dict(slot_stream=[1]), dict(winner=[1])):
        with pytest.raises(gpu.VtError):
            gpu.op_result_overlay([d.frame], res, **bad)
    f = gpu.CFrame.from_buffer_copy(bytes(d.frame))
    f.stride0 = W - 1
    with pytest.raises(gpu.VtError):
        gpu.op_result_overlay([f], res)
    assert np.array_equal(d.read(), d.host)
