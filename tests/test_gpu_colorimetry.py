"""BT.709, BT.2020 and full-range YUV frames (the colour bits of vt_frame.format) on the MI355X.

A coloured YUV frame MEANS an RGB8 frame: colorimetry_util.rgb8_sibling converts it pixel by pixel with the header's integer
rule. The oracle and an engine fed that RGB8 sibling know nothing of colour, so every check is exact:
  1. the patch matrix of every YUV format under every new code equals the oracle's on the sibling and the sibling's HIP run:
     host frames, aligned device frames (the grouped paths), unaligned ones (the per-pixel path), every crop tier;
  2. packed windows, pointer-offset views, odd sizes, graph replays;
  3. a closed loop on the synthetic clip is the sibling's run, and differs from the same bytes read as plain NV12;
  4. one pass with slots of different codes: synchronous, pipelined with redone passes, a subset, a candidate pass;
  5. every frame reader of an engine with every feature enabled, and the operator hooks that take frames;
  6. graphs: one more set at the first coloured init, nothing inside an update;
  7. refusals change nothing.
Sections 1, 2 and 4 use frames whose every Y, U and V byte is uniform in 0..255: every code then clamps on both sides."""
import ctypes
import importlib

import numpy as np
import pytest

import colorimetry_util as C
from test_gpu_planar_formats import _device, _patches, _res
from test_gpu_pixel_formats import BOXES

pytestmark = pytest.mark.gpu

W, H = 640, 480
INVALID = -1
_cache = {}


def _dev(gpu, fmt, data, w, h, code=0, **kw):
    """(CFrame of device memory with the code's format word, keep-alive tensor)"""
    f, keep = _device(gpu, fmt, data, w, h, **kw)
    if code:
        f.format = C.word(gpu, fmt, code)
    return f, keep


def _random(w, h, seed=17):
    key = ("nv12", w, h, seed)
    if key not in _cache:
        _cache[key] = C.random_nv12(w, h, seed)
    return _cache[key]


def _sibling(w, h, code, seed=17):
    """the RGB8 sibling of the random frame under a code: the same image for every format (the 4:2:2 formats are built with
    the 4:2:0 frame's chroma row on both rows of a pair)"""
    key = ("rgb", w, h, code, seed)
    if key not in _cache:
        _cache[key] = C.sibling_of("nv12", _random(w, h, seed), w, h, code)
    return _cache[key]


def _oracle_patches(oracle, weights, w, h, code, box, seed=17):
    """the oracle's patch matrix on the RGB8 sibling, once per (size, code, box): shared by every format"""
    key = ("oracle", w, h, code, box, seed)
    if key not in _cache:
        ref = oracle.VitTrackRef(weights)
        of = oracle.Frame.rgb8(_sibling(w, h, code, seed))
        ref.init(of, box)
        ref.update(of, taps=True)
        _cache[key] = oracle.bf16_bits_to_f32(ref.last["patches"])
    return _cache[key]


def test_the_random_frame_clamps_on_both_sides_under_every_code():
    y, u, v = C.yuv_planes("420", _random(W, H), W, H)
    for code in C.CODES:
        for s in C.unclamped(y, u, v, code):
            assert s.min() < 0 and s.max() > 0xffff, code
    for fmt in C.YUV_FORMATS:        # every format's sibling is the one image
        assert np.array_equal(C.sibling_of(fmt, _random(W, H), W, H, 3), _sibling(W, H, 3)), fmt


# ---- 1. patch matrix, exact ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", C.YUV_FORMATS)
def test_patch_matrix_is_the_oracles_on_the_rgb8_sibling(gpu, oracle, weights_tiny, fmt):
    nv12 = _random(W, H)
    data = C.format_bytes(fmt, nv12, W, H, rng=np.random.default_rng(5))
    trk = {k: gpu.VitTrack.new(weights_tiny, use_graph=False) for k in ("sib", "host", "wide", "pixel")}
    plain, kp = _dev(gpu, fmt, data, W, H)
    macro, km = _dev(gpu, fmt, data, W, H)
    macro.format = gpu.frame_format(C.pix(gpu, fmt), gpu.COLOR_BT601, False)
    assert macro.format == plain.format == C.pix(gpu, fmt)      # code 0 spelled with the macro is the plain format
    for code in C.NEW_CODES:
        fr = {"sib": _sibling(W, H, code), "host": C.host_frame(gpu, fmt, data, W, H, code)}
        fr["wide"], k1 = _dev(gpu, fmt, data, W, H, code, aligned=True, fill=0xA5)
        fr["pixel"], k2 = _dev(gpu, fmt, data, W, H, code, aligned=False, fill=0x5A)
        assert fr["host"].cframe().format == fr["wide"].format == C.word(gpu, fmt, code) != C.pix(gpu, fmt)
        for box in BOXES:
            want = _oracle_patches(oracle, weights_tiny, W, H, code, box)
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
                    assert np.array_equal(_patches(t), want), (fmt, code, k, box, tier)
                assert all(v == res["sib"] for v in res.values()), (fmt, code, box, tier, res)
    # code 0: the plain value and the macro's spelling are one frame, and it is BT.601 limited range
    want = _oracle_patches(oracle, weights_tiny, W, H, 0, BOXES[0])
    for f in (plain, macro):
        trk["wide"].init_device(f, gpu.BBox.new(*BOXES[0]))
        trk["wide"].update_device(f)
        assert np.array_equal(_patches(trk["wide"]), want), fmt


# ---- 2. windows, views, odd sizes, graph replays --------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", C.YUV_FORMATS)
def test_windows_views_odd_sizes_and_graph_replays(gpu, oracle, weights_tiny, fmt):
    """a packed window, a pointer-offset view and a window ending at the odd edge of a 637x479 frame (the 4:2:2 formats have
    even widths only: 640x480) give the whole sibling frame's patch matrix and result; a two-stream group replays them"""
    odd_ok = C.FAMILY[fmt] == "420" and fmt != "nv16"
    codes = (3, 4)
    for (w, h) in ([(640, 480), (637, 479)] if odd_ok else [(640, 480)]):
        nv12 = _random(w, h)
        data = C.format_bytes(fmt, nv12, w, h, rng=np.random.default_rng(6))
        ts = gpu.VitTrack.new(weights_tiny, use_graph=False)
        tn = gpu.VitTrack.new(weights_tiny, use_graph=False)
        cases = [((288, 208, 64, 64), (160, 96, 384, 320)), ((440, 330, 40, 40), (320, 240, w - 320, h - 240))]
        for code in codes:
            sib = _sibling(w, h, code)
            for box, win in cases:
                want = _oracle_patches(oracle, weights_tiny, w, h, code, box)
                ts.init(sib, gpu.BBox.new(*box))
                rs = _res(ts.update(sib))
                assert np.array_equal(_patches(ts), want)
                hf = C.host_frame(gpu, fmt, data, w, h, code)
                tn.init(hf, gpu.BBox.new(*box))
                assert _res(tn.update(hf)) == rs and np.array_equal(_patches(tn), want), (fmt, w, h, code, box)
                for aligned in (True, False):
                    for kw in ({}, {"window": win}, {"view": win}):
                        f, keep = _dev(gpu, fmt, data, w, h, code, aligned=aligned, fill=0x33, **kw)
                        for tier in (0, 2):
                            tn.as_group().set_tuning("crop_tier", tier)
                            tn.init_device(f, gpu.BBox.new(*box))
                            r = _res(tn.update_device(f))
                            assert np.array_equal(_patches(tn), want) and r == rs, (fmt, w, h, code, box, aligned, kw, tier)
                        tn.as_group().set_tuning("crop_tier", -1)
        # graph replays: a group of two streams, every tier forced, replays what the eager tracker computed
        code, box = codes[0], cases[0][0]
        sib = _sibling(w, h, code)
        ts.init(sib, gpu.BBox.new(*box))
        rs = _res(ts.update(sib))
        for tier in (-1, 0, 1, 2):
            g = gpu.Group(weights_tiny, n_streams=2, use_graph=True)
            g.set_tuning("crop_tier", tier)
            f, keep = _dev(gpu, fmt, data, w, h, code, aligned=True)
            for i in range(2):
                g.init_device(i, f, gpu.BBox.new(*box))
            r = g.update_device([f, f])
            assert [_res(x) for x in r] == [rs, rs] and g.read_tensor("graph_replays").sum() == 1, (fmt, tier)
            assert g.read_tensor("patches", 1).tobytes() == _patches(ts).tobytes()
            g.close()


# ---- 3. closed loop -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,code", [("nv12", 3), ("i420", 4)])
def test_closed_loop_is_the_rgb8_siblings_run(gpu, weights_tiny, fmt, code):
    """40 frames of the moving square: the coloured frames through a single tracker and a two-stream group give the boxes,
    score bits and flags of the run on the RGB8 sibling frames; read as plain NV12 the same bytes give another patch matrix"""
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    n = 40
    trk = {k: gpu.VitTrack.new(weights_tiny) for k in ("sib", "host", "dev", "plain")}
    grp = {k: gpu.Group(weights_tiny, n_streams=2) for k in ("sib", "new")}
    out = {k: [] for k in ("sib", "host", "dev", "gsib", "gnew")}
    box = gpu.BBox.new(*sc.gt_box(0))
    for t in range(n):
        nv12 = sc.frame_nv12(t)
        data = C.format_bytes(fmt, nv12, W, H)
        sib = C.sibling_of(fmt, nv12, W, H, code)
        fd, keep = _dev(gpu, fmt, data, W, H, code)
        fs, keep2 = _dev(gpu, "rgb8", sib, W, H)
        host = C.host_frame(gpu, fmt, data, W, H, code)
        if t == 0:
            trk["sib"].init(sib, box)
            trk["host"].init(host, box)
            trk["dev"].init_device(fd, box)
            trk["plain"].init(C.host_frame(gpu, fmt, data, W, H, 0), box)
            for i in range(2):
                grp["sib"].init_device(i, fs, box)
                grp["new"].init_device(i, fd, box)
            continue
        out["sib"].append(_res(trk["sib"].update(sib)))
        out["host"].append(_res(trk["host"].update(host)))
        out["dev"].append(_res(trk["dev"].update_device(fd)))
        out["gsib"].append([_res(r) for r in grp["sib"].update_device([fs, fs])])
        out["gnew"].append([_res(r) for r in grp["new"].update_device([fd, fd])])
        if t == 1:
            trk["plain"].update(C.host_frame(gpu, fmt, data, W, H, 0))
            assert _patches(trk["host"]).tobytes() == _patches(trk["sib"]).tobytes()
            assert _patches(trk["plain"]).tobytes() != _patches(trk["host"]).tobytes(), "the colour bits are ignored"
    assert out["host"] == out["sib"] and out["dev"] == out["sib"]
    assert out["gnew"] == out["gsib"] and [g[0] for g in out["gsib"]] == out["sib"]
    assert len(set(r[0] for r in out["sib"])) > n // 4, "the sibling run's box hardly moves: the comparison shows little"


# ---- 4. one pass, several codes -------------------------------------------------------------------------------------------

SLOTS = [("nv12", 0), ("nv12", 2), ("i420", 5), ("rgb8", 0)]


def _slot_frames(gpu, t, sibling):
    """(host frame objects, [(format, bytes, code)]) of the four slots at time t: each slot its own random picture"""
    host, raw = [], []
    for i, (fmt, code) in enumerate(SLOTS):
        if fmt == "rgb8":
            img = np.random.default_rng(900 + 10 * t + i).integers(0, 256, (H, W, 3), dtype=np.uint8)
            host.append(img)
            raw.append(("rgb8", img, 0))
            continue
        nv12 = _random(W, H, seed=900 + 10 * t + i)
        if sibling:
            img = _sibling(W, H, code, seed=900 + 10 * t + i)
            host.append(img)
            raw.append(("rgb8", img, 0))
        else:
            data = C.format_bytes(fmt, nv12, W, H)
            host.append(C.host_frame(gpu, fmt, data, W, H, code))
            raw.append((fmt, data, code))
    return host, raw


def _devs(gpu, raw, streams=None):
    out = [_dev(gpu, f, d, W, H, c) for (f, d, c) in (raw if streams is None else [raw[s] for s in streams])]
    return [o[0] for o in out], out


def test_one_pass_with_slots_of_different_codes(gpu, weights_tiny):
    B, T = 4, 8
    g_new, g_sib, g_dev, g_dsib = (gpu.Group(weights_tiny, n_streams=B) for _ in range(4))
    p_new, p_sib = (gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=-1) for _ in range(2))
    new = [_slot_frames(gpu, t, False) for t in range(T)]
    sib = [_slot_frames(gpu, t, True) for t in range(T)]
    boxes = [gpu.BBox.new(288 + 8 * i, 208 - 6 * i, 64, 64) for i in range(B)]
    fn0, k0 = _devs(gpu, new[0][1])
    fs0, k1 = _devs(gpu, sib[0][1])
    for i in range(B):
        for g, fr in ((g_new, new), (p_new, new), (g_sib, sib), (p_sib, sib)):
            g.init_host(i, fr[0][0][i], boxes[i])
        g_dev.init_device(i, fn0[i], boxes[i])
        g_dsib.init_device(i, fs0[i], boxes[i])
    sync = []
    for t in range(1, T):
        fn, kn = _devs(gpu, new[t][1])
        fs, ks = _devs(gpu, sib[t][1])
        r = [[_res(x) for x in rr] for rr in (g_new.update_host(new[t][0]), g_sib.update_host(sib[t][0]), g_dev.update_device(fn),
                                              g_dsib.update_device(fs))]
        assert r[0] == r[1] == r[2] == r[3], t
        sync.append(r[0])
    for i in range(B):
        assert g_new.read_tensor("state", i).tobytes() == g_sib.read_tensor("state", i).tobytes() == \
            g_dev.read_tensor("state", i).tobytes() == g_dsib.read_tensor("state", i).tobytes(), i
    # pipelined host passes (speculative windows without enlargement: passes are redone) equal the synchronous ones bit for bit
    pipe, pipe_sib = [], []
    p_new.enqueue_host(new[1][0])
    p_sib.enqueue_host(sib[1][0])
    for t in range(2, T):
        p_new.enqueue_host(new[t][0])
        p_sib.enqueue_host(sib[t][0])
        pipe.append([_res(r) for r in p_new.wait_next()])
        pipe_sib.append([_res(r) for r in p_sib.wait_next()])
    pipe.append([_res(r) for r in p_new.wait_next()])
    pipe_sib.append([_res(r) for r in p_sib.wait_next()])
    assert pipe == pipe_sib == sync
    print(f"\n[colorimetry] redone passes: {p_new.host_redos()} / {p_sib.host_redos()}")
    assert p_new.host_redos() > 0 and p_new.host_redos() == p_sib.host_redos()
    # a subset pass: slots 2, 0, 1 of the streams, host and device frames
    L = [2, 0, 1]
    fn, kn = _devs(gpu, new[0][1], L)
    fs, ks = _devs(gpu, sib[0][1], L)
    r = [[_res(x) for x in rr] for rr in (g_new.update_host([new[0][0][s] for s in L], streams=L),
                                          g_sib.update_host([sib[0][0][s] for s in L], streams=L),
                                          g_dev.update_device(fn, streams=L), g_dsib.update_device(fs, streams=L))]
    assert r[0] == r[1] == r[2] == r[3]
    # a candidate pass: two slots of stream 1 (NV12, BT.709 limited), one of stream 2 (I420, BT.2020 full), one of stream 0
    b1 = g_new.read_state(1)["box"]
    cands = [(1, None), (2, None), (1, [b1[0] + 20, b1[1] - 12, b1[2], b1[3]]), (0, None)]
    order = [1, 2, 1, 0]
    fn, kn = _devs(gpu, new[3][1], order)
    fs, ks = _devs(gpu, sib[3][1], order)
    (rd, wd), (rs, ws) = g_dev.update_device_candidates(cands, fn), g_dsib.update_device_candidates(cands, fs)
    (rh, wh), (rt, wt) = (g_new.update_host_candidates(cands, [new[3][0][s] for s in order]),
                          g_sib.update_host_candidates(cands, [sib[3][0][s] for s in order]))
    assert [_res(x) for x in rd] == [_res(x) for x in rs] == [_res(x) for x in rh] == [_res(x) for x in rt]
    assert wd == ws == wh == wt
    for i in range(B):
        assert g_new.read_tensor("state", i).tobytes() == g_sib.read_tensor("state", i).tobytes() == \
            g_dev.read_tensor("state", i).tobytes() == g_dsib.read_tensor("state", i).tobytes(), i


# ---- 5. every frame reader ------------------------------------------------------------------------------------------------

def _all_on(gpu, g, kind):
    g.set_template_refresh(2, 0.0)          # the shortest period the engine accepts (0 = off, else 2..1000000)
    g.enable_chips(64, kind)
    g.set_chips(2.0, 1, 0)
    g.set_peaks(3)
    g.set_appearance(True)
    g.set_proposals(2)                  # mode 2: every update evaluates
    g.set_health(True)
    g.set_arbitration(True)
    g.set_tuning("result_overlay", 7)


def _observe(g, n):
    chips, infos = g.read_chips()
    return dict(states=[g.read_tensor("state", s).tobytes() for s in range(n)], peaks=g.last_peaks().tobytes(), chips=chips.tobytes(),
                chip_infos=infos, templates=[g.read_tensor("template", s).tobytes() for s in range(n)],
                appearance=[g.appearance(s) for s in range(n)], anchors=[g.anchor(s).tobytes() for s in range(n)],
                proposals=[g.proposals(s) for s in range(n)], health=[g.frame_health(s) for s in range(n)],
                arbitration=[g.read_tensor("arbitrate", s).tobytes() for s in range(n)], refresh=[g.template_refresh_stats(s) for s in range(n)],
                overlay=[g.result_overlay_stats(s) for s in range(n)])


@pytest.mark.parametrize("kind", ["bf16", "rgb8"])
def test_every_frame_reader_of_a_full_engine(gpu, weights_tiny, kind):
    """template refresh (period 2, the engine's shortest), chips, peaks, appearance, proposals on every update, health, arbitration and the result
    overlay enabled: NV12 with BT.709 limited against the RGB8 sibling in a twin, 6 updates, everything the host can see"""
    code, n = 2, 2
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=40 + i) for i in range(n)]
    ck = gpu.CHIP_NORM_BF16 if kind == "bf16" else gpu.CHIP_RGB8
    g_new, g_sib = gpu.Group(weights_tiny, n_streams=n), gpu.Group(weights_tiny, n_streams=n)
    for g in (g_new, g_sib):
        _all_on(gpu, g, ck)
    for t in range(7):
        fn, fs, keep = [], [], []
        for i in range(n):
            nv12 = scs[i].frame_nv12(t)
            for lst, (f, k) in ((fn, _dev(gpu, "nv12", nv12, W, H, code)), (fs, _dev(gpu, "rgb8", C.sibling_of("nv12", nv12, W, H, code), W, H))):
                lst.append(f)
                keep.append(k)
        if t == 0:
            for i in range(n):
                g_new.init_device(i, fn[i], gpu.BBox.new(*scs[i].gt_box(0)))
                g_sib.init_device(i, fs[i], gpu.BBox.new(*scs[i].gt_box(0)))
            continue
        rn, rs = g_new.update_device(fn), g_sib.update_device(fs)
        assert [_res(r) for r in rn] == [_res(r) for r in rs], t
        on, os_ = _observe(g_new, n), _observe(g_sib, n)
        for key in on:
            assert on[key] == os_[key], (t, key)
    assert g_new.template_refresh_stats(0)["generation"] > 0 and g_new.result_overlay_stats(0)["n_drawn"] > 0
    assert sum(g_new.proposals(s)["evaluated"] for s in range(n)) > 0 and sum(g_new.appearance(s)["evaluated"] for s in range(n)) > 0


def test_the_overlay_draws_the_luma_it_draws_on_plain_nv12(gpu):
    """the result overlay writes luma values and does not depend on the code: the same results drawn into the same bytes,
    once declared BT.709 full range and once plain NV12, leave the same bytes"""
    nv12 = gpu.synth.MovingSquare(W, H, 64, seed=3).frame_nv12(0)
    res = np.zeros(1, gpu.RESULT_DTYPE)
    res["success"], res["score"], res["bbox"] = 1, 0.9, (200, 150, 90, 70)
    out = []
    for code in (0, 3):
        f, keep = _dev(gpu, "nv12", nv12, W, H, code)
        st = gpu.op_result_overlay([f], res)
        out.append((keep.cpu().numpy().tobytes(), st.tobytes()))
    assert out[0] == out[1]
    assert out[0][0] != _dev(gpu, "nv12", nv12, W, H)[1].cpu().numpy().tobytes(), "nothing was drawn"


def test_the_frame_hooks_read_a_coloured_frame_as_its_rgb8_sibling(gpu, weights_tiny):
    """op_frame_health, op_camera_motion and op_proposals on NV12 / I420 / YUY2 frames with a code give what they give on the
    RGB8 sibling"""
    snapshot = importlib.import_module(gpu.__name__ + ".snapshot")
    w, h = 320, 240
    mi = gpu.model_info_for("tiny")
    T_, patch, kpad = mi.template_size, mi.patch, mi.kpad
    rows = np.random.default_rng(4).integers(0x3c00, 0x4000, ((T_ // patch) ** 2, kpad)).astype(np.uint16)
    norm = (0.02, 0.02, 0.02, -2.0, -2.1, -1.9)
    for fmt, code in (("nv12", 2), ("i420", 5), ("yuy2", 1), ("p010", 4)):
        nv12 = [_random(w, h, seed=70 + k) for k in range(2)]
        st = np.zeros(1, snapshot.STATE)
        st["box"], st["frame_w"], st["frame_h"], st["frames_done"], st["initialized"] = (100.0, 80.0, 48.0, 40.0), w, h, 3, 1
        got = {}
        for name in ("new", "sib"):
            frames = []
            for k in range(2):
                if name == "new":
                    frames.append(_dev(gpu, fmt, C.format_bytes(fmt, nv12[k], w, h), w, h, code))
                else:
                    frames.append(_dev(gpu, "rgb8", C.sibling_of(fmt, nv12[k], w, h, code), w, h))
            h1 = gpu.op_frame_health([frames[0][0]], st, cell=4, max_cells=8192)
            h2 = gpu.op_frame_health([frames[1][0]], st, cell=4, max_cells=8192, **{k: h1[k] for k in ("thumbs", "hist", "records", "counts")})
            c1 = gpu.op_camera_motion([frames[0][0]], st, cell=4, max_cells=8192)
            c2 = gpu.op_camera_motion([frames[1][0]], st, cell=4, max_cells=8192, thumbs=c1["thumbs"], records=c1["records"])
            r = np.zeros(1, gpu.RESULT_DTYPE)
            p = gpu.op_proposals([frames[0][0]], st, r, rows[None, None], T_, patch, norm, min_sim_pm=0, max_cells=8192)
            got[name] = {f"{tag}.{k}": np.asarray(v).tobytes() for tag, d in (("h2", h2), ("c2", c2), ("p", p)) for k, v in d.items()
                         if isinstance(v, np.ndarray)}
        assert got["new"].keys() == got["sib"].keys()
        for k in got["new"]:
            assert got["new"][k] == got["sib"][k], (fmt, code, k)


# ---- 6. graphs ------------------------------------------------------------------------------------------------------------

def test_graphs_one_more_set_at_the_first_coloured_init_never_in_an_update(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=2)
    nv12 = sc.frame_nv12(0)
    g = gpu.Group(weights_tiny, n_streams=2)
    tiers = g.graph_captures()
    assert tiers == 3
    plain, k0 = _dev(gpu, "nv12", nv12, W, H)
    i420, k1 = _dev(gpu, "i420", C.format_bytes("i420", nv12, W, H), W, H)
    col, k2 = _dev(gpu, "nv12", nv12, W, H, 2)
    col2, k3 = _dev(gpu, "i420", C.format_bytes("i420", nv12, W, H), W, H, 5)
    box = gpu.BBox.new(*sc.gt_box(0))
    for i in range(2):
        g.init_device(i, plain, box)
    g.update_device([plain, plain])
    assert g.graph_captures() == tiers, "an engine that only sees plain NV12 captured more than its creation did"
    g.init_device(1, i420, box)
    assert g.graph_captures() == 2 * tiers
    g.update_device([plain, i420])
    assert g.graph_captures() == 2 * tiers
    g.init_device(0, col, box)
    assert g.graph_captures() == 3 * tiers, "the first init on a coloured frame captures exactly one more set"
    g.init_device(1, col2, box)
    g.init_device(0, col, box)
    assert g.graph_captures() == 3 * tiers
    before = int(g.read_tensor("graph_replays").sum())
    for s in (40, 64, 100, 160, 230):           # through the tier boundaries of the tiny model's crop
        for i in range(2):
            g.set_state_box(i, [320 - s / 2, 240 - s / 2, s, s])
        g.update_device([col, col2])
        g.update_device([plain, col2])
        g.update_device([i420, plain])
    assert g.graph_captures() == 3 * tiers, "a pass captured a graph on the hot path"
    assert int(g.read_tensor("graph_replays").sum()) == before + 15
    # an engine that never had a stream initialised on a coloured frame launches such a pass eagerly, and right
    e, twin = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    e.init_device(0, plain, box)
    twin.init_device(0, col, box)
    caps, replays = e.graph_captures(), int(e.read_tensor("graph_replays").sum())
    twin.init_device(0, plain, box)
    assert [_res(r) for r in e.update_device([col])] == [_res(r) for r in twin.update_device([col])]
    assert e.graph_captures() == caps and int(e.read_tensor("graph_replays").sum()) == replays


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------

def test_bad_format_words_are_refused_and_change_nothing(gpu, weights_tiny):
    import torch
    L_ = gpu.lib()
    sc = gpu.synth.MovingSquare(W, H, 64, seed=3)
    buf = sc.frame_nv12(0)
    d = torch.from_numpy(np.concatenate([buf, np.zeros(4 * W * H, np.uint8)])).cuda()
    p = d.data_ptr()
    q = p + W * H
    good = gpu.frame_nv12(p, q, W, H, matrix=gpu.COLOR_BT709)
    trk, twin = gpu.VitTrack.new(weights_tiny), gpu.VitTrack.new(weights_tiny)
    for t_ in (trk, twin):
        t_.init_device(good, gpu.BBox.new(*sc.gt_box(0)))
        t_.update_device(good)
    g = trk.as_group()
    before = g.read_tensor("state").tobytes()
    F, P = gpu.CFrame, gpu
    ff = gpu.frame_format
    bad = [(F(p, None, W, H, 3 * W, 0, ff(P.PIX_RGB8, 1, False), 0, 0, 0, 0, 0), "rgb8"),       # colour bits without chroma
           (F(p, None, W, H, 3 * W, 0, ff(P.PIX_RGB8, 0, True), 0, 0, 0, 0, 0), "rgb8"),
           (F(p, None, W, H, 4 * W, 0, ff(P.PIX_BGRX, 2, False), 0, 0, 0, 0, 0), "bgrx"),
           (F(p, None, W, H, W, 0, ff(P.PIX_GRAY8, 0, True), 0, 0, 0, 0, 0), "gray8"),
           (F(p, q, W, H, W, W, P.PIX_NV12 | 3 << 8, 0, 0, 0, 0, 0), "nv12"),                   # matrix 3
           (F(p, q, W, H, W, W // 2, P.PIX_I420 | 3 << 8 | 1 << 12, 0, 0, 0, 0, 0), "i420"),
           (F(p, q, W, H, W, W, P.PIX_NV12 | 2 << 12, 0, 0, 0, 0, 0), "nv12"),                  # range 2
           (F(p, None, W, H, 2 * W, 0, P.PIX_YUY2 | 1 << 8 | 2 << 12, 0, 0, 0, 0, 0), "yuy2"),
           (F(p, q, W, H, W, W, P.PIX_NV12 | 1 << 16, 0, 0, 0, 0, 0), "nv12"),                  # bit 16
           (F(p, q, W, H, W, W, ff(P.PIX_NV12, 1, True) | 1 << 16, 0, 0, 0, 0, 0), "nv12"),
           (F(p, None, W, H, 3 * W, 0, P.PIX_RGB8 | 1 << 16, 0, 0, 0, 0, 0), "rgb8")]
    r = gpu.CResult()
    box = gpu.BBox.new(10, 10, 40, 40)._c()
    host = np.zeros(8 * W * H, np.uint8)
    grp = gpu.Group(weights_tiny, n_streams=1)
    grp.init_device(0, good, gpu.BBox.new(*sc.gt_box(0)))
    st = grp.read_tensor("state").tobytes()
    # a two-stream group with a pipelined pass of stream 1 outstanding: the queued form of vt_group_enqueue_init_host
    good_host = gpu.NV12Frame(buf, W, H, matrix=gpu.COLOR_BT709)
    grp2 = gpu.Group(weights_tiny, n_streams=2)
    for i in range(2):
        grp2.init_host(i, good_host, gpu.BBox.new(*sc.gt_box(0)))
    st2 = grp2.read_tensor("state", 0).tobytes()
    grp2.enqueue_host([good_host], streams=[1])
    mi = gpu.model_info_for("tiny")
    rows = np.full(((mi.template_size // mi.patch) ** 2, mi.kpad), 0x3f80, np.uint16)
    for f, name in bad:
        tag = hex(f.format & 0xffffffff)
        assert L_.vt_update_frame(trk._h, ctypes.byref(f), 1, ctypes.byref(r)) == INVALID, tag
        text = L_.vt_last_error().decode()
        assert name in text, (tag, text)                # the text names the format
        assert L_.vt_init_frame(trk._h, ctypes.byref(f), 1, box) == INVALID, tag
        hf = gpu.CFrame(*[getattr(f, n) for n, _ in gpu.CFrame._fields_])
        hf.plane0 = host.ctypes.data
        hf.plane1 = host.ctypes.data + 2 * W * H if f.plane1 else None
        assert L_.vt_update_frame(trk._h, ctypes.byref(hf), 0, ctypes.byref(r)) == INVALID, tag
        assert name in L_.vt_last_error().decode(), tag
        assert L_.vt_init_frame(trk._h, ctypes.byref(hf), 0, box) == INVALID, tag
        for call in (lambda: grp.init_device(0, f, gpu.BBox.new(10, 10, 40, 40)), lambda: grp.update_device([f]),
                     lambda: grp.enqueue_device([f]), lambda: grp.update_device([f], streams=[0]),
                     lambda: grp.update_device_candidates([(0, None)], [f])):
            with pytest.raises(gpu.VtError) as ei:
                call()
            assert ei.value.code == INVALID and name in str(ei.value), (tag, str(ei.value))
        hcalls = [lambda: L_.vt_group_init_host(grp._h, 0, ctypes.byref(hf), box),
                  lambda: L_.vt_group_update_host(grp._h, ctypes.byref(hf), 1, ctypes.byref(r)),
                  lambda: L_.vt_group_enqueue_host(grp._h, ctypes.byref(hf), 1),
                  lambda: L_.vt_group_enqueue_init_host(grp._h, 0, ctypes.byref(hf), box),          # nothing outstanding
                  lambda: L_.vt_group_enqueue_init_host(grp2._h, 0, ctypes.byref(hf), box)]         # behind a pass of stream 1
        for call in hcalls:
            assert call() == INVALID, tag
            assert name in L_.vt_last_error().decode(), tag
        # the operator hooks that take frames
        snapshot = importlib.import_module(gpu.__name__ + ".snapshot")
        s1 = np.zeros(1, snapshot.STATE)
        s1["box"], s1["frame_w"], s1["frame_h"], s1["frames_done"], s1["initialized"] = (100.0, 80.0, 48.0, 40.0), W, H, 3, 1
        for hook in (lambda: gpu.op_frame_health([f], s1), lambda: gpu.op_camera_motion([f], s1),
                     lambda: gpu.op_result_overlay([f], np.zeros(1, gpu.RESULT_DTYPE)),
                     lambda: gpu.op_proposals([f], s1, np.zeros(1, gpu.RESULT_DTYPE), rows[None, None], mi.template_size, mi.patch,
                                              (0.02, 0.02, 0.02, -2.0, -2.1, -1.9), max_cells=8192)):
            with pytest.raises(gpu.VtError) as ei:
                hook()
            assert ei.value.code == INVALID and name in str(ei.value), tag
    assert len(grp2.wait_next()) == 1 and grp2.read_tensor("state", 0).tobytes() == st2     # the outstanding pass was stream 1's
    assert g.read_tensor("state").tobytes() == before and grp.read_tensor("state").tobytes() == st
    assert _res(trk.update_device(good)) == _res(twin.update_device(good))
