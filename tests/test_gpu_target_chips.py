"""Target chips (vt_group_enable_chips / set_chips / read_chips; DESIGN.md section 3, "Target chips"), on the MI355X.
Everything here is bit-exact. The yardsticks: the oracle's vto_preproc with patch = C, kpad = 3 C^2 (the bf16 kind), the
numpy restatement of tests/target_chips_util.py (the u8 kind, the gate), and engines that run the same clip through another
kind of pass. tests/test_target_chips_abi.py ties the restatement to the oracle and pins, on the oracle, that the clips used
here cut, skip and fail where needed.

A stream's results depend, bit for bit, on the size of the pass it runs in (tests/test_gpu_stream_subsets.py), so the pass
kinds are compared at ONE pass size: two slots. The candidate pass (three slots of one stream) is held to the oracle at the
box it committed."""
import numpy as np
import pytest

import target_chips_util as u
from test_gpu_pixel_formats import _nv12_to_yuy2, _permute, _res
from test_target_chips_abi import CLIPS

pytestmark = pytest.mark.gpu

W, H = 640, 480
INVALID, OOM = -1, -8
NORMS = ((1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044))      # a consumer's own, not the tracker's


def _frame(gpu, oracle, sc, t, fmt, w=W, h=H):
    """clip time t in `fmt` -> (device CFrame, keep-alive, oracle Frame of the same pixels, the pixels as RGB8).
    nv12p: NV12 with padded strides; rgb8odd: the left 637 columns; bgrx / nv21: the permuted siblings of rgb8 / nv12"""
    import torch
    rgb = sc.frame_rgb8(t)
    if fmt in ("rgb8", "rgb8odd", "bgrx"):
        if fmt == "rgb8odd":
            w = 637
            rgb = np.ascontiguousarray(rgb[:, :w])
        of = oracle.Frame.rgb8(rgb)
        if fmt == "bgrx":
            d = torch.from_numpy(np.ascontiguousarray(_permute("bgrx", rgb, w, h, xbyte=9))).cuda()
            return gpu.frame_bgrx(d.data_ptr(), w, h), d, of, rgb
        d = torch.from_numpy(rgb).cuda()
        return gpu.frame_rgb8(d.data_ptr(), w, h), d, of, rgb
    buf = sc.frame_nv12(t)
    if fmt == "yuy2":
        y = _nv12_to_yuy2(buf, w, h)
        d = torch.from_numpy(y).cuda()
        return gpu.CFrame(d.data_ptr(), None, w, h, 2 * w, 0, gpu.PIX_YUY2, 0, 0, 0, 0, 0), d, oracle.Frame.yuy2(y, w, h), rgb
    of = oracle.Frame.nv12(buf, w, h)
    if fmt == "nv21":
        d = torch.from_numpy(_permute("nv21", buf, w, h)).cuda()
        return gpu.CFrame(d.data_ptr(), d.data_ptr() + w * h, w, h, w, w, gpu.PIX_NV21, 0, 0, 0, 0, 0), d, of, rgb
    if fmt == "nv12":
        d = torch.from_numpy(buf).cuda()
        return gpu.frame_nv12(d.data_ptr(), d.data_ptr() + w * h, w, h), d, of, rgb
    assert fmt == "nv12p"
    sy, suv = w + 8, w + 16
    pad = np.full(sy * h + suv * (h // 2), 0x5a, np.uint8)
    pad[:sy * h].reshape(h, sy)[:, :w] = buf[:w * h].reshape(h, w)
    pad[sy * h:].reshape(h // 2, suv)[:, :w] = buf[w * h:].reshape(h // 2, w)
    d = torch.from_numpy(pad).cuda()
    return gpu.frame_nv12(d.data_ptr(), d.data_ptr() + sy * h, w, h, sy, suv), d, of, rgb


def _want(oracle, kind, of, rgb, box, factor, C):
    if kind == u.NORM_BF16:
        return u.oracle_chip_bf16(of, box, factor, C, *NORMS)
    return u.chip_u8(u.bilinear(rgb, box, factor, C))


def _info_words(g, streams=None):
    """the raw records, for bit-for-bit comparisons"""
    import ctypes
    n = g.streams if streams is None else len(streams)
    lst = list(range(n)) if streams is None else streams
    infos = (gpu_mod.CChipInfo * n)()
    gpu_mod._check(gpu_mod.lib().vt_group_read_chips(g._h, (ctypes.c_int * n)(*lst), n, None, 0, infos))
    return np.frombuffer(bytes(infos), np.uint32).reshape(n, 12).copy()


gpu_mod = None


@pytest.fixture(autouse=True)
def _module(gpu):
    global gpu_mod
    gpu_mod = gpu


def _state_words(g, s):
    return g.read_tensor("state", s).view(np.uint32).copy()


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------------

CASES = [   # C, kind, square, factor, format, MovingSquare keyword arguments
    (64, u.NORM_BF16, 64, 1.0, "rgb8", {}),                 # the tile body, its tile staged in LDS (64 x 32 source pixels)
    (64, u.NORM_BF16, 64, 1.0, "nv12p", {}),                # ... NV12 with padded strides: the 8-pixel group loads
    (64, u.NORM_BF16, 64, 2.0, "rgb8", {}),                 # 128 x 64 source pixels per tile: over the pass's tier 0, per-pixel path
    (40, u.NORM_BF16, 64, 2.0, "nv12p", {}),                # the wide-store body
    (64, u.NORM_BF16, 200, 2.0, "yuy2", {}),                # a 200-px target: the rectangle exceeds every LDS tier
    (64, u.NORM_BF16, 64, 1.0, "bgrx", {}),                 # the kernels that read any layout, against the RGB8 sibling
    (40, u.NORM_BF16, 64, 1.0, "nv21", {}),                 # ... against the NV12 sibling
    (64, u.NORM_BF16, 64, 2.0, "rgb8odd", {}),              # an odd-width frame
    (64, u.NORM_BF16, 64, 3.0, "nv12", dict(center=(30.0, 30.0), amp=3.0)),     # the frame's corner: black taps
    (64, u.RGB8, 64, 1.0, "nv12p", {}),                     # the u8 store behind the staged tile
    (64, u.RGB8, 64, 2.0, "rgb8", {}),                      # ... behind the per-pixel path
    (40, u.RGB8, 64, 2.0, "yuy2", {}),                      # ... of the wide body
    (64, u.RGB8, 200, 2.0, "rgb8", {}),
    (64, u.RGB8, 64, 1.5, "bgrx", dict(center=(30.0, 30.0), amp=3.0)),      # the corner, through the 16-byte RGBX loads
    (40, u.RGB8, 64, 2.0, "rgb8odd", {}),
]


@pytest.mark.parametrize("C,kind,sq,factor,fmt,kw", CASES)
def test_chip_equals_the_oracle_after_every_update(gpu, oracle, weights_tiny, C, kind, sq, factor, fmt, kw):
    sc = gpu.synth.MovingSquare(W, H, sq, seed=0, **kw)
    g = gpu.Group(weights_tiny, n_streams=1)
    f0, k0, _, _ = _frame(gpu, oracle, sc, 0, fmt)
    g.init_device(0, f0, gpu.BBox.new(*sc.gt_box(0)))
    g.enable_chips(C, kind, *NORMS)
    g.set_chips(factor)
    black = 0
    for t in range(4):
        f, k, of, rgb = _frame(gpu, oracle, sc, t, fmt)
        r = g.update_device([f])[0]
        st = g.read_state(0)
        box = tuple(float(v) for v in r.bbox) if r.success else tuple(float(v) for v in st["box"])
        assert tuple(float(v) for v in st["box"]) == box
        chips, infos = g.read_chips()
        i = infos[0]
        assert (i["status"], i["frames_done"], i["success"], i["box"]) == (u.CUT, t + 1, int(r.success), tuple(int(v) for v in box)), i
        assert np.float32(i["score"]) == np.float32(r.score)
        geo = u.chip_geometry(box, factor, C)
        assert np.array_equal(np.float32(i["geo"]).view(np.uint32), geo[:3].view(np.uint32)), (i["geo"], geo)
        want = _want(oracle, kind, of, rgb, box, factor, C)
        assert chips[0].shape == want.shape and chips[0].dtype == want.dtype
        assert np.array_equal(chips[0], want), f"update {t + 1}: {(chips[0] != want).sum()} of {want.size} elements differ"
        black += int(geo[0] < -1 or geo[1] < -1)
        assert want.any()
    if "center" in kw:
        assert black == 4, "the chip crop does not leave the frame: the corner case shows nothing"
    g.close()


# ---- 2. pass kinds ----------------------------------------------------------------------------------------------------------------

def _record(g, streams):
    chips, infos = g.read_chips(streams)
    return [(chips[i].copy() if infos[i]["status"] == u.CUT else None) for i in range(len(streams))], _info_words(g, streams)


def _same(a, b, tag):
    assert np.array_equal(a[1], b[1]), f"{tag}: infos differ\n{a[1]}\n{b[1]}"
    for s, (x, y) in enumerate(zip(a[0], b[0])):
        assert (x is None) == (y is None) and (x is None or np.array_equal(x, y)), f"{tag}: chip of slot {s} differs"


@pytest.mark.parametrize("kind", [u.NORM_BF16, u.RGB8])
def test_every_kind_of_pass_cuts_the_same_chips(gpu, weights_tiny, kind):
    """two clips (seeds 1, 2; every second clip frame), C 64, factor 2, period 2 phase 1 on the second clip: full device
    passes, device passes over the shuffled list [2, 0] of a three-stream engine, synchronous host passes and pipelined
    host passes - with the default margin and with margin -1, where the speculative windows miss and passes are redone.
    The pipelined runs read the chips whenever no younger pass has been queued behind the one collected (the store has
    one buffer per stream): two schedules cover every frame."""
    import torch
    N, C = 12, 64
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in (1, 2)]
    rgb = [[sc.frame_rgb8(2 * i) for sc in scs] for i in range(N)]

    def setup(g, smap=(0, 1), host=False):
        for j, s in enumerate(smap):
            box = gpu.BBox.new(*scs[j].gt_box(0))
            if host:
                g.init_host(s, rgb[0][j], box)
            else:
                d = torch.from_numpy(rgb[0][j]).cuda()
                g.init_device(s, gpu.frame_rgb8(d.data_ptr(), W, H), box)
        g.enable_chips(C, kind, *NORMS)
        g.set_chips(2.0, stream=smap[0])
        g.set_chips(2.0, 2, 1, stream=smap[1])

    def dev(i):
        keep = [torch.from_numpy(a).cuda() for a in rgb[i]]
        return [gpu.frame_rgb8(d.data_ptr(), W, H) for d in keep], keep

    full = gpu.Group(weights_tiny, n_streams=2)
    setup(full)
    want_res, want = [], []
    for i in range(N):
        fr, keep = dev(i)
        want_res.append([_res(r) for r in full.update_device(fr)])
        want.append(_record(full, [0, 1]))
    cut = [[w[0][j] is not None for w in want] for j in range(2)]
    assert all(cut[0]) and cut[1] == [i % 2 == 0 for i in range(N)], cut       # frames_done = i + 1: odd ones are due
    full.close()

    sub = gpu.Group(weights_tiny, n_streams=3)
    setup(sub, smap=(2, 0))
    d1 = torch.from_numpy(rgb[0][0]).cuda()
    sub.init_device(1, gpu.frame_rgb8(d1.data_ptr(), W, H), gpu.BBox.new(*scs[0].gt_box(0)))
    sub.set_chips(2.0, stream=1)
    for i in range(N):
        fr, keep = dev(i)
        assert [_res(r) for r in sub.update_device(fr, streams=[2, 0])] == want_res[i], f"subset pass, frame {i}"
        _same(_record(sub, [2, 0]), want[i], f"subset pass, frame {i}")
    assert not _info_words(sub, [1]).any(), "a stream outside every pass got a record"
    sub.close()

    sync = gpu.Group(weights_tiny, n_streams=2)
    setup(sync, host=True)
    for i in range(N):
        assert [_res(r) for r in sync.update_host(rgb[i])] == want_res[i], f"host pass, frame {i}"
        _same(_record(sync, [0, 1]), want[i], f"host pass, frame {i}")
    assert sync.host_redos() == 0
    sync.close()

    for margin in (0, -1):
        seen = set()
        for first in (0, 1):            # schedule 0: pairs (0,1), (2,3), ...; schedule 1: frame 0 alone, then (1,2), (3,4), ...
            pipe = gpu.Group(weights_tiny, n_streams=2, host_window_margin_pct=margin)
            setup(pipe, host=True)
            i = 0
            if first:
                pipe.enqueue_host(rgb[0])
                assert [_res(r) for r in pipe.wait_next()] == want_res[0]
                _same(_record(pipe, [0, 1]), want[0], f"pipelined (margin {margin}), frame 0")
                seen.add(0)
                i = 1
            while i + 1 < N:
                pipe.enqueue_host(rgb[i])
                pipe.enqueue_host(rgb[i + 1])
                assert [_res(r) for r in pipe.wait_next()] == want_res[i], f"pipelined (margin {margin}), frame {i}"
                assert [_res(r) for r in pipe.wait_next()] == want_res[i + 1], f"pipelined (margin {margin}), frame {i + 1}"
                _same(_record(pipe, [0, 1]), want[i + 1], f"pipelined (margin {margin}), frame {i + 1}")
                seen.add(i + 1)
                i += 2
            if margin < 0:
                assert pipe.host_redos() > 0, "no pass was redone: the redo path was not exercised"
            pipe.close()
        assert seen == set(range(N))


def test_candidate_pass_cuts_the_winners_chip_only(gpu, oracle, weights_tiny):
    """three slots on stream 1 of a three-stream engine (a pass holds at most as many slots as the engine has streams):
    one record, one chip - the oracle's at the box the pass committed"""
    C, factor = 64, 2.0
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in (0, 1, 2)]
    g = gpu.Group(weights_tiny, n_streams=3)
    fr = [_frame(gpu, oracle, sc, 0, "nv12") for sc in scs]
    for s in range(3):
        g.init_device(s, fr[s][0], gpu.BBox.new(*scs[s].gt_box(0)))
    g.enable_chips(C, u.RGB8)
    g.set_chips(factor)
    g.update_device([f[0] for f in fr])
    before_chips, _ = g.read_chips()
    before = _info_words(g)
    for t in (1, 2):
        f, k, of, rgb = _frame(gpu, oracle, scs[1], t, "nv12")
        box = g.read_state(1)["box"]
        cands = [(1, [4.0, 4.0, 40.0, 40.0]), (1, None), (1, [float(box[0]) + 6, float(box[1]) - 4, float(box[2]), float(box[3])])]
        res, win = g.update_device_candidates(cands, [f] * 3)
        assert win[0] in (1, 2) and win == [win[0]] * 3 and res[win[0]].success
        chips, infos = g.read_chips()
        committed = tuple(int(v) for v in res[win[0]].bbox)
        assert (infos[1]["status"], infos[1]["frames_done"], infos[1]["box"]) == (u.CUT, t + 1, committed), infos[1]
        assert tuple(int(v) for v in g.read_state(1)["box"]) == committed
        assert np.array_equal(chips[1], _want(oracle, u.RGB8, of, rgb, committed, factor, C))
        for s in (0, 2):
            assert np.array_equal(_info_words(g)[s], before[s]) and np.array_equal(chips[s], before_chips[s]), f"stream {s} was not in the pass"
    g.close()


def test_refresh_and_chips_on_one_engine(gpu, oracle, weights_tiny):
    """both features on one engine: results and templates are those of the engine that only refreshes (the chip launch
    touches neither), and every chip is the oracle's at the box that engine committed - as on the engine that only cuts
    chips, whose boxes may differ once the templates do"""
    C, factor = 64, 2.0
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    both, refresh, chips_only = (gpu.Group(weights_tiny, n_streams=1) for _ in range(3))
    f0 = _frame(gpu, oracle, sc, 0, "nv12")
    for g in (both, refresh, chips_only):
        g.init_device(0, f0[0], gpu.BBox.new(*sc.gt_box(0)))
    both.set_template_refresh(2, 0.0)
    both.enable_chips(C, u.NORM_BF16, *NORMS)
    both.set_chips(factor)
    refresh.set_template_refresh(2, 0.0)
    chips_only.enable_chips(C, u.NORM_BF16, *NORMS)
    chips_only.set_chips(factor)
    same_box = 0
    for t in range(8):
        f, k, of, rgb = _frame(gpu, oracle, sc, t, "nv12")
        rb, rr, rc = both.update_device([f])[0], refresh.update_device([f])[0], chips_only.update_device([f])[0]
        assert _res(rb) == _res(rr), f"update {t + 1}"
        assert np.array_equal(both.read_tensor("template", 0).view(np.uint32), refresh.read_tensor("template", 0).view(np.uint32))
        assert np.array_equal(_state_words(both, 0), _state_words(refresh, 0))
        for g, r in ((both, rb), (chips_only, rc)):
            chips, infos = g.read_chips()
            assert infos[0]["status"] == u.CUT and r.success
            assert np.array_equal(chips[0], _want(oracle, u.NORM_BF16, of, rgb, r.bbox, factor, C)), f"update {t + 1}"
        same_box += int(tuple(rb.bbox) == tuple(rc.bbox))
    assert both.template_refresh_stats(0)["generation"] == 4 and same_box >= 2
    for g in (both, refresh, chips_only):
        g.close()


@pytest.mark.parametrize("with_refresh", [False, True])
def test_pipelined_equals_synchronous_at_the_frame_edge(gpu, weights_tiny, capsys, with_refresh):
    """The clip of the template refresh's edge test: a 96-px target moving along the left frame edge, every third clip
    frame, margin -1. The search rectangle hangs over the edge, where a speculative window can end inside it without a
    miss of the search crop; the chip (factor 2, C 64: the template crop's geometry) taps denser, and rule 5 then reports
    the pass as a miss so that the redo cuts the chip. With refresh on the same engine the refresh launch has run in the
    pass the chip launch sends back. Whatever the windows were: results, chips, infos, states (and templates) are the
    synchronous run's on every frame."""
    N, C = 16, 64
    sc = gpu.synth.MovingSquare(W, H, 96, seed=7, center=(70.0, 240.0), amp=22.0)
    frames = [[sc.frame_rgb8(3 * i)] for i in range(N)]

    def make(chips=True):
        g = gpu.Group(weights_tiny, n_streams=1, host_window_margin_pct=-1)
        g.init_host(0, frames[0][0], gpu.BBox.new(*sc.gt_box(0)))
        if with_refresh:
            g.set_template_refresh(2, 0.0)
        if chips:
            g.enable_chips(C, u.NORM_BF16, *NORMS)
            g.set_chips(2.0)
        return g

    def tpl(g):
        return g.read_tensor("template", 0).view(np.uint32).copy()

    sync = make()
    want = []
    for i in range(N):
        r = _res(sync.update_host(frames[i])[0])
        want.append((r, _record(sync, [0]), _state_words(sync, 0), tpl(sync)))
    assert all(w[1][0][0] is not None for w in want), "a synchronous pass did not cut"
    assert sync.host_redos() == 0
    redos, seen = [], set()
    for first in (0, 1):
        pipe = make()
        i = 0
        if first:
            pipe.enqueue_host(frames[0])
            assert _res(pipe.wait_next()[0]) == want[0][0]
            i = 1
        while i + 1 < N:
            pipe.enqueue_host(frames[i])
            pipe.enqueue_host(frames[i + 1])
            assert _res(pipe.wait_next()[0]) == want[i][0], f"frame {i}"
            assert _res(pipe.wait_next()[0]) == want[i + 1][0], f"frame {i + 1}"
            _same(_record(pipe, [0]), want[i + 1][1], f"frame {i + 1}")
            assert np.array_equal(_state_words(pipe, 0), want[i + 1][2]), f"frame {i + 1}: state"
            assert np.array_equal(tpl(pipe), want[i + 1][3]), f"frame {i + 1}: template"
            seen.add(i + 1)
            i += 2
        redos.append(pipe.host_redos())
        pipe.close()
    assert seen == set(range(1, N))
    # the same schedule on an engine without chips: the chip launch may only add redos
    bare = make(chips=False)
    for i in range(0, N - 1, 2):
        bare.enqueue_host(frames[i])
        bare.enqueue_host(frames[i + 1])
        bare.wait_next()
        bare.wait_next()
    with capsys.disabled():
        print(f"\n[chips at the edge, refresh {with_refresh}] redos {redos}, without chips {bare.host_redos()}, "
              f"generation {sync.template_refresh_stats(0)['generation']}")
    assert redos[0] > 0 and redos[0] >= bare.host_redos()
    if with_refresh:
        assert sync.template_refresh_stats(0)["generation"] >= 1, "no refresh fired: the case shows nothing"
    bare.close()
    sync.close()


# ---- 3. the gate --------------------------------------------------------------------------------------------------------------------

def _run_clip(gpu, oracle, weights, name, factor, period=1, phase=0, C=64, kind=u.RGB8):
    """clip `name` of tests/test_target_chips_abi.py on one stream -> per update (result, info, chip, wanted chip at the
    state's box), and the restated gate's verdicts on the engine's own states"""
    kw, n, step = CLIPS[name]
    sc = gpu.synth.MovingSquare(W, H, 64, **kw)
    g = gpu.Group(weights, n_streams=1)
    f0 = _frame(gpu, oracle, sc, 0, "rgb8")
    g.init_device(0, f0[0], gpu.BBox.new(*sc.gt_box(0)))
    g.enable_chips(C, kind, *NORMS)
    g.set_chips(factor, period, phase)
    rule = u.ChipRule(C, g.model_info().search_size, factor, period, phase)
    out, verdicts = [], []
    for i in range(n):
        f, k, of, rgb = _frame(gpu, oracle, sc, i * step, "rgb8")
        r = g.update_device([f])[0]
        st = g.read_state(0)
        verdicts.append(rule.step(st["box"], st["geo"]))
        chips, infos = g.read_chips()
        out.append((r, infos[0], chips[0].copy(), _want(oracle, kind, of, rgb, st["box"], factor, C)))
    g.close()
    return out, verdicts, rule


def test_period_and_phase_cut_exactly_the_due_updates(gpu, oracle, weights_tiny):
    out, verdicts, rule = _run_clip(gpu, oracle, weights_tiny, "a", 2.0, 3, 1)
    assert [i["status"] for _, i, _, _ in out] == verdicts
    assert rule.cut == [1, 4, 7, 10] and rule.skipped == []
    last = None
    for n, (r, i, chip, want) in enumerate(out):
        assert i["frames_done"] == n + 1
        if i["status"] == u.CUT:
            assert np.array_equal(chip, want)
            last = chip
        else:
            assert np.array_equal(chip, last), f"update {n + 1} was not due and changed the chip"


@pytest.mark.parametrize("factor,skipped", [(2.0, [2, 6]), (4.0, list(range(2, 13)))])
def test_geometry_skips_say_so_and_keep_the_last_chip(gpu, oracle, weights_tiny, factor, skipped):
    """clip (b): a fast target. The pinned updates (the oracle's, tests/test_target_chips_abi.py) skip with status 2"""
    out, verdicts, rule = _run_clip(gpu, oracle, weights_tiny, "b", factor)
    assert [i["status"] for _, i, _, _ in out] == verdicts
    assert rule.skipped == skipped
    last = None
    for n, (r, i, chip, want) in enumerate(out):
        assert r.success and i["frames_done"] == n + 1 and i["box"] == tuple(int(v) for v in r.bbox)
        if i["status"] == u.CUT:
            assert np.array_equal(chip, want)
            last = chip
        else:
            assert i["status"] == u.SKIPPED and np.array_equal(chip, last), f"update {n + 1}"
            assert not np.array_equal(chip, want), "the skipped chip would have equalled the last one: the check shows nothing"


def test_a_failed_update_cuts_at_the_last_good_box(gpu, oracle, weights_tiny):
    out, verdicts, rule = _run_clip(gpu, oracle, weights_tiny, "c", 2.0, kind=u.NORM_BF16)
    failed = [n + 1 for n, (r, _, _, _) in enumerate(out) if not r.success]
    assert failed == [11, 12, 13, 14, 15, 16]
    good = out[9][1]["box"]
    for n, (r, i, chip, want) in enumerate(out):
        assert (i["status"], i["success"], i["frames_done"]) == (u.CUT, int(r.success), n + 1)
        assert np.array_equal(chip, want), f"update {n + 1}"
        if n + 1 in failed:
            assert i["box"] == good, f"update {n + 1} failed and moved the chip's box"
    assert not np.array_equal(out[10][2], out[9][2]), "the frame changed: so must the chip at the same box"


def test_factor_zero_leaves_the_streams_record_untouched(gpu, oracle, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = gpu.Group(weights_tiny, n_streams=3)
    f0 = _frame(gpu, oracle, sc, 0, "nv12")
    for s in range(3):
        g.init_device(s, f0[0], gpu.BBox.new(*sc.gt_box(0)))
    g.enable_chips(40, u.RGB8)
    g.set_chips(2.0)
    f1 = _frame(gpu, oracle, sc, 1, "nv12")
    g.update_device([f1[0]] * 3)
    chips1, _ = g.read_chips()
    words1 = _info_words(g)
    assert (words1[:, 0] == u.CUT).all() and np.array_equal(chips1[0], chips1[1])
    g.set_chips(0.0, stream=1)
    f2 = _frame(gpu, oracle, sc, 2, "nv12")
    g.update_device([f2[0]] * 3)
    chips2, infos2 = g.read_chips()
    words2 = _info_words(g)
    assert np.array_equal(words2[1], words1[1]) and np.array_equal(chips2[1], chips1[1]), "stream 1 is off"
    for s in (0, 2):
        assert infos2[s]["frames_done"] == 2 and infos2[s]["status"] == u.CUT and not np.array_equal(chips2[s], chips1[s])
    g.close()


# ---- 4. no effect on tracking ------------------------------------------------------------------------------------------------------

def test_a_twin_that_never_enables_tracks_identically(gpu, oracle, weights_tiny):
    import torch
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(3)]
    main, twin = gpu.Group(weights_tiny, n_streams=3), gpu.Group(weights_tiny, n_streams=3)
    fr = [_frame(gpu, oracle, sc, 0, "nv12") for sc in scs]
    for g in (main, twin):
        for s in range(3):
            g.init_device(s, fr[s][0], gpu.BBox.new(*scs[s].gt_box(0)))
    main.enable_chips(64, u.NORM_BF16, *NORMS)
    main.enable_chips(64, u.NORM_BF16, *NORMS)         # the same parameters again: fine
    main.set_chips(2.0, 2, 0)
    caps = main.graph_captures()
    for t in range(6):
        fr = [_frame(gpu, oracle, sc, t, "nv12") for sc in scs]
        frames = [f[0] for f in fr]
        a, b = main.update_device(frames), twin.update_device(frames)
        assert [_res(r) for r in a] == [_res(r) for r in b], f"update {t + 1}"
        for s in range(3):
            assert np.array_equal(_state_words(main, s), _state_words(twin, s)), f"update {t + 1}, stream {s}"
    assert main.graph_captures() == caps, "a graph was captured after the enable"
    # the device view of the store is what read_chips copies
    chips, infos = main.read_chips()
    dc = main.chips_device()
    assert dc.stride == 6 * 64 * 64 and dc.ptr and dc.infos == dc.ptr + 3 * dc.stride
    t_dev = torch.as_tensor(dc, device="cuda")
    assert tuple(t_dev.shape) == (3, 3, 64, 64) and t_dev.data_ptr() == dc.ptr
    assert np.array_equal(t_dev.cpu().numpy().view(np.uint16), chips)
    assert all(i["status"] == u.CUT and i["frames_done"] == 6 for i in infos)
    names = [[f["name"] for f in g.profile_device(frames, iters=1)] for g in (main, twin)]
    assert "target_chips" in names[0] and "target_chips" not in names[1]
    assert [n for n in names[0] if n != "target_chips"] == names[1]
    with pytest.raises(gpu.VtError) as ei:
        twin.read_chips()
    main.close()
    twin.close()


def test_single_tracker_wrappers(gpu, oracle, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    trk = gpu.VitTrack(weights_tiny)
    trk.init(sc.frame_rgb8(0), gpu.BBox.new(*sc.gt_box(0)))
    trk.enable_chips(40, u.RGB8)
    trk.set_chips(2.0)
    for t in range(3):
        rgb = sc.frame_rgb8(t)
        r = trk.update(rgb)
        chips, infos = trk.read_chips()
        assert (infos[0]["status"], infos[0]["frames_done"], infos[0]["box"]) == (u.CUT, t + 1, tuple(r.bbox))
        assert np.array_equal(chips[0], u.chip_u8(u.bilinear(rgb, r.bbox, 2.0, 40))), f"update {t + 1}"
    # a second wrapper of the enabled engine reads too: size and kind come from the engine
    view = trk.as_group()
    vchips, vinfos = view.read_chips()
    assert np.array_equal(vchips, chips) and vinfos == infos
    none, no_infos = view.read_chips([])
    assert none.shape == (0, 40, 40, 3) and no_infos == []
    trk.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_change_nothing(gpu, oracle, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = gpu.Group(weights_tiny, n_streams=2, host_window_margin_pct=0)
    rgb0, rgb1 = sc.frame_rgb8(0), sc.frame_rgb8(1)
    for s in range(2):
        g.init_host(s, rgb0, gpu.BBox.new(*sc.gt_box(0)))
    caps = g.graph_captures()
    nan, inf = float("nan"), float("inf")

    def refused(fn, *a, **k):
        with pytest.raises(gpu.VtError) as ei:
            fn(*a, **k)
        assert ei.value.code == INVALID, (a, k)

    refused(g.set_chips, 2.0)                                       # before the enable
    refused(g.read_chips)
    for size, kind in [(24, 0), (520, 0), (68, 0), (0, 1), (-64, 1), (64, 2), (64, -1)]:
        refused(g.enable_chips, size, kind, *NORMS)
    refused(g.enable_chips, 64, u.NORM_BF16, (1.0, nan, 1.0), (0.0, 0.0, 0.0))
    refused(g.enable_chips, 64, u.NORM_BF16, (1.0, 1.0, 1.0), (0.0, inf, 0.0))
    g.enqueue_host([rgb1, rgb1])
    refused(g.enable_chips, 64, u.RGB8)                             # a pipelined pass is outstanding
    g.wait_next()
    assert g.graph_captures() == caps
    refused(g.set_chips, 2.0)                                       # still not enabled
    g.enable_chips(64, u.RGB8, (nan, nan, nan), (inf, inf, inf))    # the norms are not this kind's
    caps = g.graph_captures()
    g.set_chips(2.0, 3, 1, stream=1)
    g.update_host([rgb1, rgb1])
    chips, _ = g.read_chips()
    words = _info_words(g)
    for size, kind in [(40, u.RGB8), (64, u.NORM_BF16)]:
        refused(g.enable_chips, size, kind, *NORMS)                 # a second enable with other parameters
    g.enable_chips(64, u.RGB8)
    for stream, factor, period, phase in [(2, 2.0, 1, 0), (0, nan, 1, 0), (0, 0.49, 1, 0), (0, 4.01, 1, 0), (0, -1.0, 1, 0),
                                          (0, inf, 1, 0), (1, 2.0, 0, 0), (1, 2.0, -3, 0), (None, 2.0, 4, 4), (None, 2.0, 4, -1),
                                          (0, 2.0, 1000001, 0)]:
        refused(g.set_chips, factor, period, phase, stream=stream)
    refused(lambda: gpu._check(gpu.lib().vt_group_set_chips(g._h, -2, 2.0, 1, 0)))
    g.enqueue_host([rgb1, rgb1])
    refused(g.set_chips, 1.0)
    g.wait_next()
    assert g.graph_captures() == caps
    # the policy is what it was: stream 0 off, stream 1 due when frames_done % 3 == 1 (update 4 is the next)
    st_words = [_state_words(g, s) for s in range(2)]
    assert st_words[0][11] == 3
    g.update_host([rgb1, rgb1])
    w2 = _info_words(g)
    assert np.array_equal(w2[0], words[0]) and not words[0].any()
    assert (w2[1][0], w2[1][1]) == (u.CUT, 4) and (words[1][0], words[1][1]) == (u.NOT_DUE, 2)
    g.close()


def test_enable_under_a_memory_cap_is_refused_and_the_engine_still_tracks(gpu, oracle, weights_tiny):
    """64 tiny streams, C 512 bf16: the store is 64 x 1.5 MiB = 96 MiB. Under the smallest max_device_mib that still
    creates the engine the enable must return VT_ERR_OOM and change nothing: the engine tracks bit-identically to one
    without a cap."""
    B = 64

    def create(mib):
        try:
            return gpu.Group(weights_tiny, n_streams=B, max_device_mib=mib, use_graph=False)
        except gpu.VtError as e:
            assert e.code == OOM
            return None

    lo, hi = 0, 4096                                    # (refused, created]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        g = create(mid)
        if g is None:
            lo = mid
        else:
            g.close()
            hi = mid
    g, free = create(hi), gpu.Group(weights_tiny, n_streams=B, use_graph=False)
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    f0 = _frame(gpu, oracle, sc, 0, "nv12")
    for e in (g, free):
        for s in range(B):
            e.init_device(s, f0[0], gpu.BBox.new(*sc.gt_box(0)))
    with pytest.raises(gpu.VtError) as ei:
        g.enable_chips(512, u.NORM_BF16, *NORMS)
    assert ei.value.code == OOM
    with pytest.raises(gpu.VtError) as ei:
        g.set_chips(2.0)
    assert ei.value.code == INVALID
    f1 = _frame(gpu, oracle, sc, 1, "nv12")
    a, b = g.update_device([f1[0]] * B), free.update_device([f1[0]] * B)
    assert [_res(r) for r in a] == [_res(r) for r in b] and all(r.success for r in a)
    assert np.array_equal(_state_words(g, 5), _state_words(free, 5))
    names = [f["name"] for f in g.profile_device([f1[0]] * B, iters=1)]
    assert "target_chips" not in names
    g.close()
    free.close()
    roomy = gpu.Group(weights_tiny, n_streams=B, max_device_mib=hi + 100, use_graph=False)
    roomy.enable_chips(512, u.NORM_BF16, *NORMS)
    roomy.close()
