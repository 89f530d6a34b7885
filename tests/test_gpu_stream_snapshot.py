"""Stream snapshots on the MI355X: export, import and copy a stream between engines (vt_group_export_stream /
vt_group_import_stream / vt_group_copy_stream, vt_export_state / vt_import_state).

The yardstick is always a TWIN that never exports or imports: an engine that simply kept tracking the same frames.
"Equal" means success, score and bbox bit-identical on every frame, and the "state" and "template" words bit-identical
after every update - no tolerance is chosen anywhere in this file. Both sides always run passes of the same size, the
compared streams in the same slot, because a stream's bits depend on the pass size.

Model tiny_t64_s128 on 640x480 synthetic clips, groups of 3 or 4 streams, 6 to 10 frames per test; one case on the
benchmarked layout (cfg3, engines of 30)."""
import shutil

import numpy as np
import pytest

from test_gpu_stream_subsets import _res
from test_gpu_template_refresh import _tpl

pytestmark = pytest.mark.gpu

W, H = 640, 480
INVALID, FORMAT, NOT_INIT, SHORT, OOM = -1, -4, -6, -7, -8
_DEV, _NV12 = {}, {}


def _clips(gpu, n, first=20):
    """moving squares of different sizes, seeds and paths (the clips of the subset tests)"""
    return [gpu.synth.MovingSquare(W, H, 48 + 4 * (first - 20 + i), seed=first + i) for i in range(n)]


def _nv12(sc, t):
    key = (sc.seed, sc.sq, t)
    if key not in _NV12:
        _NV12[key] = np.ascontiguousarray(sc.frame_nv12(t))
    return _NV12[key]


def _dev(gpu, sc, t):
    """device NV12 frame of clip time t (cached: the twins read the same tensors)"""
    import torch
    key = (sc.seed, sc.sq, t)
    if key not in _DEV:
        _DEV[key] = torch.from_numpy(_nv12(sc, t)).cuda()
    d = _DEV[key]
    return gpu.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H)


def _host(gpu, sc, t):
    return gpu.NV12Frame(_nv12(sc, t), W, H)


def _words(g, s):
    return g.read_tensor("state", s).view(np.uint32).copy()


def _sig(g, s):
    return _words(g, s), _tpl(g, s)


def _same(a, b, tag):
    assert np.array_equal(a[0], b[0]), f"{tag}: state words differ"
    assert np.array_equal(a[1], b[1]), f"{tag}: template words differ"


def _group(gpu, weights, scs, init=None, **kw):
    """a group of len(scs) streams, stream s initialised on clip scs[s] at time 0 (init: the streams to initialise)"""
    g = gpu.Group(weights, n_streams=len(scs), **kw)
    for s in (range(len(scs)) if init is None else init):
        g.init_device(s, _dev(gpu, scs[s], 0), gpu.BBox.new(*scs[s].gt_box(0)))
    return g


def _full(gpu, g, scs, t):
    return g.update_device([_dev(gpu, sc, t) for sc in scs])


def _close(*gs):
    for g in gs:
        g.close()


# ---- 1. checkpoint and resume ---------------------------------------------------------------------------------------------

def test_checkpoint_and_resume_replays_the_same_continuation(gpu, weights_tiny):
    scs, k, m, s = _clips(gpu, 3), 3, 4, 1
    g, twin = _group(gpu, weights_tiny, scs), _group(gpu, weights_tiny, scs)
    for t in range(1, k + 1):
        _full(gpu, g, scs, t), _full(gpu, twin, scs, t)
    before = [_sig(g, b) for b in range(3)]
    blob = g.export_stream(s)
    assert len(blob) == g.snapshot_bytes() == 256 + 24576
    for b in range(3):
        _same(_sig(g, b), before[b], f"export changed stream {b}")
    info = gpu.snapshot_info(blob)
    assert info["frames_done"] == k and info["flags"] == 0 and info["period"] == 0
    assert np.array_equal(gpu.snapshot.parse(blob)["rows"].reshape(-1), (_tpl(g, s) >> 16).astype(np.uint16))
    first = []
    for t in range(k + 1, k + m + 1):
        r, rt = _full(gpu, g, scs, t), _full(gpu, twin, scs, t)
        assert [_res(x) for x in r] == [_res(x) for x in rt]
        _same(_sig(g, s), _sig(twin, s), f"first run, frame {t}")
        first.append((_res(r[s]), _sig(g, s)))
    others = [_sig(g, b) for b in (0, 2)]
    g.import_stream(s, blob)
    _same(_sig(g, s), before[s], "the imported stream is not the exported one")
    for b, o in zip((0, 2), others):
        _same(_sig(g, b), o, f"import disturbed stream {b}")
    for i, t in enumerate(range(k + 1, k + m + 1)):
        r = _full(gpu, g, scs, t)
        assert _res(r[s]) == first[i][0], f"second run, frame {t}: {r[s]}"
        _same(_sig(g, s), first[i][1], f"second run, frame {t}")
    _close(g, twin)


# ---- 2. across engines and slots -------------------------------------------------------------------------------------------

def test_a_stream_moves_to_another_slot_of_another_engine(gpu, weights_tiny):
    ca, cb, k, m = _clips(gpu, 3), _clips(gpu, 3, first=23), 3, 5
    a, twin_a = _group(gpu, weights_tiny, ca), _group(gpu, weights_tiny, ca)
    b, twin_b = _group(gpu, weights_tiny, cb), _group(gpu, weights_tiny, cb)
    for t in range(1, k + 1):
        for g, scs in ((a, ca), (twin_a, ca), (b, cb), (twin_b, cb)):
            _full(gpu, g, scs, t)
    b.import_stream(2, a.export_stream(1))
    _same(_sig(b, 2), _sig(twin_a, 1), "after import")
    mixed = [cb[0], cb[1], ca[1]]
    for t in range(k + 1, k + m + 1):
        ra, rta, rb, rtb = _full(gpu, a, ca, t), _full(gpu, twin_a, ca, t), _full(gpu, b, mixed, t), _full(gpu, twin_b, cb, t)
        assert [_res(x) for x in ra] == [_res(x) for x in rta], f"frame {t}: the source engine left its twin"
        assert _res(rb[2]) == _res(rta[1]), f"frame {t}: imported stream {rb[2]} vs twin {rta[1]}"
        _same(_sig(b, 2), _sig(twin_a, 1), f"frame {t}, imported stream")
        for s in (0, 1):
            assert _res(rb[s]) == _res(rtb[s]), f"frame {t}: stream {s} of the destination was disturbed"
            _same(_sig(b, s), _sig(twin_b, s), f"frame {t}, destination stream {s}")
    assert rb[2].success, "the moved stream lost its target: the comparison shows little"
    _close(a, twin_a, b, twin_b)


# ---- 3. process restart, single tracker -------------------------------------------------------------------------------------

def test_a_tracker_resumes_from_its_exported_state(gpu, weights_tiny):
    sc, k, m = _clips(gpu, 1)[0], 4, 5
    trk, twin = gpu.VitTrack.new(weights_tiny), gpu.VitTrack.new(weights_tiny)
    for v in (trk, twin):
        v.init(_host(gpu, sc, 0), gpu.BBox.new(*sc.gt_box(0)))
    for t in range(1, k + 1):
        assert _res(trk.update(_host(gpu, sc, t))) == _res(twin.update(_host(gpu, sc, t)))
    blob = trk.export_state()
    trk.close()
    again = gpu.VitTrack.new(weights_tiny)
    with pytest.raises(gpu.VtError) as e:
        again.update(_host(gpu, sc, k + 1))
    assert e.value.code == NOT_INIT
    again.import_state(blob)
    _same(_sig(again.as_group(), 0), _sig(twin.as_group(), 0), "after import_state")
    for t in range(k + 1, k + m + 1):
        r, rt = again.update(_host(gpu, sc, t)), twin.update(_host(gpu, sc, t))
        assert _res(r) == _res(rt) and r.success, f"frame {t}: {r} vs twin {rt}"
        _same(_sig(again.as_group(), 0), _sig(twin.as_group(), 0), f"frame {t}")
    again.close()
    twin.close()


# ---- 4. with refresh, odd generation ------------------------------------------------------------------------------------------

def test_a_refreshing_stream_moves_into_an_engine_that_never_enabled_refresh(gpu, weights_tiny):
    ca, cd, k, m = _clips(gpu, 3), _clips(gpu, 3, first=23), 3, 6
    src, twin = _group(gpu, weights_tiny, ca), _group(gpu, weights_tiny, ca)
    dst = _group(gpu, weights_tiny, cd)
    for g in (src, twin):
        g.set_template_refresh(2, 0.0)
    for t in range(1, k + 1):
        _full(gpu, src, ca, t), _full(gpu, twin, ca, t), _full(gpu, dst, cd, t)
    st = src.template_refresh_stats(1)
    assert st["generation"] % 2 == 1, f"the export must happen at an odd generation: {st}"
    blob = src.export_stream(1)
    assert gpu.snapshot_info(blob)["generation"] == st["generation"] and gpu.snapshot_info(blob)["period"] == 2
    assert dst.template_refresh_stats(2)["period"] == 0
    dst.import_stream(2, blob)
    assert dst.template_refresh_stats(2) == st
    assert dst.template_refresh_stats(0)["period"] == 0 and dst.template_refresh_stats(0)["generation"] == 0
    _same(_sig(dst, 2), _sig(twin, 1), "after import")
    mixed, gens = [cd[0], cd[1], ca[1]], []
    for t in range(k + 1, k + m + 1):
        _full(gpu, src, ca, t)
        rt, rd = _full(gpu, twin, ca, t), _full(gpu, dst, mixed, t)
        assert _res(rd[2]) == _res(rt[1]), f"frame {t}: {rd[2]} vs twin {rt[1]}"
        assert dst.template_refresh_stats(2) == twin.template_refresh_stats(1), f"frame {t}"
        _same(_sig(dst, 2), _sig(twin, 1), f"frame {t}")
        gens.append(dst.template_refresh_stats(2)["generation"])
    assert gens[-1] >= st["generation"] + 2, f"no later refresh fired: {gens}"
    assert dst.template_refresh_stats(0)["generation"] == 0, "a stream without a policy refreshed"
    _close(src, twin, dst)


def test_an_import_that_would_enable_refresh_under_a_memory_cap_changes_nothing(gpu, weights_tiny):
    """64 tiny streams: the second template buffers are 1.5 MiB; under the smallest max_device_mib that still creates the
    engine less than 1 MiB is left, so the enabling the snapshot's policy asks for must fail with VT_ERR_OOM. The engines
    replay graphs: an enabling that dropped or recaptured them before it met the cap would show in graph_captures."""
    sc = _clips(gpu, 1)[0]
    src = _group(gpu, weights_tiny, [sc])
    src.set_template_refresh(2, 0.0)
    _full(gpu, src, [sc], 1)
    blob = src.export_stream(0)
    B = 64

    def create(mib):
        try:
            return gpu.Group(weights_tiny, n_streams=B, max_device_mib=mib)
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
    dst = create(hi)
    other = _clips(gpu, 1, first=24)[0]
    for s in range(B):
        dst.init_device(s, _dev(gpu, other, 0), gpu.BBox.new(*other.gt_box(0)))
    dst.update_device([_dev(gpu, other, 1)] * B)
    before, caps, replays = _sig(dst, 5), dst.graph_captures(), int(dst.read_tensor("graph_replays").sum())
    assert caps > 0 and replays == 1, "the destination replays no graph: graph_captures could not show a change"
    with pytest.raises(gpu.VtError) as e:
        dst.import_stream(5, blob)
    assert e.value.code == OOM
    _same(_sig(dst, 5), before, "a refused import")
    assert dst.graph_captures() == caps and dst.template_refresh_stats(5)["period"] == 0
    # and the graphs it had still run: the next full pass replays one and continues stream 5 as a twin's
    twin = gpu.Group(weights_tiny, n_streams=B)
    for s in range(B):
        twin.init_device(s, _dev(gpu, other, 0), gpu.BBox.new(*other.gt_box(0)))
    twin.update_device([_dev(gpu, other, 1)] * B)
    r, rt = dst.update_device([_dev(gpu, other, 2)] * B), twin.update_device([_dev(gpu, other, 2)] * B)
    assert _res(r[5]) == _res(rt[5])
    assert int(dst.read_tensor("graph_replays").sum()) == 2 and dst.graph_captures() == caps
    _same(_sig(dst, 5), _sig(twin, 5), "the pass after the refused import")
    _close(src, dst, twin)


def test_an_odd_generation_survives_a_later_enabling_of_refresh(gpu, weights_tiny):
    """A stream whose refresh was switched off after an odd number of refreshes is exported (period 0, generation odd) and
    imported into an engine that never enabled refresh: the engine keeps its single template buffer. When refresh is
    enabled there later - by a policy on ANOTHER stream - the store grows to two buffers and the stream's rows must be in
    the one its generation names. Template, state and continuation equal the twin's, which did the same without moving."""
    ca, cd, k, m = _clips(gpu, 3), _clips(gpu, 3, first=23), 3, 5
    src, twin, dst = _group(gpu, weights_tiny, ca), _group(gpu, weights_tiny, ca), _group(gpu, weights_tiny, cd)
    for g in (src, twin):
        g.set_template_refresh(2, 0.0, stream=1)
    for t in range(1, k + 1):
        _full(gpu, src, ca, t), _full(gpu, twin, ca, t), _full(gpu, dst, cd, t)
    for g in (src, twin):
        g.set_template_refresh(0, 0.0, stream=1)
    st = src.template_refresh_stats(1)
    assert st["generation"] % 2 == 1 and st["period"] == 0, st
    blob = src.export_stream(1)
    info = gpu.snapshot_info(blob)
    assert info["generation"] == st["generation"] and info["period"] == 0
    caps = dst.graph_captures()
    dst.import_stream(2, blob)
    assert dst.graph_captures() == caps, "a snapshot without a policy enabled refresh"
    _same(_sig(dst, 2), _sig(twin, 1), "after import")
    mixed = [cd[0], cd[1], ca[1]]
    t = k + 1
    rd, rt = _full(gpu, dst, mixed, t), _full(gpu, twin, ca, t)       # one pass on the single buffer
    assert _res(rd[2]) == _res(rt[1])
    _same(_sig(dst, 2), _sig(twin, 1), "single-buffer pass")
    dst.set_template_refresh(2, 0.0, stream=0)                         # the later enabling, on another stream
    assert dst.graph_captures() > caps
    assert np.any(_tpl(dst, 2)), "the imported stream's template reads as zeros after the enabling"
    _same(_sig(dst, 2), _sig(twin, 1), "after the enabling")
    assert dst.export_stream(2)[256:] == twin.export_stream(1)[256:], "the exported rows after the enabling"
    for t in range(k + 2, k + m + 1):
        rd, rt = _full(gpu, dst, mixed, t), _full(gpu, twin, ca, t)
        assert _res(rd[2]) == _res(rt[1]) and rd[2].success, f"frame {t}: {rd[2]} vs twin {rt[1]}"
        _same(_sig(dst, 2), _sig(twin, 1), f"frame {t}")
    # a policy for the stream itself now refreshes into the other buffer, as on the twin
    dst.set_template_refresh(2, 0.0, stream=2)
    twin.set_template_refresh(2, 0.0, stream=1)
    for t in range(k + m + 1, k + m + 4):
        rd, rt = _full(gpu, dst, mixed, t), _full(gpu, twin, ca, t)
        assert _res(rd[2]) == _res(rt[1]), f"frame {t}"
        sd, stw = dst.template_refresh_stats(2), twin.template_refresh_stats(1)
        assert [sd[key] for key in ("period", "generation", "last_frame")] == [stw[key] for key in ("period", "generation", "last_frame")]
        _same(_sig(dst, 2), _sig(twin, 1), f"frame {t}")
    assert dst.template_refresh_stats(2)["generation"] > st["generation"]
    _close(src, twin, dst)


# ---- 5. subset and candidate passes after import ------------------------------------------------------------------------------

def test_the_imported_stream_runs_in_subset_and_candidate_passes(gpu, weights_tiny):
    ca, cb, k = _clips(gpu, 3), _clips(gpu, 3, first=23), 3
    a, b = _group(gpu, weights_tiny, ca), _group(gpu, weights_tiny, cb)     # a keeps tracking: it is the twin
    for t in range(1, k + 1):
        _full(gpu, a, ca, t), _full(gpu, b, cb, t)
    b.import_stream(2, a.export_stream(1))
    # subset passes of two slots, the stream in slot 0 - its own segment of the patch matrix is slot 2
    for t in (k + 1, k + 2):
        rb = b.update_device([_dev(gpu, ca[1], t), _dev(gpu, cb[0], t)], streams=[2, 0])
        ra = a.update_device([_dev(gpu, ca[1], t), _dev(gpu, ca[0], t)], streams=[1, 0])
        assert _res(rb[0]) == _res(ra[0]), f"subset pass, frame {t}: {rb[0]} vs twin {ra[0]}"
        _same(_sig(b, 2), _sig(a, 1), f"subset pass, frame {t}")
    # a candidate list with two boxes for the stream: its own and one a quarter of a window off
    t = k + 3
    own = a.read_state(1)["box"]
    off = (float(own[0]) + 40.0, float(own[1]) - 24.0, float(own[2]), float(own[3]))
    f = _dev(gpu, ca[1], t)
    rb, wb = b.update_device_candidates([(2, None), (2, off)], [f, f])
    ra, wa = a.update_device_candidates([(1, None), (1, off)], [f, f])
    assert [_res(x) for x in rb] == [_res(x) for x in ra] and wb == wa
    _same(_sig(b, 2), _sig(a, 1), "candidate pass")
    # and a full pass behind them
    rb, ra = _full(gpu, b, [cb[0], cb[1], ca[1]], t + 1), _full(gpu, a, ca, t + 1)
    assert _res(rb[2]) == _res(ra[1])
    _same(_sig(b, 2), _sig(a, 1), "full pass behind the candidate pass")
    _close(a, b)


# ---- 6. vt_group_copy_stream ---------------------------------------------------------------------------------------------------

def test_copy_stream_equals_the_byte_path_and_copies_within_an_engine(gpu, weights_tiny):
    ca, cb, k, m = _clips(gpu, 3), _clips(gpu, 3, first=23), 3, 4
    a = _group(gpu, weights_tiny, ca)
    by_bytes, by_copy = _group(gpu, weights_tiny, cb), _group(gpu, weights_tiny, cb)
    a.set_template_refresh(2, 0.0, stream=1)        # the copy carries policy and the second buffer too
    for t in range(1, k + 1):
        _full(gpu, a, ca, t), _full(gpu, by_bytes, cb, t), _full(gpu, by_copy, cb, t)
    before = [_sig(a, s) for s in range(3)]
    by_bytes.import_stream(2, a.export_stream(1))
    a.copy_stream(1, by_copy, 2)
    for s in range(3):
        _same(_sig(a, s), before[s], f"copy changed source stream {s}")
    _same(_sig(by_copy, 2), _sig(by_bytes, 2), "after the copy")
    assert by_copy.template_refresh_stats(2) == by_bytes.template_refresh_stats(2) == a.template_refresh_stats(1)
    mixed = [cb[0], cb[1], ca[1]]
    for t in range(k + 1, k + m + 1):
        r1, r2 = _full(gpu, by_bytes, mixed, t), _full(gpu, by_copy, mixed, t)
        assert [_res(x) for x in r1] == [_res(x) for x in r2], f"frame {t}"
        for s in range(3):
            _same(_sig(by_copy, s), _sig(by_bytes, s), f"frame {t}, stream {s}")
    # within one engine: stream 1 into slot 0, then both on the same frames
    with pytest.raises(gpu.VtError) as e:
        a.copy_stream(1, a, 1)
    assert e.value.code == INVALID
    a.copy_stream(1, a, 0)
    _same(_sig(a, 0), _sig(a, 1), "copy within the engine")
    assert a.template_refresh_stats(0) == a.template_refresh_stats(1)
    for t in range(k + 1, k + m + 1):
        r = _full(gpu, a, [ca[1], ca[1], ca[2]], t)
        assert _res(r[0]) == _res(r[1]) and r[0].success, f"frame {t}: {r[0]} vs {r[1]}"
        _same(_sig(a, 0), _sig(a, 1), f"frame {t}, the two copies")
    _close(a, by_bytes, by_copy)


def test_copy_stream_across_two_gpus(gpu, weights_tiny):
    if gpu.device_count() < 2:
        pytest.skip("one gfx950 device visible: a copy between GPUs needs two")
    import torch
    ca, k, m = _clips(gpu, 3), 3, 4
    a = _group(gpu, weights_tiny, ca)
    far = gpu.Group(weights_tiny, n_streams=3, device=1)
    for t in range(1, k + 1):
        _full(gpu, a, ca, t)
    a.copy_stream(1, far, 2)
    _same(_sig(far, 2), _sig(a, 1), "after the copy")
    for t in range(k + 1, k + m + 1):
        d = torch.from_numpy(_nv12(ca[1], t)).to("cuda:1")
        f = gpu.frame_nv12(d.data_ptr(), d.data_ptr() + W * H, W, H)
        rf = far.update_device([f], streams=[2])
        ra = a.update_device([_dev(gpu, ca[1], t)], streams=[1])
        assert _res(rf[0]) == _res(ra[0]), f"frame {t}"
        _same(_sig(far, 2), _sig(a, 1), f"frame {t}")
    _close(a, far)


# ---- 7. pipelined ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("margin_pct,expect_redo", [(0, False), (-1, True)])
def test_import_behind_two_outstanding_passes(gpu, weights_tiny, margin_pct, expect_redo):
    """pipe: streams 0, 1, 2 track, stream 3 is empty. While passes 1 and 2 over [0, 1, 2] are outstanding a snapshot of
    src's stream 1 is imported into stream 3; from pass 3 on the list is [0, 1, 3]. The twins are synchronous: `sync` for
    streams 0 and 1 (same lists, its stream 3 is a stand-in that keeps the pass size), `src` itself for the imported
    stream (its stream 1 in slot 2 of passes of three). With the enlargement off the moving targets leave their
    speculative windows: pass 2 is redone behind the import, and pass 3 with it - stream 3 rewound to the imported state."""
    cs, k, n = _clips(gpu, 4), 3, 9

    def hf(s, t):           # every fifth clip frame: up to 15 px per pass, well outside an exact window's 4 px of slack
        return _host(gpu, cs[s], 5 * t)

    src = gpu.Group(weights_tiny, n_streams=3)
    for s in range(3):
        src.init_host(s, hf(s, 0), gpu.BBox.new(*cs[s].gt_box(0)))
    for t in range(1, k + 1):
        src.update_host([hf(s, t) for s in range(3)])
    blob = src.export_stream(1)
    pipe = gpu.Group(weights_tiny, n_streams=4, host_window_margin_pct=margin_pct)
    sync = gpu.Group(weights_tiny, n_streams=4)
    for g in (pipe, sync):
        for s in (0, 1, 2):
            g.init_host(s, hf(s, 0), gpu.BBox.new(*cs[s].gt_box(0)))
    sync.init_host(3, hf(3, 0), gpu.BBox.new(*cs[3].gt_box(0)))
    caps = pipe.graph_captures()

    def lists(t):
        return [0, 1, 2] if t <= 2 else [0, 1, 3]

    def frames(t):          # the imported stream continues src's clip at src's clock
        return [hf(0, t), hf(1, t), hf(2, t) if t <= 2 else hf(1, k + t - 2)]

    got = {}
    pipe.enqueue_host(frames(1), streams=lists(1))
    pipe.enqueue_host(frames(2), streams=lists(2))
    with pytest.raises(gpu.VtError) as e:
        pipe.import_stream(0, blob)                 # in both outstanding passes
    assert e.value.code == INVALID
    pipe.import_stream(3, blob)                     # in neither: queued behind them
    for t in range(3, n + 1):
        got[t - 2] = pipe.wait_next()
        pipe.enqueue_host(frames(t), streams=lists(t))
    got[n - 1], got[n] = pipe.wait_next(), pipe.wait_next()
    for t in range(1, n + 1):
        want = sync.update_host(frames(t), streams=lists(t))
        for i in (0, 1):
            assert _res(got[t][i]) == _res(want[i]), f"pass {t}, stream {i}: {got[t][i]} vs twin {want[i]}"
        if t <= 2:
            assert _res(got[t][2]) == _res(want[2]), f"pass {t}, stream 2"
        else:
            u = k + t - 2
            ws = src.update_host([hf(0, u), hf(2, u), hf(1, u)], streams=[0, 2, 1])
            assert _res(got[t][2]) == _res(ws[2]), f"pass {t}, imported stream: {got[t][2]} vs twin {ws[2]}"
    _same(_sig(pipe, 3), _sig(src, 1), "imported stream at the end")
    for s in (0, 1, 2):
        _same(_sig(pipe, s), _sig(sync, s), f"stream {s} at the end")
    assert got[n][2].success
    assert (pipe.host_redos() > 0) == expect_redo, pipe.host_redos()
    assert sync.host_redos() == 0 and pipe.graph_captures() == caps
    _close(src, pipe, sync)


def test_export_beside_outstanding_passes_leaves_their_results_alone(gpu, weights_tiny):
    cs = _clips(gpu, 3)
    pipe, sync = gpu.Group(weights_tiny, n_streams=3), gpu.Group(weights_tiny, n_streams=3)
    for g in (pipe, sync):
        for s in range(3):
            g.init_host(s, _host(gpu, cs[s], 0), gpu.BBox.new(*cs[s].gt_box(0)))
    ref = sync.export_stream(2)
    for t in (1, 2):
        pipe.enqueue_host([_host(gpu, cs[0], t), _host(gpu, cs[1], t)], streams=[0, 1])
    with pytest.raises(gpu.VtError) as e:
        pipe.export_stream(1)
    assert e.value.code == INVALID
    assert pipe.export_stream(2) == ref             # in no outstanding pass: the init state, byte for byte
    for t in (1, 2):
        got = pipe.wait_next()
        want = sync.update_host([_host(gpu, cs[0], t), _host(gpu, cs[1], t)], streams=[0, 1])
        assert [_res(x) for x in got] == [_res(x) for x in want], f"pass {t}"
    _close(pipe, sync)


# ---- 8. refusals with nothing changed --------------------------------------------------------------------------------------------

def test_refusals_leave_the_destination_as_it_was(gpu, weights_tiny, weights_cfg2):
    import ctypes
    cs = _clips(gpu, 3)
    g = _group(gpu, weights_tiny, cs, init=[0, 1])
    g.update_device([_dev(gpu, cs[0], 1), _dev(gpu, cs[1], 1)], streams=[0, 1])
    before = [_sig(g, s) for s in range(3)]
    L, n = gpu.lib(), ctypes.c_size_t(0)
    buf = ctypes.create_string_buffer(g.snapshot_bytes())
    assert L.vt_group_export_stream(g._h, 2, buf, len(buf), ctypes.byref(n)) == NOT_INIT
    n.value = 0
    assert L.vt_group_export_stream(g._h, 1, buf, len(buf) - 1, ctypes.byref(n)) == SHORT and n.value == len(buf)
    assert L.vt_group_export_stream(g._h, 1, None, 0, ctypes.byref(n)) == SHORT and n.value == len(buf)
    assert L.vt_group_export_stream(g._h, 3, buf, len(buf), ctypes.byref(n)) == INVALID
    assert L.vt_group_export_stream(g._h, -1, buf, len(buf), ctypes.byref(n)) == INVALID
    blob = g.export_stream(1)
    for bad in (3, -1):
        assert L.vt_group_import_stream(g._h, bad, blob, len(blob)) == INVALID
    assert L.vt_group_import_stream(g._h, 0, None, len(blob)) == INVALID
    broken = bytearray(blob)
    broken[gpu.snapshot.ROWS_OFF + 99] ^= 0x10
    assert L.vt_group_import_stream(g._h, 0, bytes(broken), len(broken)) == FORMAT
    assert L.vt_group_import_stream(g._h, 0, blob, len(blob) - 2) == FORMAT
    for s in range(3):
        _same(_sig(g, s), before[s], f"tiny engine, stream {s}")
    # a tiny snapshot into an engine of another input geometry
    big = gpu.Group(weights_cfg2, n_streams=1)
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    big.init_device(0, _dev(gpu, sc, 0), gpu.BBox.new(*sc.gt_box(0)))
    was = _sig(big, 0)
    with pytest.raises(gpu.VtError) as e:
        big.import_stream(0, blob)
    assert e.value.code == FORMAT and "geometry" in str(e.value)
    with pytest.raises(gpu.VtError) as e:
        g.copy_stream(1, big, 0)
    assert e.value.code == FORMAT
    _same(_sig(big, 0), was, "cfg2 engine")
    _close(g, big)


# ---- 9. another checkpoint, same geometry ---------------------------------------------------------------------------------------

def test_import_into_an_engine_that_runs_another_checkpoint(gpu, weights_tiny, tmp_path):
    other = str(tmp_path / "tiny_lo10.vtwb")
    shutil.copyfile(weights_tiny, other)
    gpu.weights.set_lo_shift(other, 10)
    cs = _clips(gpu, 3)
    a = _group(gpu, weights_tiny, cs)
    for t in (1, 2, 3):
        _full(gpu, a, cs, t)
    b = gpu.Group(other, n_streams=3)
    b.import_stream(0, a.export_stream(1))
    _same(_sig(b, 0), _sig(a, 1), "after import")
    r = b.update_device([_dev(gpu, cs[1], 4)], streams=[0])      # returns VT_OK (anything else raises)
    assert b.read_state(0)["frames_done"] == a.read_state(1)["frames_done"] + 1 and len(r) == 1
    _close(a, b)


# ---- 10. nothing for engines that do not use it ----------------------------------------------------------------------------------

def test_export_and_a_plain_import_capture_no_graph(gpu, weights_tiny):
    cs = _clips(gpu, 3)
    a, b = _group(gpu, weights_tiny, cs), _group(gpu, weights_tiny, cs)
    _full(gpu, a, cs, 1)
    ca, cb = a.graph_captures(), b.graph_captures()
    assert ca > 0
    blob = a.export_stream(1)
    assert gpu.snapshot_info(blob)["flags"] == 0
    assert a.graph_captures() == ca
    b.import_stream(2, blob)
    assert b.graph_captures() == cb
    # flag bit 0 is an init on such a format: the second set of graphs, once, inside the import
    flagged = bytearray(blob)
    flagged[28] |= 1
    b.import_stream(2, gpu.snapshot.restamp(bytes(flagged)))
    assert b.graph_captures() == 2 * cb
    b.import_stream(1, gpu.snapshot.restamp(bytes(flagged)))
    assert b.graph_captures() == 2 * cb
    assert gpu.snapshot_info(b.export_stream(1))["flags"] == 1
    _close(a, b)


# ---- 11. the benchmarked layout ------------------------------------------------------------------------------------------------

def test_copy_between_two_engines_of_thirty_at_cfg3(gpu, weights_cfg3):
    """stream 7 of engine A tracks clip x, everything else clip y; A's stream 7 is copied into stream 0 of engine B, which
    then follows clip x there exactly as stream 7 of a twin of A does"""
    B = 30
    x, y = gpu.synth.MovingSquare(W, H, 80, seed=9), gpu.synth.MovingSquare(W, H, 64, seed=0)
    of_a = [x if s == 7 else y for s in range(B)]
    a, twin, b = (_group(gpu, weights_cfg3, of_a), _group(gpu, weights_cfg3, of_a), _group(gpu, weights_cfg3, [y] * B))
    for g, scs in ((a, of_a), (twin, of_a), (b, [y] * B)):
        _full(gpu, g, scs, 1)
    assert b.snapshot_bytes() == 256 + 221184
    a.copy_stream(7, b, 0)
    _same(_sig(b, 0), _sig(twin, 7), "after the copy")
    for t in (2, 3, 4):
        rb, rt = _full(gpu, b, [x] + [y] * (B - 1), t), _full(gpu, twin, of_a, t)
        assert _res(rb[0]) == _res(rt[7]), f"frame {t}: {rb[0]} vs twin {rt[7]}"
        assert _res(rb[1]) != _res(rb[0]), "the two clips give the same results: the comparison shows nothing"
        _same(_sig(b, 0), _sig(twin, 7), f"frame {t}")
    _close(a, twin, b)
