"""Response peaks (vt_group_set_peaks / vt_group_last_peaks; DESIGN.md section 3, "Response peaks"), on the MI355X.

Operator level, through vt_op_response_peaks (the launch alone) on the case sets of tests/peaks_util.py at du.SHAPES: the
specification is vto_decode iterated (peaks_util.iterate_oracle). Cells, n and the record's other integers are exact
everywhere; score, response and box are held to du.sweep(grid, C).tol, the shape's existing bar (the sets keep device expf
out of every decision: tests/test_response_peaks_cases.py), NaNs where and only where the specification has them. Peak 0 is
held to the BITS of what the decode (vt_op_head_decode, form 0) writes for the same operands.

Engine level, tiny model: after every update each slot's record is bit-identical to the hook run on that pass's own logits,
window, states and policy - no tolerance - and peak 0 to the slot's vt_result.score and the state's last_fbox / last_idx.
A stream's bits depend on the size of the pass it runs in (tests/test_gpu_stream_subsets.py), so the pass kinds are
compared at one pass size.

The launch has no result pointer, so "the results come back unchanged" is checked at engine level (the twin)."""
import ctypes

import numpy as np
import pytest

import decode_util as du
import peaks_util as pu
from test_gpu_pixel_formats import _res

pytestmark = pytest.mark.gpu

W, H = 640, 480
INVALID = -1
FILL = 0xA5A5A5A5


def _op(gpu, s, K, R=None, min_resp=None, **kw):
    return gpu.op_response_peaks(s.head_out(), s.hann, s.states, (K, s.R if R is None else R, s.min_resp if min_resp is None else min_resp),
                                 s.n, s.grid, **kw)


def _compare(rec, want, K, R, tol, states, tag, streams=None):
    """records [n] against the reference lists `want` (peaks_util.iterate) truncated to K"""
    n = np.minimum(want["n"], K)
    assert np.array_equal(rec["n"], n), f"{tag}: n {rec['n'][rec['n'] != n][:8]} != {n[rec['n'] != n][:8]}"
    assert np.array_equal(rec["stream"], np.arange(len(rec)) if streams is None else streams), f"{tag}: stream"
    assert np.array_equal(rec["frames_done"], states["frames_done"]) and np.all(rec["radius"] == R), f"{tag}: header"
    worst = 0.0
    for k in range(pu.KMAX):
        on = n > k
        p = rec["peak"][:, k]
        off = p[~on].view(np.uint32)
        assert not off.any(), f"{tag}: words behind the list are not zero (peak {k})"
        if not on.any():
            continue
        assert np.array_equal(p["cell"][on], want["cell"][on, k]), f"{tag}: cells of peak {k}"
        assert not p["reserved"][on].any()
        for name, got, ref in (("score", p["score"][on], want["score"][on, k]), ("resp", p["resp"][on], want["resp"][on, k]),
                               ("box", p["box"][on], want["fbox"][on, k])):
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan), f"{tag}: NaNs of {name}, peak {k}"
            if (~nan).any():
                d = float(np.abs(got[~nan].astype(np.float64) - ref[~nan].astype(np.float64)).max())
                worst = max(worst, d)
                assert d <= tol, f"{tag}: {name} of peak {k} off by {d:.3e} (bar {tol:.3e})"
    return worst


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_planted_maxima(gpu, grid, C, capsys):
    """five planted maxima, R = 1..4, K = 1, 3, 8; peak 0 against the decode's bits; mirror = device records"""
    worst = 0.0
    for R in (1, 2, 3, 4):
        s = pu.planted(grid, C, R)
        c = du.Cases(grid, C, s.logits, s.hann, s.states, 0.5, tol=s.tol)
        t, w4, b4 = c.operands()
        dec = gpu.op_head_decode(t, w4, b4, s.hann, s.states, s.n, grid, form=0)
        assert du.same_logits(dec["head_out"][:, :5], s.logits.reshape(-1, 5))
        for K in (1, 3, 8):
            out = gpu.op_response_peaks(dec["head_out"], s.hann, dec["states"], (K, R, s.min_resp), s.n, grid)
            rec = out["records"]
            assert out["host_records"].tobytes() == rec.tobytes(), "pinned mirror != device records"
            assert out["states"].tobytes() == dec["states"].tobytes(), "the launch wrote a state"
            worst = max(worst, _compare(rec, s.ora, K, R, s.tol, dec["states"], f"planted grid {grid} R {R} K {K}"))
            p0 = rec["peak"][:, 0]
            assert np.array_equal(p0["score"].view(np.uint32), dec["results"]["score"].view(np.uint32)), "peak 0 score != vt_result.score"
            assert np.array_equal(p0["box"].view(np.uint32), dec["states"]["last_fbox"].view(np.uint32)), "peak 0 box != last_fbox"
            assert np.array_equal(p0["cell"], dec["states"]["last_idx"]), "peak 0 cell != last_idx"
            assert np.array_equal(p0["score"].view(np.uint32), dec["states"]["last_score"].view(np.uint32))
    with capsys.disabled():
        print(f"\n[planted, grid {grid}] largest |device - specification| {worst:.3e}, bar {du.sweep(grid, C).tol:.3e}")


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_border_geometry_and_distances(gpu, grid, C, capsys):
    """every cell as peak 0 with a second maximum R + 1 away (squares cut by edges and corners, windows of 4 and 6 cells,
    windows beside a suppressed square); two maxima R and R + 1 apart; the NaN offset on a suppressed window cell"""
    worst = 0.0
    for R in (1, 2, 3, 4):
        b = pu.border(grid, C, R)
        out = _op(gpu, b, b.K)
        assert out["host_records"].tobytes() == out["records"].tobytes()
        worst = max(worst, _compare(out["records"], b.ora, b.K, R, b.tol, b.states, f"border grid {grid} R {R}"))
        if R + 1 < grid:
            a = pu.apart(grid, C, R)
            rec = _op(gpu, a, a.K)["records"]
            worst = max(worst, _compare(rec, a.ora, a.K, R, a.tol, a.states, f"apart grid {grid} R {R}"))
            assert rec["n"].tolist() == [1, 2, 2]
            # the NaN x-offset of the suppressed cell reaches peak 1's x and nothing else, as in the specification
            assert rec["peak"][2, 1]["box"][0] == 0.0 and rec["peak"][2, 1]["box"][2] == 10.0
            assert np.array_equal(rec["peak"][2, 1]["box"][[1, 3]].view(np.uint32), rec["peak"][1, 1]["box"][[1, 3]].view(np.uint32))
    with capsys.disabled():
        print(f"\n[border, grid {grid}] largest |device - specification| {worst:.3e}, bar {du.sweep(grid, C).tol:.3e}")


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_exact_sets(gpu, grid, C):
    """ties and the order of the list, the flat map, min_resp exactly at a response and one float above, all-NaN maps,
    +-inf logits"""
    t = pu.tie_order(grid, C)
    _compare(_op(gpu, t, t.K)["records"], t.ora, t.K, t.R, t.tol, t.states, f"ties grid {grid}")
    for R in (1, 2, 4):
        f = pu.flat(grid, C, R)
        rec = _op(gpu, f, f.K)["records"]
        want = pu.flat_expected(grid, R)
        assert rec["n"][0] == len(want) and rec["peak"][0]["cell"][:len(want)].tolist() == want, (grid, R)
        assert np.all(rec["peak"][0]["resp"][:len(want)] == np.float32(0.5)) and np.all(rec["peak"][0]["score"][:len(want)] == np.float32(0.5))
        _compare(rec, f.ora, f.K, R, f.tol, f.states, f"flat grid {grid} R {R}")
    for thr, n in ((0.5, 2), (pu.THR_ABOVE_HALF, 1)):
        m = pu.at_min_resp(grid, C, thr)
        rec = _op(gpu, m, m.K)["records"]
        assert rec["n"].tolist() == [n, n], f"min_resp {thr!r}"
        _compare(rec, m.ora, m.K, m.R, m.tol, m.states, f"min_resp grid {grid}")
        if n == 2:
            assert np.all(rec["peak"][:, 1]["resp"] == np.float32(0.5))
    nf = pu.nonfinite(grid, C)
    rec = _op(gpu, nf, nf.K)["records"]
    _compare(rec, nf.ora, nf.K, nf.R, nf.tol, nf.states, f"nonfinite grid {grid}")
    k = nf.names.index("all nan")
    p = rec["peak"][k, 0]
    assert rec["n"][k] == 1 and p["cell"] == 0 and np.isnan(p["score"]) and np.isnan(p["resp"]) and p["box"].tolist() == [0.0, 0.0, 10.0, 10.0]
    k = nf.names.index("all -inf")
    assert rec["n"][k] == 1 and rec["peak"][k, 0]["cell"] == 0 and rec["peak"][k, 0]["score"] == 0.0


def test_gates_subset_map_and_untouched_words(gpu):
    """K = 0 streams and losing candidate slots write n = 0 and nothing else; a subset map puts `stream` right and reads the
    mapped stream's geometry and policy; the mirror equals the device records; the states come back bit-unchanged"""
    grid, C, R = 13, 64, 2
    s = pu.planted(grid, C, R)
    B = 12
    ho = s.head_out()[:B * s.ns]
    # slot i works for stream smap[i] of 20 states; slot 3 is silent because its stream (7) has the policy off; slot 5
    # loses a candidate pass to slot 4 and slot 8 to slot 9 (winner[i] != i)
    smap = np.array([4, 19, 0, 7, 11, 3, 8, 15, 2, 9, 13, 1], np.int32)
    states = du.make_states(*du.draw_geometry(20, np.random.default_rng(11)), 12)
    pol = np.zeros(20, gpu.PEAKS_POLICY_DTYPE)
    pol["max_peaks"], pol["radius"], pol["min_resp"] = 8, R, s.min_resp
    pol["max_peaks"][7] = 0
    pol["max_peaks"][11], pol["radius"][11] = 2, 1
    winner = np.arange(B, dtype=np.int32)
    winner[5] = 4
    winner[8] = 9
    out = gpu.op_response_peaks(ho, s.hann, states, pol, B, grid, slot_stream=smap, winner=winner)
    rec, words = out["records"], out["records"].view(np.uint32).reshape(B, 68)
    assert out["host_records"].tobytes() == rec.tobytes()
    assert out["states"].tobytes() == states.tobytes()
    for b in (3, 5, 8):
        assert words[b, 0] == 0 and np.all(words[b, 1:] == FILL), f"slot {b} lists nothing: n = 0 and no other word"
    on = np.array([b for b in range(B) if b not in (3, 5, 8)])
    plain = on[smap[on] != 11]
    want = pu.iterate_oracle(s.logits[plain], s.hann, grid, states["geo"][smap[plain]], states["frame_w"][smap[plain]],
                             states["frame_h"][smap[plain]], 8, R, s.min_resp)
    _compare(rec[plain], want, 8, R, s.tol, states[smap[plain]], "subset map", streams=smap[plain])
    b = int(np.flatnonzero(smap == 11)[0])
    want = pu.iterate_oracle(s.logits[b:b + 1], s.hann, grid, states["geo"][[11]], states["frame_w"][[11]], states["frame_h"][[11]],
                             2, 1, s.min_resp)
    _compare(rec[b:b + 1], want, 2, 1, s.tol, states[[11]], "stream 11's own policy", streams=[11])
    # bad operands are refused before anything runs
    bad = pol.copy()
    bad["max_peaks"][0] = 9
    with pytest.raises(gpu.VtError):
        gpu.op_response_peaks(ho, s.hann, states, bad, B, grid, slot_stream=smap)
    bad = pol.copy()
    bad["radius"][0] = 5
    with pytest.raises(gpu.VtError):
        gpu.op_response_peaks(ho, s.hann, states, bad, B, grid, slot_stream=smap)
    with pytest.raises(gpu.VtError):
        gpu.op_response_peaks(ho, s.hann, states, pol, B, grid, slot_stream=np.full(B, 20, np.int32))


# ---- engine level -------------------------------------------------------------------------------------------------------------

def _hann(gpu, weights):
    return np.ascontiguousarray(gpu.weights.parse_blob(open(weights, "rb").read())[1]["hann"], np.float32).reshape(-1)


def _states(g):
    from gstreamer_vit_tracker_amd.snapshot import STATE
    return np.concatenate([g.read_tensor("state", s).view(np.uint8).view(STATE) for s in range(g.streams)])


def _policies(gpu, B, pols):
    """pols: {stream: (K, R, min_resp)}; streams not named are off (as set_peaks leaves them: zero records)"""
    p = np.zeros(B, gpu.PEAKS_POLICY_DTYPE)
    p["radius"] = 1         # the hook refuses radius 0 even where the policy is off
    for s, (K, R, m) in pols.items():
        p[s] = (K, R, m, 0)
    return p


def _apply(g, pols):
    for s, (K, R, m) in pols.items():
        g.set_peaks(K, R, m, stream=s)


def _words(rec):
    return np.ascontiguousarray(rec).view(np.uint32).reshape(len(rec), 68)


def _check_pass(gpu, g, hann, streams, pols, results, tag, winner=None):
    """the records of the pass just collected against the hook on the pass's own inputs (bit for bit) and peak 0 against
    the pass's results and states; -> the records"""
    n, grid = len(streams), g.model_info().score_grid
    rec = g.last_peaks(n)
    ho = np.concatenate([g.read_tensor("slot.head_out", i).reshape(-1, 8) for i in range(n)])
    st = _states(g)
    hook = gpu.op_response_peaks(ho, hann, st, _policies(gpu, g.streams, pols), n, grid, slot_stream=np.asarray(streams, np.int32),
                                 winner=None if winner is None else np.asarray(winner, np.int32))["records"]
    for i, s in enumerate(streams):
        lists = s in pols and pols[s][0] > 0 and (winner is None or winner[i] == i)
        if not lists:
            assert rec["n"][i] == 0 == hook["n"][i], f"{tag}: slot {i} lists nothing"
            continue
        assert rec[i].tobytes() == hook[i].tobytes(), f"{tag}: slot {i} (stream {s}) differs from the hook\n{rec[i]}\n{hook[i]}"
        assert 1 <= rec["n"][i] <= pols[s][0] and rec["stream"][i] == s and rec["radius"][i] == pols[s][1]
        assert rec["frames_done"][i] == st["frames_done"][s]
        p0 = rec["peak"][i, 0]
        assert p0["score"].view(np.uint32) == np.float32(results[i].score).view(np.uint32), f"{tag}: peak 0 score != vt_result.score"
        assert np.array_equal(p0["box"].view(np.uint32), st["last_fbox"][s].view(np.uint32)), f"{tag}: peak 0 box != last_fbox"
        assert p0["cell"] == st["last_idx"][s], f"{tag}: peak 0 cell != last_idx"
        r = rec["peak"][i]["resp"][:rec["n"][i]]
        assert np.all(r[1:] <= r[:-1]) and np.all(r[1:] >= np.float32(pols[s][2])) and np.all(r[1:] > 0), f"{tag}: responses {r}"
    return rec


def _dev(gpu, arrays):
    import torch
    keep = [torch.from_numpy(a).cuda() for a in arrays]
    return [gpu.frame_rgb8(d.data_ptr(), W, H) for d in keep], keep


POLS3 = {0: (8, 2, 0.0), 1: (3, 1, 0.02), 2: (5, 4, 0.0)}


def test_engine_records_equal_the_hook_on_every_pass(gpu, weights_tiny):
    """three streams, a dozen frames, full and subset passes on device frames; one stream switched off and on again"""
    hann = _hann(gpu, weights_tiny)
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(3)]
    g = gpu.Group(weights_tiny, n_streams=3)
    fr, keep = _dev(gpu, [sc.frame_rgb8(0) for sc in scs])
    for s in range(3):
        g.init_device(s, fr[s], gpu.BBox.new(*scs[s].gt_box(0)))
    with pytest.raises(gpu.VtError):
        g.last_peaks()
    _apply(g, POLS3)
    caps = g.graph_captures()
    pols = dict(POLS3)
    deep = 0
    for t in range(12):
        fr, keep = _dev(gpu, [sc.frame_rgb8(t) for sc in scs])
        if t % 4 == 3:
            lst = [2, 0]
            res = g.update_device([fr[2], fr[0]], streams=lst)
        else:
            lst = [0, 1, 2]
            res = g.update_device(fr)
        rec = _check_pass(gpu, g, hann, lst, pols, res, f"frame {t}")
        deep += int(rec["n"].max() >= 3)
        if t == 5:
            g.set_peaks(0, stream=1)
            pols.pop(1)
        if t == 8:
            g.set_peaks(2, 3, 0.5, stream=1)
            pols[1] = (2, 3, 0.5)
    assert deep >= 6, "the lists stay short: the comparison shows little"
    assert g.graph_captures() == caps, "a graph was captured after the enable"
    assert len(g.last_peaks(2)) == 2 and len(g.last_peaks()) == 3
    g.close()


def _masked(rec):
    """record words without the `stream` word (engines of another size number their streams differently)"""
    w = _words(rec).copy()
    w[:, 1] = 0
    return w


def test_every_kind_of_pass_writes_the_same_records(gpu, weights_tiny):
    """two clips at pass size two: full device passes, device and pipelined host passes over the permuted list [2, 0] of a
    three-stream engine, synchronous host passes, pipelined host passes with the default margin and with margin -1
    (speculative windows miss, passes are redone), and a run that moves both streams to a second engine half-way"""
    hann = _hann(gpu, weights_tiny)
    N = 12
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in (1, 2)]
    rgb = [[sc.frame_rgb8(2 * i) for sc in scs] for i in range(N)]
    pol = [(8, 2, 0.0), (4, 1, 0.05)]

    def setup(g, smap=(0, 1), host=False, init=True):
        for j, s in enumerate(smap):
            if init:
                box = gpu.BBox.new(*scs[j].gt_box(0))
                if host:
                    g.init_host(s, rgb[0][j], box)
                else:
                    fr, keep = _dev(gpu, [rgb[0][j]])
                    g.init_device(s, fr[0], box)
            g.set_peaks(*pol[j], stream=s)

    full = gpu.Group(weights_tiny, n_streams=2)
    setup(full)
    want_res, want = [], []
    for i in range(N):
        fr, keep = _dev(gpu, rgb[i])
        res = full.update_device(fr)
        want_res.append([_res(r) for r in res])
        want.append(_masked(_check_pass(gpu, full, hann, [0, 1], {0: pol[0], 1: pol[1]}, res, f"full pass, frame {i}")))
    assert all(w[0, 0] >= 2 for w in want), "stream 0 lists one peak only"
    full.close()

    def same(g, i, tag, streams=(0, 1)):
        rec = g.last_peaks(2)
        assert rec["stream"].tolist() == list(streams), tag
        assert np.array_equal(_masked(rec), want[i]), f"{tag}, frame {i}: records differ\n{rec}"

    sub = gpu.Group(weights_tiny, n_streams=3)
    setup(sub, smap=(2, 0))
    for i in range(N):
        fr, keep = _dev(gpu, rgb[i])
        assert [_res(r) for r in sub.update_device(fr, streams=[2, 0])] == want_res[i], f"subset pass, frame {i}"
        same(sub, i, "subset pass", (2, 0))
    sub.close()

    sync = gpu.Group(weights_tiny, n_streams=2)
    setup(sync, host=True)
    for i in range(N):
        assert [_res(r) for r in sync.update_host(rgb[i])] == want_res[i], f"host pass, frame {i}"
        same(sync, i, "host pass")
    sync.close()

    for margin in (0, -1):
        for smap, B in (((0, 1), 2), ((2, 0), 3)):
            pipe = gpu.Group(weights_tiny, n_streams=B, host_window_margin_pct=margin)
            setup(pipe, smap=smap, host=True)
            lst = None if B == 2 else list(smap)
            tag = f"pipelined (margin {margin}, streams {smap})"
            pipe.enqueue_host(rgb[0], streams=lst)
            assert [_res(r) for r in pipe.wait_next()] == want_res[0]
            same(pipe, 0, tag, smap)
            i = 1
            while i + 1 < N:
                pipe.enqueue_host(rgb[i], streams=lst)
                pipe.enqueue_host(rgb[i + 1], streams=lst)
                assert [_res(r) for r in pipe.wait_next()] == want_res[i], f"{tag}, frame {i}"
                same(pipe, i, tag, smap)                    # the older pass's records, a younger one still outstanding
                assert [_res(r) for r in pipe.wait_next()] == want_res[i + 1], f"{tag}, frame {i + 1}"
                same(pipe, i + 1, tag, smap)
                i += 2
            if margin < 0:
                assert pipe.host_redos() > 0, "no pass was redone: the redo path was not exercised"
            pipe.close()

    a, b = gpu.Group(weights_tiny, n_streams=2), gpu.Group(weights_tiny, n_streams=3)
    setup(a)
    setup(b, smap=(2, 0), init=False)
    for i in range(N):
        fr, keep = _dev(gpu, rgb[i])
        if i < N // 2:
            assert [_res(r) for r in a.update_device(fr)] == want_res[i]
            same(a, i, "first engine")
            if i == N // 2 - 1:
                a.copy_stream(0, b, 2)
                a.copy_stream(1, b, 0)
        else:
            assert [_res(r) for r in b.update_device(fr, streams=[2, 0])] == want_res[i], f"second engine, frame {i}"
            same(b, i, "second engine", (2, 0))
    a.close()
    b.close()


def test_pipelined_equals_synchronous_at_the_frame_edge(gpu, weights_tiny):
    """the clip of the chips' and the refresh's edge test (a 96-px target along the left frame edge, every third clip frame,
    margin -1): passes are redone, and whatever the windows were, the records after every wait_next are the synchronous run's"""
    N = 16
    sc = gpu.synth.MovingSquare(W, H, 96, seed=7, center=(70.0, 240.0), amp=22.0)
    frames = [[sc.frame_rgb8(3 * i)] for i in range(N)]

    def make():
        g = gpu.Group(weights_tiny, n_streams=1, host_window_margin_pct=-1)
        g.init_host(0, frames[0][0], gpu.BBox.new(*sc.gt_box(0)))
        g.set_peaks(6, 2, 0.0)
        return g

    sync = make()
    want = []
    for i in range(N):
        r = _res(sync.update_host(frames[i])[0])
        want.append((r, sync.last_peaks(1).tobytes()))
    assert sync.host_redos() == 0
    sync.close()
    redos = []
    for first in (0, 1):
        pipe = make()
        i = 0
        if first:
            pipe.enqueue_host(frames[0])
            assert _res(pipe.wait_next()[0]) == want[0][0]
            assert pipe.last_peaks(1).tobytes() == want[0][1]
            i = 1
        while i + 1 < N:
            pipe.enqueue_host(frames[i])
            pipe.enqueue_host(frames[i + 1])
            assert _res(pipe.wait_next()[0]) == want[i][0], f"frame {i}"
            assert pipe.last_peaks(1).tobytes() == want[i][1], f"frame {i}: records"
            assert _res(pipe.wait_next()[0]) == want[i + 1][0], f"frame {i + 1}"
            assert pipe.last_peaks(1).tobytes() == want[i + 1][1], f"frame {i + 1}: records"
            i += 2
        redos.append(pipe.host_redos())
        pipe.close()
    assert redos[0] > 0, "no pass was redone: the case shows nothing"


def test_candidate_pass_winners_carry_records_losers_none(gpu, weights_tiny):
    hann = _hann(gpu, weights_tiny)
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in (0, 1, 2)]
    g = gpu.Group(weights_tiny, n_streams=3)
    fr, keep = _dev(gpu, [sc.frame_rgb8(0) for sc in scs])
    for s in range(3):
        g.init_device(s, fr[s], gpu.BBox.new(*scs[s].gt_box(0)))
    pols = {0: (4, 2, 0.0), 1: (8, 2, 0.0), 2: (4, 2, 0.0)}
    _apply(g, pols)
    res = g.update_device(fr)
    _check_pass(gpu, g, hann, [0, 1, 2], pols, res, "full pass")
    for t in (1, 2):
        f1, keep1 = _dev(gpu, [scs[1].frame_rgb8(t), scs[2].frame_rgb8(t)])
        box = g.read_state(1)["box"]
        cands = [(1, [4.0, 4.0, 40.0, 40.0]), (2, None), (1, [float(box[0]) + 6, float(box[1]) - 4, float(box[2]), float(box[3])])]
        res, win = g.update_device_candidates(cands, [f1[0], f1[1], f1[0]])
        assert win[1] == 1 and win[0] == win[2] and win[0] in (0, 2) and res[win[0]].success, (win, res)
        rec = _check_pass(gpu, g, hann, [1, 2, 1], pols, res, f"candidate pass {t}", winner=win)
        w, loser = win[0], 2 - win[0]
        assert rec["n"][loser] == 0 and rec["n"][1] >= 1 and rec["n"][w] >= 1 and (rec["stream"][1], rec["stream"][w]) == (2, 1)
        assert rec["frames_done"][w] == t + 1 and rec["frames_done"][1] == t + 1
    g.close()


def test_a_twin_that_never_enables_tracks_and_launches_as_before(gpu, weights_tiny):
    """targets of 40, 64 and 104 px: at search 128 the crop tiers change near 43 and 67 px, so the subset passes [0], [0, 1]
    and [1, 2] and the full pass run in different tiers; then every stream's box is grown through both boundaries on full
    passes, which replay all three captured graphs (graph_replays says so). Results and states are the twin's throughout
    and no graph is captured after the enable."""
    scs = [gpu.synth.MovingSquare(W, H, sq, seed=s) for s, sq in enumerate((40, 64, 104))]
    main, twin = gpu.Group(weights_tiny, n_streams=3), gpu.Group(weights_tiny, n_streams=3)
    fr, keep = _dev(gpu, [sc.frame_rgb8(0) for sc in scs])
    for g in (main, twin):
        for s in range(3):
            g.init_device(s, fr[s], gpu.BBox.new(*scs[s].gt_box(0)))
    twin_caps = twin.graph_captures()
    main.set_peaks(8, 2, 0.0)
    main.set_peaks(8, 2, 0.0)          # again: a policy write, no capture
    caps = main.graph_captures()
    assert caps > twin_caps
    lists = [None, [0], None, [0, 1], [1, 2], None, [0], [0, 1]]
    for t, lst in enumerate(lists):
        fr, keep = _dev(gpu, [sc.frame_rgb8(t) for sc in scs])
        if lst is None:
            a, b = main.update_device(fr), twin.update_device(fr)
        else:
            sub = [fr[s] for s in lst]
            a, b = main.update_device(sub, streams=lst), twin.update_device(sub, streams=lst)
        assert [_res(r) for r in a] == [_res(r) for r in b], f"update {t + 1}"
        assert _states(main).tobytes() == _states(twin).tobytes(), f"update {t + 1}: states"
        assert main.last_peaks(len(a))["n"].min() >= 1
        if t == 4:
            main.set_peaks(3, 1, 0.1, stream=2)
    assert main.graph_captures() == caps and twin.graph_captures() == twin_caps, "a graph was captured after the enable"
    # full passes while every target grows from 30 to 100 px: the replayed graph changes twice
    before = [g.read_tensor("graph_replays").copy() for g in (main, twin)]
    fr, keep = _dev(gpu, [sc.frame_rgb8(8) for sc in scs])
    for size in range(30, 102, 6):
        for g in (main, twin):
            for s in range(3):
                g.set_state_box(s, [300.0 - size / 2 + 10 * s, 240.0 - size / 2, float(size), float(size)])
        a, b = main.update_device(fr), twin.update_device(fr)
        assert [_res(r) for r in a] == [_res(r) for r in b], f"target size {size}"
        assert _states(main).tobytes() == _states(twin).tobytes(), f"target size {size}: states"
    for g, b0 in zip((main, twin), before):
        rep = g.read_tensor("graph_replays") - b0
        assert rep.sum() == 12 and (rep > 0).all(), f"the full passes did not cross the tiers: replays per tier {rep}"
    assert main.graph_captures() == caps and twin.graph_captures() == twin_caps, "a tier crossing captured a graph"
    names = [[f["name"] for f in g.profile_device(fr, iters=1)] for g in (main, twin)]
    assert "response_peaks" not in names[1] and names[1][-1].startswith(("head_conv3x3", "decode")), names[1]
    assert names[0] == names[1] + ["response_peaks"], names[0]
    with pytest.raises(gpu.VtError) as ei:
        twin.last_peaks()
    assert ei.value.code == INVALID
    main.close()
    twin.close()


def test_refresh_chips_and_peaks_on_one_engine(gpu, weights_tiny):
    """all three launches behind one decode: tracking, templates and chips are those of the engine without peaks, and a
    stream's snapshot is the same bytes with and without a peaks policy"""
    hann = _hann(gpu, weights_tiny)
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    allf, twin = gpu.Group(weights_tiny, n_streams=1), gpu.Group(weights_tiny, n_streams=1)
    fr, keep = _dev(gpu, [sc.frame_rgb8(0)])
    for g in (allf, twin):
        g.init_device(0, fr[0], gpu.BBox.new(*sc.gt_box(0)))
        g.set_template_refresh(2, 0.0)
        g.enable_chips(64, gpu.CHIP_RGB8)
        g.set_chips(2.0)
    allf.set_peaks(8, 2, 0.0)
    for t in range(8):
        fr, keep = _dev(gpu, [sc.frame_rgb8(t)])
        ra, rb = allf.update_device(fr), twin.update_device(fr)
        assert _res(ra[0]) == _res(rb[0]), f"update {t + 1}"
        _check_pass(gpu, allf, hann, [0], {0: (8, 2, 0.0)}, ra, f"update {t + 1}")
        assert _states(allf).tobytes() == _states(twin).tobytes()
        assert np.array_equal(allf.read_tensor("template", 0).view(np.uint32), twin.read_tensor("template", 0).view(np.uint32))
        ca, cb = allf.read_chips(), twin.read_chips()
        assert np.array_equal(ca[0], cb[0]) and ca[1] == cb[1]
        assert allf.export_stream(0) == twin.export_stream(0), "the snapshot carries something of the peaks policy"
    assert allf.template_refresh_stats(0)["generation"] == 4
    names = [f["name"] for f in allf.profile_device(fr, iters=1)]
    assert names[-3:] == ["refresh_template", "target_chips", "response_peaks"], names[-4:]
    allf.close()
    twin.close()


def test_bad_arguments_change_nothing(gpu, weights_tiny):
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

    bad = [(9, 2, 0.0, None), (-1, 2, 0.0, None), (4, 0, 0.0, None), (4, 5, 0.0, None), (4, 2, nan, None), (4, 2, -0.01, None),
           (4, 2, 1.01, None), (4, 2, inf, None), (4, 2, 0.0, 2)]
    refused(g.last_peaks)                                           # before any enable
    refused(g.set_peaks, 0)                                         # switching off what was never on
    for K, R, m, s in bad:
        refused(g.set_peaks, K, R, m, stream=s)
    refused(lambda: gpu._check(gpu.lib().vt_group_set_peaks(g._h, -2, 4, 2, ctypes.c_float(0.0))))
    g.enqueue_host([rgb1, rgb1])
    refused(g.set_peaks, 4)                                         # a pipelined pass is outstanding
    g.wait_next()
    assert g.graph_captures() == caps, "a refused call captured"
    refused(g.last_peaks)                                           # still not enabled
    g.set_peaks(4, 2, 0.0, stream=1)
    caps = g.graph_captures()
    g.update_host([rgb1, rgb1])
    before = g.last_peaks().tobytes()
    assert np.frombuffer(before, gpu.PEAKS_DTYPE)["n"][0] == 0 and np.frombuffer(before, gpu.PEAKS_DTYPE)["n"][1] >= 1
    for K, R, m, s in bad:
        refused(g.set_peaks, K, R, m, stream=s)
    assert g.last_peaks().tobytes() == before, "a refused set_peaks touched the records"
    refused(lambda: gpu._check(gpu.lib().vt_group_last_peaks(g._h, None, 2)))
    rec = np.zeros(2, gpu.PEAKS_DTYPE)
    refused(lambda: gpu._check(gpu.lib().vt_group_last_peaks(g._h, rec.ctypes.data, 0)))
    refused(lambda: gpu._check(gpu.lib().vt_group_last_peaks(g._h, rec.ctypes.data, -3)))
    assert not rec.view(np.uint8).any(), "a refused last_peaks wrote to its output"
    assert g.last_peaks().tobytes() == before, "a refused last_peaks touched the records"
    g.enqueue_host([rgb1, rgb1])
    refused(g.set_peaks, 2, 1, 0.0)
    assert g.last_peaks().tobytes() == before, "the records moved before the outstanding pass was collected"
    g.wait_next()
    assert g.graph_captures() == caps
    # the policy is what it was: stream 0 off, stream 1 lists up to 4 at radius 2 - the next record's header says so
    now = g.last_peaks()
    assert now["n"][0] == 0 and 1 <= now["n"][1] <= 4 and now["radius"][1] == 2 and now["frames_done"][1] == 3
    g.close()


def test_single_tracker_wrappers(gpu, weights_tiny):
    hann = _hann(gpu, weights_tiny)
    sc = gpu.synth.MovingSquare(W, H, 64, seed=1)
    trk = gpu.VitTrack(weights_tiny)
    trk.init(sc.frame_rgb8(0), gpu.BBox.new(*sc.gt_box(0)))
    with pytest.raises(gpu.VtError):
        trk.last_peaks()
    with pytest.raises(gpu.VtError):
        trk.set_peaks(9)
    trk.set_peaks(5, 2, 0.0)
    view = trk.as_group()
    for t in range(3):
        r = trk.update(sc.frame_rgb8(t))
        rec = trk.last_peaks()
        assert rec.tobytes() == view.last_peaks(1).tobytes()
        assert 1 <= rec["n"][0] <= 5 and rec["stream"][0] == 0 and rec["frames_done"][0] == t + 1 and rec["radius"][0] == 2
        _check_pass(gpu, view, hann, [0], {0: (5, 2, 0.0)}, [r], f"update {t + 1}")
    trk.close()
