"""Reacquire proposals in the engine (the "proposals*" keys of vt_group_set_tuning), on the MI355X.

Yardsticks: the NumPy model of tests/proposals_util.py fed with the "state" and "template" the engine returns (record,
pattern and map bit for bit); a PLAIN engine that never enables the option (the read-only twin: results, state words,
templates, chips, peaks and drawn frames bit for bit); and the oracle fixture tests/golden/proposals_cfg2.npz
(tests/golden/make_proposals.py) with the bars of test_gpu_candidates.py: boxes within 1 px, scores within 0.03, equal
success flags."""
import os

import numpy as np
import pytest

import proposals_util as pu
from test_gpu_stream_subsets import FRAMES_DONE, _res, _words

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 640, 480
INVALID, OOM = -1, -8


def _dev(gpu, buf, w=W, h=H):
    """(device NV12 frame, keep-alive tensor) of a packed buffer"""
    import torch
    d = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
    return gpu.frame_nv12(d.data_ptr(), d.data_ptr() + w * h, w, h), d


def _norm(oracle, weights):
    hdr = oracle.Model(weights).hdr
    return hdr["norm_a"], hdr["norm_b"]


def _rows(g, s):
    mi = g.model_info()
    return (g.read_tensor("template", s).view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(mi.tokens_template, mi.kpad)


def _check_record(g, s, buf, w, h, norm, status=1):
    """stream s's record, pattern and map against the model on the state and template the engine returns"""
    rec = g.proposals(s)
    mi = g.model_info()
    st = g.read_state(s)
    assert rec["status"] == status and rec["frames_done"] == int(_words(g, s)[FRAMES_DONE]), rec
    if status != 1:
        assert rec["n"] == 0 and rec["proposals"] == []
        return rec, None
    want = pu.evaluate(pu.to_rgb("nv12", buf, w, h), st["box"], _rows(g, s), mi.template_size, mi.patch, norm[0], norm[1],
                       max_cells=rec["max_cells"], max_n=rec["max_n"], min_sim_pm=rec["min_sim_pm"])
    assert want["status"] == 1
    assert np.float32(rec["c"]).tobytes() == np.float32(want["c"]).tobytes() and rec["grid"] == (want["Wg"], want["Hg"])
    assert np.array_equal(g.proposals_pattern(s), want["pattern"].astype(np.float32))
    assert np.array_equal(g.proposals_map(s).view(np.uint32), want["map"].view(np.uint32))
    p = want["proposals"]
    assert rec["n"] == len(p)
    for k, q in enumerate(rec["proposals"]):
        assert np.float32(q["sim"]).tobytes() == p["sim"][k].tobytes() and q["pos"] == int(p["pos"][k])
        assert np.array(q["box"], np.float32).tobytes() == p["box"][k].tobytes()
    return rec, want


def _group(gpu, weights, B, scs, **kw):
    g = gpu.Group(weights, n_streams=B, **kw)
    keep = [_dev(gpu, sc.frame_nv12(0)) for sc in scs]
    for s in range(B):
        g.init_device(s, keep[s][0], gpu.BBox.new(*scs[s].gt_box(0)))
    return g


def test_record_pattern_and_map_equal_the_model(gpu, oracle, weights_tiny):
    B = 3
    scs = [gpu.synth.MovingSquare(W, H, 56 + 8 * s, seed=s) for s in range(B)]
    g = _group(gpu, weights_tiny, B, scs)
    norm = _norm(oracle, weights_tiny)
    g.set_proposals(2, min_sim=0.3, max_cells=16384)
    for t in (1, 2):
        bufs = [sc.frame_nv12(t) for sc in scs]
        pairs = [_dev(gpu, b) for b in bufs]
        res = g.update_device([p[0] for p in pairs])
        for s in range(B):
            rec, want = _check_record(g, s, bufs[s], W, H, norm)
            assert rec["evaluated"] == t and rec["n"] >= 1
            gt = scs[s].gt_box(t)
            b0 = rec["proposals"][0]["box"]
            assert abs(b0[0] + b0[2] / 2 - gt[0] - gt[2] / 2) <= rec["c"] and abs(b0[1] + b0[3] / 2 - gt[1] - gt[3] / 2) <= rec["c"]
    # a subset pass: the record of a stream outside it stays
    bufs = [sc.frame_nv12(3) for sc in scs]
    pairs = [_dev(gpu, b) for b in bufs]
    before = g.proposals(1)
    g.update_device([pairs[2][0], pairs[0][0]], streams=[2, 0])
    _check_record(g, 2, bufs[2], W, H, norm)
    _check_record(g, 0, bufs[0], W, H, norm)
    assert g.proposals(1) == before
    g.close()


def _enable_all(gpu, g, proposals):
    g.set_template_refresh(2, 0.0)
    g.enable_chips(32, gpu.CHIP_RGB8)
    g.set_chips(2.0)
    g.set_peaks(4)
    g.set_result_overlay()
    if proposals:
        g.set_proposals(2, min_sim=0.3, max_cells=16384)


def test_read_only_twin_over_a_dozen_passes(gpu, weights_tiny):
    """full, subset, candidate and pipelined host passes with refresh, chips, peaks and the overlay beside the option on
    both engines: the option only reads. Each engine draws into device frames of its own."""
    B = 3
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=s) for s in range(B)]
    main, plain = _group(gpu, weights_tiny, B, scs), _group(gpu, weights_tiny, B, scs)
    _enable_all(gpu, main, True)
    _enable_all(gpu, plain, False)
    caps = main.graph_captures()

    def same(rm, rp, tag, drawn=None):
        assert [_res(r) for r in rm] == [_res(r) for r in rp], tag
        for s in range(B):
            assert np.array_equal(_words(main, s), _words(plain, s)), f"{tag}: stream {s}: state words"
            assert np.array_equal(_rows(main, s), _rows(plain, s)), f"{tag}: stream {s}: template"
        (cm, im), (cp, ip) = main.read_chips(), plain.read_chips()
        assert np.array_equal(cm, cp) and im == ip, f"{tag}: chips"
        assert main.last_peaks().tobytes() == plain.last_peaks().tobytes(), f"{tag}: peaks"
        for a, b in drawn or []:
            assert np.array_equal(a[1].cpu().numpy(), b[1].cpu().numpy()), f"{tag}: drawn frame"

    t = 1
    for L in [None, None, [2, 0], None, [1], None]:
        streams = L if L is not None else list(range(B))
        pm, pp = ([_dev(gpu, scs[s].frame_nv12(t)) for s in streams] for _ in range(2))
        same(main.update_device([p[0] for p in pm], streams=L), plain.update_device([p[0] for p in pp], streams=L), f"pass {t} {L}",
             list(zip(pm, pp)))
        for s in streams:
            assert main.proposals(s)["status"] == 1
        t += 1
    box = main.read_state(1)["box"]
    cands = [(1, [4.0, 4.0, 40.0, 40.0]), (1, None), (1, [float(box[0]) + 5, float(box[1]) - 3, float(box[2]), float(box[3])])]
    fm, fp = _dev(gpu, scs[1].frame_nv12(t)), _dev(gpu, scs[1].frame_nv12(t))
    ev = main.proposals(1)["evaluated"]
    (rm, wm), (rp, wp) = main.update_device_candidates(cands, [fm[0]] * 3), plain.update_device_candidates(cands, [fp[0]] * 3)
    assert wm == wp
    same(rm, rp, "candidate pass", [(fm, fp)])
    rec = main.proposals(1)
    assert rec["status"] == 1 and rec["evaluated"] == ev + 1, "a candidate pass evaluates its winning slot, once"
    t += 1
    pm, pp = ([_dev(gpu, sc.frame_nv12(t)) for sc in scs] for _ in range(2))
    same(main.update_device([p[0] for p in pm]), plain.update_device([p[0] for p in pp]), "full pass after the candidate pass", list(zip(pm, pp)))
    # host passes: synchronous, then pipelined - only their windows are on the device: status 4, nothing evaluated
    ev = [main.proposals(s)["evaluated"] for s in range(B)]
    frames = [[gpu.NV12Frame(sc.frame_nv12(t + 1 + i), W, H) for sc in scs] for i in range(4)]
    same(main.update_host(frames[0]), plain.update_host(frames[0]), "synchronous host pass")
    for g in (main, plain):
        g.enqueue_host(frames[1])
    for i in (2, 3):
        for g in (main, plain):
            g.enqueue_host(frames[i])
        assert [_res(r) for r in main.wait_next()] == [_res(r) for r in plain.wait_next()], f"pipelined pass {i - 1}"
    same(main.wait_next(), plain.wait_next(), "the last pipelined pass")
    assert main.host_redos() == plain.host_redos(), "the option added a redo"
    for s in range(B):
        rec = main.proposals(s)
        assert rec["status"] == 4 and rec["n"] == 0 and rec["evaluated"] == ev[s]
        assert rec["frames_done"] == int(_words(main, s)[FRAMES_DONE])
    assert sum(main.template_refresh_stats(s)["generation"] for s in range(B)) >= 3, "no refresh ran beside the option"
    assert main.graph_captures() == caps, "a pass or a key captured a graph"
    main.close()
    plain.close()


def test_due_rules(gpu, oracle, weights_tiny):
    B = 2
    scs = [gpu.synth.MovingSquare(W, H, 64, seed=0), gpu.synth.MovingSquare(W, H, 64, seed=1, hide=(3, 6))]
    g = _group(gpu, weights_tiny, B, scs)
    norm = _norm(oracle, weights_tiny)
    caps = g.graph_captures()
    g.set_proposals(1, min_sim=0.3, max_cells=16384)
    assert g.graph_captures() > caps
    caps = g.graph_captures()
    # mode 1: a successful update is not due, a failed one (stream 1's target is hidden on frames 3-5) is
    failed = 0
    for t in range(1, 7):
        bufs = [sc.frame_nv12(t) for sc in scs]
        pairs = [_dev(gpu, b) for b in bufs]
        res = g.update_device([p[0] for p in pairs])
        for s in range(B):
            _check_record(g, s, bufs[s], W, H, norm, status=0 if res[s].success else 1)
        failed += not res[1].success
    assert res[0].success and failed >= 1, "the occlusion failed no update"
    # mode 2 with period 2: due on even frames_done (the count behind the pass)
    g.set_proposals(2, period=2)
    for t in (7, 8, 9):
        bufs = [sc.frame_nv12(t) for sc in scs]
        pairs = [_dev(gpu, b) for b in bufs]
        g.update_device([pairs[0][0]], streams=[0])
        fd = int(_words(g, 0)[FRAMES_DONE])
        _check_record(g, 0, bufs[0], W, H, norm, status=1 if fd % 2 == 0 else 0)
    # a windowed device frame: its planes do not hold the whole frame
    g.set_proposals(2, period=1)
    buf = scs[0].frame_nv12(10)
    f, keep = _dev(gpu, buf)
    win = gpu.CFrame(f.plane0, f.plane1, W, H, f.stride0, f.stride1, f.format, 0, 0, 1, W, H - 2)
    assert g.update_device([win], streams=[0])[0].success
    _check_record(g, 0, buf, W, H, norm, status=4)
    assert g.update_device([f], streams=[0])[0].success
    _check_record(g, 0, buf, W, H, norm, status=1)
    # off again: status 0, and no capture since the enable
    g.set_proposals(0)
    g.update_device([f], streams=[0])
    assert g.proposals(0)["status"] == 0 and g.proposals(0)["mode"] == 0
    assert g.graph_captures() == caps
    g.close()


def test_keys_ranges_and_memory_cap(gpu, weights_tiny):
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = _group(gpu, weights_tiny, 2, [sc, sc])
    for name in ("proposals", "proposals_pattern", "proposals_map"):      # never enabled: no such tensor
        with pytest.raises(gpu.VtError) as ei:
            g.read_tensor(name, 0)
        assert ei.value.code == INVALID
    caps = g.graph_captures()
    for key, v in (("proposals_period", 5), ("proposals_max", 2), ("proposals_min_sim_pm", 250), ("proposals_max_cells", 16384),
                   ("proposals", 0)):
        g.set_tuning(key, v)                                # remembered until the enable
    bad = (("proposals", 3), ("proposals_period", 0), ("proposals_period", 1000001), ("proposals_max", 0), ("proposals_max", 9),
           ("proposals_min_sim_pm", 1001), ("proposals_max_cells", 16383), ("proposals_max_cells", 4194305), ("proposals_nope", 1))
    for key, v in bad:
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning(key, v)
        assert ei.value.code == INVALID, (key, v)
    assert g.graph_captures() == caps
    g.set_tuning("proposals", 1)
    caps_on = g.graph_captures()
    assert caps_on > caps
    rec = g.proposals(1)
    assert (rec["mode"], rec["period"], rec["max_n"], rec["min_sim_pm"], rec["max_cells"], rec["status"], rec["evaluated"]) == \
        (1, 5, 2, 250, 16384, 0, 0)
    for key, v in bad + (("proposals_max_cells", 32768), ("proposals_max_cells", -1)):     # max_cells: before the first enable only
        with pytest.raises(gpu.VtError) as ei:
            g.set_tuning(key, v)
        assert ei.value.code == INVALID, (key, v)
        assert g.proposals(1) == rec
    for key in ("proposals_period", "proposals_max", "proposals_min_sim_pm"):
        g.set_tuning(key, -1)                               # negative: the default
    rec = g.proposals(0)
    assert (rec["period"], rec["max_n"], rec["min_sim_pm"]) == (1, 4, 500) and g.graph_captures() == caps_on
    g.close()
    # under the smallest max_device_mib that still creates a 64-stream engine the default store (64 x 1.5 MiB) cannot fit
    B = 64

    def create(mib):
        try:
            return gpu.Group(weights_tiny, n_streams=B, max_device_mib=mib, use_graph=False)
        except gpu.VtError as e:
            assert e.code == OOM
            return None
    lo, hi = 0, 4096
    while hi - lo > 1:
        mid = (lo + hi) // 2
        h = create(mid)
        if h is None:
            lo = mid
        else:
            h.close()
            hi = mid
    h = create(hi + 8)
    f0, k0 = _dev(gpu, sc.frame_nv12(0))
    for s in range(B):
        h.init_device(s, f0, gpu.BBox.new(*sc.gt_box(0)))
    h.set_tuning("proposals_period", 7)
    with pytest.raises(gpu.VtError) as ei:
        h.set_tuning("proposals", 1)
    assert ei.value.code == OOM
    with pytest.raises(gpu.VtError) as ei:
        h.read_tensor("proposals", 5)
    assert ei.value.code == INVALID, "the refused enable left the engine capable"
    f1, k1 = _dev(gpu, sc.frame_nv12(1))
    assert all(r.success for r in h.update_device([f1] * B))
    h.set_tuning("proposals_max_cells", 16384)              # 64 x 96 KiB = 6 MiB fit into the 8 MiB of room
    h.set_tuning("proposals", 2)
    assert all(r.success for r in h.update_device([f1] * B))
    rec = h.proposals(63)
    assert (rec["period"], rec["status"], rec["max_cells"]) == (7, 0, 16384)
    h.close()


def test_four_launches_on_enabled_engines_only(gpu, weights_tiny):
    assert len(gpu.EXPORTS) == 91 and "vt_op_proposals" in gpu.OPS_EXPORTS
    sc = gpu.synth.MovingSquare(W, H, 64, seed=0)
    g = _group(gpu, weights_tiny, 2, [sc, sc])
    f0, k0 = _dev(gpu, sc.frame_nv12(0))
    g.set_template_refresh(2, 0.0)
    g.set_result_overlay()
    plain = g.profile_device([f0, f0], iters=2)
    assert not [k for k in plain if k["name"].startswith("proposals")]
    g.set_proposals(2, max_cells=16384)
    fams = {k["name"]: k["launches"] for k in g.profile_device([f0, f0], iters=2)}
    names = ["proposals_prepare", "proposals_thumb", "proposals_match", "proposals_list"]
    assert {n: c for n, c in fams.items() if n.startswith("proposals")} == {n: 1 for n in names}
    assert sum(fams.values()) == sum(k["launches"] for k in plain) + 4
    order = [k["name"] for k in g.profile_device([f0, f0], iters=1)]
    at = [order.index(n) for n in names]
    assert at == list(range(at[0], at[0] + 4)) and at[3] < order.index("refresh_template") < order.index("result_overlay")
    g.close()


def test_reacquisition_on_the_committed_clip(gpu, oracle, weights_cfg2, capsys):
    """stream 0 of a 4-stream cfg2 group loses its target on frame 3 (a jump of about 550 px) while three streams track
    clips of their own. The failed update's record lists the target; ONE candidate pass over the listed boxes commits it
    (Group.reacquire(..., proposals=True) never starts the scan); that result and five closed-loop frames follow the
    oracle fixture."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_reacquire", os.path.join(HERE, "golden", "make_reacquire.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with np.load(os.path.join(HERE, "golden", "proposals_cfg2.npz")) as z:
        fx = {k: z[k] for k in z.files}
    assert gen.sha256_file(weights_cfg2) == str(fx["weights_sha256"]), "fixture made with other weights"
    w, h, G, jump = gen.W, gen.H, 4, int(fx["jump_at"])
    frame0, gt0 = gen.clip()
    others = [gpu.synth.MovingSquare(w, h, 56 + 4 * i, seed=100 + i) for i in range(1, G)]
    norm = _norm(oracle, weights_cfg2)
    grp = gpu.Group(weights_cfg2, n_streams=G)
    grp.set_proposals(1)
    caps = grp.graph_captures()

    def frames_at(t):
        bufs = [frame0(t)] + [sc.frame_nv12(t) for sc in others]
        return bufs, [_dev(gpu, b, w, h) for b in bufs]

    def near(r, bbox, score, success, tag):
        assert bool(r.success) == bool(success), (tag, r)
        assert np.abs(np.array(r.bbox) - bbox).max() <= 1 and abs(r.score - float(score)) < 0.03, (tag, r, bbox, score)

    for t in range(jump + 1 + len(fx["track_bbox"])):
        bufs, pairs = frames_at(t)
        if t == 0:
            grp.init_device(0, pairs[0][0], gpu.BBox.new(*gt0(0)))
            for i, sc in enumerate(others, start=1):
                grp.init_device(i, pairs[i][0], gpu.BBox.new(*sc.gt_box(0)))
        res = grp.update_device([p[0] for p in pairs])
        assert all(r.success for r in res[1:]), f"frame {t}: a tracking stream failed"
        if t < jump:
            assert res[0].success and grp.proposals(0)["status"] == 0
        elif t == jump:
            assert not res[0].success
            rec, want = _check_record(grp, 0, bufs[0], w, h, norm)
            gt = fx["gt_box"].astype(np.float64)
            b0 = rec["proposals"][0]["box"]
            assert abs(b0[0] + b0[2] / 2 - gt[0] - gt[2] / 2) <= rec["c"] and abs(b0[1] + b0[3] / 2 - gt[1] - gt[3] / 2) <= rec["c"]
            assert rec["proposals"][0]["sim"] >= 0.8
            with capsys.disabled():
                print(f"\n[proposals cfg2] frame {t}: {[(round(p['sim'], 4), p['box']) for p in rec['proposals']]}; fixture "
                      f"{fx['proposal_sim'].tolist()} {fx['proposal_box'].tolist()}")
            assert all(grp.proposals(i)["status"] == 0 for i in range(1, G))
            done = int(_words(grp, 0)[FRAMES_DONE])
            best = grp.reacquire(0, pairs[0][0], proposals=True)
            assert grp.last_scan == [] and grp.last_proposal_pass is not None, "the scan ran"
            assert len(grp.last_proposal_pass[0]) == rec["n"] <= G
            assert int(_words(grp, 0)[FRAMES_DONE]) == done + 1, "one candidate pass is one update of the stream"
            wi = int(fx["winner"])
            near(best, fx["cand_bbox"][wi], fx["cand_score"][wi], fx["cand_success"][wi], "the committed candidate")
        else:
            k = t - jump - 1
            near(res[0], fx["track_bbox"][k], fx["track_score"][k], fx["track_success"][k], f"closed loop, frame {t}")
    assert grp.graph_captures() == caps
    grp.close()
