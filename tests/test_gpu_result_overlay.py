"""Result overlay inside the pass (the "result_overlay*" keys of vt_group_set_tuning), on the MI355X.

Tiny model, frames of 320x240, 3-4 streams, 6-8 frames, NV12 and RGB8. For every kind of device pass the frames after the
call equal result_overlay_util.expected drawn (by the existing oracle.vit_ref.draw / draw_rgb) from the RETURNED results -
every byte - and a twin engine without the overlay returns bit-identical results and states. One check at cfg3 with 1080p."""
import struct

import numpy as np
import pytest

import result_overlay_util as ro

pytestmark = pytest.mark.gpu

W, H = 320, 240
GATE = 0        # the tiny model's scores are whatever its seeded weights give: the gate of these tests is score > 0


def _res(r):
    return tuple(r.bbox), int(r.success), struct.unpack("<I", struct.pack("<f", r.score))[0]


def _slot(r):
    return (int(r.success), r.score, tuple(r.bbox))


def _clip(gpu, fmt, seed, t, w=W, h=H, square=48):
    sc = gpu.synth.MovingSquare(w, h, square, seed=seed, period=60)
    return (sc.frame_nv12(t) if fmt == "nv12" else sc.frame_rgb8(t).reshape(-1)), sc.gt_box(0)


class Up:
    """a packed NV12 / RGB8 frame uploaded to the device"""

    def __init__(self, gpu, fmt, buf, w=W, h=H):
        import torch
        self.fmt, self.buf, self.w, self.h = fmt, np.ascontiguousarray(buf, np.uint8).reshape(-1), w, h
        self.t = torch.from_numpy(self.buf.copy()).cuda()
        p = self.t.data_ptr()
        self.frame = gpu.frame_nv12(p, p + w * h, w, h) if fmt == "nv12" else gpu.frame_rgb8(p, w, h)

    def read(self):
        return self.t.cpu().numpy()


def _states(g):
    return [g.read_tensor("state", s).tobytes() for s in range(g.streams)]


def _pair(gpu, weights, fmt, B, overlay=None, seeds=None):
    """an engine with the overlay and its twin without, every stream initialised on frame 0 of its clip"""
    seeds = list(range(B)) if seeds is None else seeds
    a, b = gpu.Group(weights, n_streams=B), gpu.Group(weights, n_streams=B)
    for g in (a, b):
        for s in range(B):
            buf, box = _clip(gpu, fmt, seeds[s], 0)
            g.init_device(s, Up(gpu, fmt, buf).frame, gpu.BBox.new(*box))
    a.set_result_overlay(**(overlay or dict(min_score_pct=GATE)))
    return a, b, seeds


def _expect(oracle, ups, results, winners=None, **pol):
    """every uploaded frame against the list of the slots that drew into it, in slot order"""
    drew = 0
    seen = []
    for u in ups:
        if any(u is v for v in seen):
            continue
        seen.append(u)
        slots = [_slot(results[i]) for i, v in enumerate(ups) if v is u and (winners is None or winners[i] == i)]
        want = ro.expected(oracle, u.fmt, u.buf, u.w, u.h, slots, **pol)
        assert np.array_equal(u.read(), want), f"frame of slots {[i for i, v in enumerate(ups) if v is u]} differs from the reference"
        drew += int((want != u.buf).any())
    return drew


@pytest.mark.parametrize("fmt", ["nv12", "rgb8"])
def test_every_kind_of_device_pass_draws_and_the_twin_agrees(gpu, oracle, weights_tiny, fmt, capsys):
    B = 4
    pol = dict(min_score_pct=GATE, luma=250, rgb=0xF000F0)
    a, tw, seeds = _pair(gpu, weights_tiny, fmt, B, overlay=pol)
    caps = a.graph_captures()
    drew, scores = 0, []
    passes = {s: 0 for s in range(B)}
    for t in range(1, 9):
        bufs = [_clip(gpu, fmt, seeds[s], t)[0] for s in range(B)]
        ua, ut = [Up(gpu, fmt, b) for b in bufs], [Up(gpu, fmt, b) for b in bufs]
        kind = ("full", "subset", "candidate", "enqueue")[t % 4]
        winners = None
        if kind == "full":
            fa, ft, lst = ua, ut, list(range(B))
            ra, rt = a.update_device([u.frame for u in fa]), tw.update_device([u.frame for u in ft])
        elif kind == "subset":
            lst = [2, 0, 3]
            fa, ft = [ua[s] for s in lst], [ut[s] for s in lst]
            ra = a.update_device([u.frame for u in fa], streams=lst)
            rt = tw.update_device([u.frame for u in ft], streams=lst)
        elif kind == "candidate":      # stream 0 twice on ONE frame (its own box and one 12 px off), streams 1 and 2 plain
            box = a.read_state(0)["box"]
            cands = [0, (0, (float(box[0]) + 12.0, float(box[1]) - 8.0, float(box[2]), float(box[3]))), 1, 2]
            lst = [0, 0, 1, 2]
            fa, ft = [ua[s] for s in lst], [ut[s] for s in lst]
            ra, winners = a.update_device_candidates(cands, [u.frame for u in fa])
            rt, wt = tw.update_device_candidates(cands, [u.frame for u in ft])
            assert winners == wt and winners[0] == winners[1] and winners[2:] == [2, 3]
        else:
            fa, ft, lst = ua, ut, list(range(B))
            a.enqueue_device([u.frame for u in fa])
            tw.enqueue_device([u.frame for u in ft])
            ra, rt = a.wait(), tw.wait()
        assert [_res(r) for r in ra] == [_res(r) for r in rt], f"frame {t} ({kind}): the overlay changed a result"
        assert _states(a) == _states(tw), f"frame {t} ({kind}): the overlay changed a state"
        drew += _expect(oracle, fa, ra, winners, **pol)
        for u, b in zip(ut, bufs):
            assert np.array_equal(u.read(), b), "an engine without the overlay wrote a frame"
        for u in ua:
            if not any(u is v for v in fa):
                assert np.array_equal(u.read(), u.buf), "a frame that was not in the pass was written"
        for i, s in enumerate(lst):
            if winners is None or winners[i] == i:
                passes[s] += 1
                st = a.result_overlay_stats(s)
                d = ro.draws(ra[i].success, ra[i].score, GATE)
                assert st["drawn"] == int(d) and st["flags"] == 7, (t, kind, s, st)
                if d:
                    assert st["last_n"] == ro.label_n(ra[i].score)
                scores.append(ra[i].score)
    for s in range(B):
        st = a.result_overlay_stats(s)
        assert st["n_drawn"] + st["n_gated"] == passes[s] and st["n_unsupported"] == 0, (s, st, passes)
    assert a.graph_captures() == caps, "a graph was captured after the enable"
    assert drew >= 12, f"only {drew} frames were drawn into: the comparison shows little"
    with capsys.disabled():
        print(f"\n[{fmt}] frames drawn {drew}, scores {min(scores):.3f} .. {max(scores):.3f}")
    a.close()
    tw.close()


@pytest.mark.parametrize("fmt", ["nv12", "rgb8"])
def test_single_tracker_device_calls(gpu, oracle, weights_tiny, fmt):
    pol = dict(min_score_pct=GATE, thickness=2, scale=1)
    a, tw = gpu.VitTrack.new(weights_tiny), gpu.VitTrack.new(weights_tiny)
    buf, box = _clip(gpu, fmt, 5, 0)
    for trk in (a, tw):
        trk.init_device(Up(gpu, fmt, buf).frame, gpu.BBox.new(*box))
    a.set_result_overlay(**pol)
    drew = 0
    for t in range(1, 7):
        buf = _clip(gpu, fmt, 5, t)[0]
        ua, ut = Up(gpu, fmt, buf), Up(gpu, fmt, buf)
        if t % 2:       # the format's own entry point, then vt_update_frame(on_device = 1)
            p, q = ua.t.data_ptr(), ut.t.data_ptr()
            if fmt == "nv12":
                ra, rt = a.update_nv12_device(p, p + W * H, W, H, W, W), tw.update_nv12_device(q, q + W * H, W, H, W, W)
            else:
                ra, rt = a.update_rgb8_device(p, W, H, 3 * W), tw.update_rgb8_device(q, W, H, 3 * W)
        else:
            ra, rt = a.update_device(ua.frame), tw.update_device(ut.frame)
        assert _res(ra) == _res(rt)
        drew += _expect(oracle, [ua], [ra], **pol)
        assert np.array_equal(ut.read(), buf)
        assert a.result_overlay_stats()["drawn"] == int(ro.draws(ra.success, ra.score, GATE))
    assert drew >= 4
    # a host frame through the same tracker: staged, never drawn into, and the record says so
    host = _clip(gpu, fmt, 5, 7)[0]
    keep = host.copy()
    f = gpu.NV12Frame(host, W, H) if fmt == "nv12" else host.reshape(H, W, 3)
    a.update(f)
    assert np.array_equal(host, keep) and a.result_overlay_stats()["drawn"] == 0
    a.close()
    tw.close()


def test_refresh_chips_and_peaks_see_undrawn_pixels(gpu, oracle, weights_tiny):
    """template refresh every second update, a chip every update, peaks - all beside an overlay of thickness 16 in the
    brightest colour, whose rectangle lies INSIDE the template crop (side 2 sqrt(w h)) and the chip crop (factor 2): were the
    overlay launched ahead of them, the template rows and the chips would carry the rectangle. They equal the twin's bits."""
    B, fmt = 3, "rgb8"
    pol = dict(min_score_pct=GATE, thickness=16, luma=255, rgb=0xFFFFFF)
    a, tw, seeds = _pair(gpu, weights_tiny, fmt, B, overlay=pol)
    for g in (a, tw):
        g.set_template_refresh(2, 0.0)
        g.enable_chips(64, gpu.CHIP_RGB8)
        g.set_chips(2.0)
        g.set_peaks(4, 2, 0.0)
    drew = refreshed = 0
    for t in range(1, 8):
        bufs = [_clip(gpu, fmt, seeds[s], t)[0] for s in range(B)]
        ua, ut = [Up(gpu, fmt, b) for b in bufs], [Up(gpu, fmt, b) for b in bufs]
        ra, rt = a.update_device([u.frame for u in ua]), tw.update_device([u.frame for u in ut])
        assert [_res(r) for r in ra] == [_res(r) for r in rt]
        assert _states(a) == _states(tw)
        for s in range(B):
            assert np.array_equal(a.read_tensor("template", s), tw.read_tensor("template", s)), f"frame {t}: template of stream {s}"
        ca, ia = a.read_chips()
        ct, it = tw.read_chips()
        assert np.array_equal(ca, ct) and ia == it, f"frame {t}: chips"
        assert a.last_peaks().tobytes() == tw.last_peaks().tobytes(), f"frame {t}: peaks"
        drew += _expect(oracle, ua, ra, **pol)
        for r in ra:
            x, y, w, h = r.bbox
            assert x >= 0 and y >= 0 and x + w < W and y + h < H, "the rectangle is cut by the frame: place the target elsewhere"
        refreshed = sum(a.template_refresh_stats(s)["generation"] for s in range(B))
    assert drew >= 12 and refreshed >= 3, (drew, refreshed)
    a.close()
    tw.close()


def test_host_passes_never_draw(gpu, weights_tiny):
    """synchronous and pipelined host passes leave the caller's buffers alone; the keys are refused while a pipelined pass is
    outstanding, like every key of vt_group_set_tuning"""
    B = 3
    g = gpu.Group(weights_tiny, n_streams=B)
    clips = [[_clip(gpu, "rgb8", s, t)[0].reshape(H, W, 3) for s in range(B)] for t in range(5)]
    for s in range(B):
        g.init_host(s, clips[0][s], gpu.BBox.new(*_clip(gpu, "rgb8", s, 0)[1]))
    g.set_result_overlay(min_score_pct=GATE)
    keep = [[f.copy() for f in fr] for fr in clips]
    g.update_host(clips[1])
    assert all(g.result_overlay_stats(s)["drawn"] == 0 for s in range(B))
    g.enqueue_host(clips[2])
    for key in ro_keys():
        with pytest.raises(gpu.VtError):
            g.set_tuning(key, 1)
    g.enqueue_host(clips[3])
    g.wait_next()
    g.wait_next()
    g.set_tuning("result_overlay_luma", 17)      # collected: accepted again
    for fr, kp in zip(clips, keep):
        for f, k in zip(fr, kp):
            assert np.array_equal(f, k), "a host pass wrote the caller's frame"
    assert all(g.result_overlay_stats(s)["n_drawn"] == 0 and g.result_overlay_stats(s)["drawn"] == 0 for s in range(B))
    # the same engine draws as soon as a pass comes in through a device entry point
    ups = [Up(gpu, "rgb8", clips[4][s]) for s in range(B)]
    res = g.update_device([u.frame for u in ups])
    n = sum(ro.draws(r.success, r.score, GATE) for r in res)
    assert n >= 2 and sum(g.result_overlay_stats(s)["n_drawn"] for s in range(B)) == n
    g.close()


def ro_keys():
    return ("result_overlay", "result_overlay_style", "result_overlay_luma", "result_overlay_rgb", "result_overlay_min_score_pct")


def test_keys_values_and_the_never_enabled_engine(gpu, oracle, weights_tiny):
    B, fmt = 3, "nv12"
    g = gpu.Group(weights_tiny, n_streams=B)
    for s in range(B):
        buf, box = _clip(gpu, fmt, s, 0)
        g.init_device(s, Up(gpu, fmt, buf).frame, gpu.BBox.new(*box))
    frames = lambda t: [Up(gpu, fmt, _clip(gpu, fmt, s, t)[0]) for s in range(B)]
    # never enabled: no read-out, no launch of the family, no capture outside set_tuning
    with pytest.raises(gpu.VtError):
        g.read_tensor("result_overlay", 0)
    caps = g.graph_captures()
    ups = frames(1)
    fams = [k["name"] for k in g.profile_device([u.frame for u in ups], iters=1)]
    assert not [n for n in fams if "overlay" in n], fams
    g.update_device([u.frame for u in frames(2)])
    assert g.graph_captures() == caps
    # style, colour and gate set BEFORE the enable are remembered; flags 0 does not enable
    g.set_tuning("result_overlay_style", 5 | 9 << 8 | 1 << 16)
    g.set_tuning("result_overlay_luma", 180)
    g.set_tuning("result_overlay_min_score_pct", GATE)
    g.set_tuning("result_overlay", 0)
    assert g.graph_captures() == caps
    with pytest.raises(gpu.VtError):
        g.read_tensor("result_overlay", 0)
    g.set_tuning("result_overlay", 3)
    caps2 = g.graph_captures()
    assert caps2 > caps, "the enable did not capture the passes again"
    pol = dict(flags=3, thickness=5, size=9, scale=1, luma=180, min_score_pct=GATE)
    ups = frames(3)
    res = g.update_device([u.frame for u in ups])
    assert _expect(oracle, ups, res, **pol) >= 2
    # bad values and keys: VT_ERR_INVALID_ARG, nothing changes
    for key, v in (("result_overlay", 8), ("result_overlay_style", 0), ("result_overlay_style", 17 | 15 << 8 | 2 << 16),
                   ("result_overlay_style", 3 | 65 << 8 | 2 << 16), ("result_overlay_style", 3 | 15 << 8 | 5 << 16),
                   ("result_overlay_style", 3 | 0 << 8 | 2 << 16), ("result_overlay_luma", 256), ("result_overlay_rgb", 0x1000000),
                   ("result_overlay_min_score_pct", 101), ("result_overlay_colour", 1), ("result_overlays", 1)):
        with pytest.raises(gpu.VtError):
            g.set_tuning(key, v)
    ups = frames(4)
    res = g.update_device([u.frame for u in ups])
    assert _expect(oracle, ups, res, **pol) >= 2
    assert g.result_overlay_stats(0)["flags"] == 3
    # the profiled pass is a device pass: it carries the family, once, and draws
    ups = frames(5)
    prof = {k["name"]: k for k in g.profile_device([u.frame for u in ups], iters=1)}
    assert prof["result_overlay"]["launches"] == 1
    assert any((u.read() != u.buf).any() for u in ups)
    # a negative value selects the default; later changes capture nothing; flags 0 stops the drawing
    g.set_tuning("result_overlay_style", -1)
    g.set_tuning("result_overlay_luma", -1)
    g.set_tuning("result_overlay", 7)
    ups = frames(6)
    res = g.update_device([u.frame for u in ups])
    assert _expect(oracle, ups, res, min_score_pct=GATE) >= 2
    before = [g.result_overlay_stats(s) for s in range(B)]
    g.set_tuning("result_overlay", 0)
    ups = frames(7)
    g.update_device([u.frame for u in ups])
    for u in ups:
        assert np.array_equal(u.read(), u.buf), "flags 0 still draws"
    for s in range(B):
        st = g.result_overlay_stats(s)
        assert st["flags"] == 0 and st["drawn"] == 0 and st["n_drawn"] == before[s]["n_drawn"] and st["n_gated"] == before[s]["n_gated"]
    assert g.graph_captures() == caps2, "a later key captured the passes again"
    g.close()


def test_default_gate_counts_gated_passes(gpu, oracle, weights_tiny):
    """the default gate (score > 0.25) and one at 100: what does not pass is counted and nothing is drawn"""
    B, fmt = 3, "rgb8"
    g = gpu.Group(weights_tiny, n_streams=B)
    for s in range(B):
        buf, box = _clip(gpu, fmt, s, 0)
        g.init_device(s, Up(gpu, fmt, buf).frame, gpu.BBox.new(*box))
    g.set_result_overlay()
    want = {s: [0, 0] for s in range(B)}
    for t, pct in ((1, 25), (2, 25), (3, 100), (4, 100)):
        g.set_tuning("result_overlay_min_score_pct", pct)
        ups = [Up(gpu, fmt, _clip(gpu, fmt, s, t)[0]) for s in range(B)]
        res = g.update_device([u.frame for u in ups])
        _expect(oracle, ups, res, min_score_pct=pct)
        for s in range(B):
            want[s][0 if ro.draws(res[s].success, res[s].score, pct) else 1] += 1
    for s in range(B):
        st = g.result_overlay_stats(s)
        assert [st["n_drawn"], st["n_gated"]] == want[s], (s, st, want[s])
        assert st["n_gated"] >= 2 and st["drawn"] == 0      # nothing exceeds a score of 1
    g.close()


def test_cfg3_1080p_nv12(gpu, oracle, weights_cfg3):
    w, h, B = 1920, 1080, 2
    a, tw = gpu.Group(weights_cfg3, n_streams=B), gpu.Group(weights_cfg3, n_streams=B)
    clip = lambda s, t: gpu.synth.MovingSquare(w, h, 128, seed=s)
    for g in (a, tw):
        for s in range(B):
            sc = clip(s, 0)
            g.init_device(s, Up(gpu, "nv12", sc.frame_nv12(0), w, h).frame, gpu.BBox.new(*sc.gt_box(0)))
    a.set_result_overlay(min_score_pct=GATE)
    drew = 0
    for t in (1, 2):
        bufs = [clip(s, t).frame_nv12(t) for s in range(B)]
        ua, ut = [Up(gpu, "nv12", b, w, h) for b in bufs], [Up(gpu, "nv12", b, w, h) for b in bufs]
        ra, rt = a.update_device([u.frame for u in ua]), tw.update_device([u.frame for u in ut])
        assert [_res(r) for r in ra] == [_res(r) for r in rt] and _states(a) == _states(tw)
        drew += _expect(oracle, ua, ra, min_score_pct=GATE)
    assert drew >= 2
    a.close()
    tw.close()
