"""The decode stage (csrc/k_head.hip: 5-logit layer, Hann-weighted argmax, 3x3 window, box clamps and rounding, success
gate, write-back of StreamState / vt_result / the pinned host mirrors) through vt_op_head_decode, on logits chosen to break
it, against vto_decode (oracle/vt_oracle.c) on the logits the kernels returned. Form 0 is head_out_kernel + decode_kernel,
form 1 the band kernel's fused tail at R = 1, at the launcher's plan and at the largest R with R * grid <= 112.
Cases, references, tolerance and exclusions: tests/decode_util.py (checked on the CPU by tests/test_decode_cases.py)."""
import numpy as np
import pytest

import decode_util as du

pytestmark = pytest.mark.gpu

_W3 = {}


def _configs(grid):
    """(form, R): both kernels, the band kernel at every band height that takes another path"""
    return [(0, 0), (1, 1), (1, 0), (1, du.r_max(grid))]


def _run(gpu, c, form, R, states=None, slot_stream=None, launches=1, **kw):
    t, w4, b4 = c.operands()
    if c.C not in _W3:
        _W3[c.C] = du.identity_conv(c.C)
    w3, b3 = _W3[c.C]
    return gpu.op_head_decode(t, w4, b4, c.hann, c.states if states is None else states, c.n, c.grid, form=form,
                              w3_bf16_bits=w3, b3=b3, slot_stream=slot_stream, success_threshold=c.thr, R=R,
                              launches=launches, **kw)


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _within(got, want, tol):
    """|got - want| <= tol, NaN where and only where the specification has NaN -> (ok, largest distance)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False, np.inf
    d = float(np.abs(got[~nan] - want[~nan]).max()) if (~nan).any() else 0.0
    return d <= tol, d


def _check(c, out, tag, updates=1, smap=None, states_in=None):
    """one hook call against the specification. smap: slot -> stream (states_in: the whole state array then)"""
    tag = f"{tag} grid {c.grid}"
    # the logit layer first: a failure here is not the decode's
    ho = out["head_out"]
    assert du.same_logits(ho[:, :5].reshape(c.n, c.ns, 5), c.logits), tag + ": head_out is not the intended logits"
    assert not ho[:, 5:].any(), tag
    ora, k = c.ora, c.keep
    streams = np.arange(c.n) if smap is None else np.asarray(smap)
    before = c.states if states_in is None else states_in[streams]
    st, res = out["states"][streams], out["results"]
    want_st, want_res = du.expected_states(before, ora, c.thr, updates), du.expected_results(ora, c.thr)
    ok_s, d_s = _within(res["score"], ora["score"], c.tol)
    ok_b, d_b = _within(st["last_fbox"], ora["fbox"], c.tol)
    print(f"{tag}: largest distance from vto_decode: score {d_s:.3e}, float box {d_b:.3e} px (bar {c.tol:.3e})")
    assert np.array_equal(st["last_idx"], ora["idx"]), (tag, st["last_idx"][st["last_idx"] != ora["idx"]][:8])
    assert ok_s and ok_b, (tag, d_s, d_b, c.tol)
    assert _bytes_equal(st["last_score"], res["score"]), tag
    assert np.array_equal(res["success"][k], want_res["success"][k]), tag
    assert np.array_equal(res["bbox"][k], want_res["bbox"][k]), (tag, np.where((res["bbox"] != want_res["bbox"]).any(axis=1) & k)[0][:8])
    # the committed box is the integer box the caller sees, on success only; a failed update keeps box and success_count
    won = res["success"].astype(bool)
    assert np.array_equal(st["box"][won], res["bbox"][won].astype(np.float32)), tag
    assert _bytes_equal(st["box"][~won], before["box"][~won]), tag
    assert np.array_equal(st["box"][k], want_st["box"][k]), tag
    assert np.array_equal(st["frames_done"], before["frames_done"] + updates), tag
    assert np.array_equal(st["success_count"], before["success_count"] + updates * res["success"]), tag
    assert np.array_equal(st["success_count"][k], want_st["success_count"][k]), tag
    # a dropped case may round the other way, by one pixel and no more
    assert np.abs(res["bbox"].astype(np.int64) - want_res["bbox"]).max() <= 1, tag
    for name in du.KEPT:
        assert _bytes_equal(st[name], before[name]), (tag, name)
    # each host mirror is its device copy, bit for bit
    assert _bytes_equal(out["host_results"], out["results"]), tag
    assert _bytes_equal(out["host_states"][streams], st), tag
    assert not out["band_cnt"].any(), (tag, out["band_cnt"])


def _check_all_forms(gpu, c, name):
    outs = []
    for form, R in _configs(c.grid):
        out = _run(gpu, c, form, R)
        _check(c, out, f"{name} form {form} R {R}")
        outs.append(out)
    for (form, R), out in zip(_configs(c.grid)[1:], outs[1:]):      # the two kernels agree bit for bit on the same logits
        for key in ("results", "states", "host_results", "host_states"):
            assert _bytes_equal(out[key], outs[0][key]), (name, form, R, key)
    return outs[0]


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_every_cell_as_the_argmax(gpu, oracle, grid, C):
    """one stream per cell: borders and corners (windows of 6 and 4 cells), every band of the fused tail handing its
    logits to whichever workgroup arrives last, boxes clamped at every frame edge"""
    c = du.sweep(grid, C)
    out = _check_all_forms(gpu, c, "sweep")
    assert np.array_equal(out["states"]["last_idx"], np.arange(grid * grid))


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_ties_decode_the_lowest_cell(gpu, oracle, grid, C):
    """exact ties: inside one 64-lane stride, 64 cells apart, across bands, first and last cell, all cells, the map's last
    cell against the short band's padding positions (which repeat it), and the saturated head under the real window"""
    flat, real = du.ties(grid, C)
    out = _check_all_forms(gpu, flat, "ties, flat window")
    want = [min(cells) for cells in du.tie_sets(grid).values()]
    assert out["states"]["last_idx"].tolist() == want
    out = _check_all_forms(gpu, real, "ties, saturated head")
    assert out["results"]["score"][0] == np.float32(1.0)


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_score_at_the_threshold_and_a_failed_update(gpu, oracle, grid, C):
    at = du.threshold_cases(grid, C, 0.5)
    out = _check_all_forms(gpu, at, "score == threshold")
    assert np.all(out["results"]["score"] == np.float32(0.5)) and np.all(out["results"]["success"] == 1)
    above = du.threshold_cases(grid, C, du.THR_ABOVE_HALF)
    out = _check_all_forms(gpu, above, "threshold one float above the score")
    st, was = out["states"], above.states
    assert np.all(out["results"]["success"] == 0)
    assert _bytes_equal(st["box"], was["box"]) and _bytes_equal(st["success_count"], was["success_count"])
    assert np.array_equal(st["frames_done"], was["frames_done"] + 1) and np.all(st["last_score"] == np.float32(0.5))
    assert np.array_equal(st["last_idx"], above.ora["idx"]) and not _bytes_equal(st["last_fbox"], was["last_fbox"])


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_boxes_clamped_at_every_edge_and_at_the_minimum(gpu, oracle, grid, C):
    c = du.clamp_cases(grid, C)
    out = _check_all_forms(gpu, c, "clamps")
    box = dict(zip(c.names, out["results"]["bbox"].tolist()))
    assert box["top-left"] == [0, 0, 10, 10] and box["bottom-right"] == [630, 470, 10, 10]
    assert box["top-right"] == [630, 0, 10, 10] and box["bottom-left"] == [0, 470, 10, 10]
    assert box["smaller than 10 px"][2:] == [10, 10] and box["larger than the frame"] == [0, 0, 640, 480]


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_non_finite_logits(gpu, oracle, grid, C):
    """NaN and +-inf are ordinary float arithmetic: the specification's cell, score, box and state, last_idx included -
    where no cell has a comparable response (every score logit NaN) that is cell 0, not the reductions' start value"""
    c = du.nonfinite_cases(grid, C)
    out = _check_all_forms(gpu, c, "non-finite")
    k = c.names.index("all nan")
    assert out["states"]["last_idx"][k] == 0 and np.isnan(out["results"]["score"][k]) and out["results"]["success"][k] == 0
    assert out["results"]["bbox"][k].tolist() == [0, 0, 10, 10]
    k = c.names.index("all -inf")
    assert out["states"]["last_idx"][k] == 0 and out["results"]["score"][k] == 0.0


def _subset(c, cells):
    """the cases `cells` of a set as a set of their own (references recomputed: a handful of cases)"""
    cells = np.asarray(cells)
    s = du.Cases(c.grid, c.C, c.logits[cells], c.hann, c.states[cells].copy(), c.thr, [c.names[i] for i in cells], tol=c.tol)
    assert np.array_equal(s.keep, c.keep[cells])
    return s


@pytest.mark.parametrize("grid,C", [(13, 64), (16, 128)])
def test_subset_pass_results_by_slot_states_by_stream(gpu, oracle, grid, C):
    full = du.sweep(grid, C)
    ns = grid * grid
    c = _subset(full, [0, grid - 1, ns // 2 + 3, ns - grid, ns - 1])
    smap = np.array([7, 2, 8, 0, 4], np.int32)
    states = du.make_states(np.tile(np.array([5.0, 6.0, 7.0, 8.0], np.float32), (9, 1)), np.full(9, 320, np.int32),
                            np.full(9, 240, np.int32), 77)
    states[smap] = c.states
    unlisted = np.setdiff1d(np.arange(9), smap)
    for form, R in _configs(grid):
        out = _run(gpu, c, form, R, states=states, slot_stream=smap)
        _check(c, out, f"subset form {form} R {R}", smap=smap, states_in=states)
        assert _bytes_equal(out["states"][unlisted], states[unlisted])              # all 88 bytes
        assert np.all(out["host_states"][unlisted].view(np.uint8) == 0xA5)            # the mirror is indexed by stream too
        # either mirror may be null: the other one and the device copies are written all the same
        for flag in ("host_results", "host_states"):
            o2 = _run(gpu, c, form, R, states=states, slot_stream=smap, **{flag: False})
            assert np.all(o2[flag].view(np.uint8) == 0xA5), (form, R, flag)
            for key in ("results", "states", "host_results", "host_states"):
                if key != flag:
                    assert _bytes_equal(o2[key], out[key]), (form, R, flag, key)


def test_hand_off_with_more_workgroups_than_cus_and_a_second_launch(gpu, oracle):
    """grid 24 at R = 1 with 11 streams: 264 workgroups of one per CU on 256 CUs, so some stream's last band arrives in a
    later round; two launches on the same counters: they must have come back to zero by themselves"""
    full = du.sweep(24, 128)
    c = _subset(full, [0, 23, 24, 47, 100, 287, 300, 301, 552, 553, 575])
    one = _run(gpu, c, 1, 1)
    _check(c, one, "hand-off, one launch")
    two = _run(gpu, c, 1, 1, launches=2)
    _check(c, two, "hand-off, two launches", updates=2)
    assert not two["band_cnt"].any()
    assert np.array_equal(two["states"]["frames_done"], c.states["frames_done"] + 2)
    assert _bytes_equal(two["results"], one["results"])         # geo is not the decode's to write: the same inputs twice
    for name in ("box", "last_idx", "last_fbox", "last_score"):
        assert _bytes_equal(two["states"][name], one["states"][name]), name
    ref = _run(gpu, c, 0, 0, launches=2)
    assert _bytes_equal(ref["states"], two["states"]) and _bytes_equal(ref["results"], two["results"])


def test_what_the_launchers_refuse_is_an_error_code(gpu, oracle):
    c = _subset(du.sweep(16, 128), [5])
    t, w4, b4 = c.operands()
    w3, b3 = du.identity_conv(128)

    def refused(**kw):
        args = dict(form=1, w3_bf16_bits=w3, b3=b3, R=1)
        args.update(kw)
        tt, ww4, grid = args.pop("t", t), args.pop("w4", w4), args.pop("grid", 16)
        states, B = args.pop("states", c.states), args.pop("B", 1)
        hann = np.ones(grid * grid, np.float32)
        with pytest.raises(gpu.VtError) as e:
            gpu.op_head_decode(tt, ww4, b4, hann, states, B, grid, **args)
        assert e.value.code == -1, e.value      # VT_ERR_INVALID_ARG

    refused(R=8)                                                                    # 8 * 16 = 128 cells > 112
    refused(slot_stream=np.array([1], np.int32))                                    # one state, stream 1
    refused(slot_stream=np.array([-1], np.int32))
    refused(launches=0)
    refused(form=2)
    w3_96 = np.zeros((96, 9 * 96), np.uint16)
    refused(t=np.zeros((256, 96), np.uint16), w4=np.zeros((8, 96), np.float32), w3_bf16_bits=w3_96, b3=np.zeros(96, np.float32))
    refused(t=np.zeros((100 * 100, 128), np.uint16), grid=100)                      # no band of a 100-cell row fits LDS
    two = np.concatenate([c.states, c.states])
    refused(t=np.concatenate([t, t]), B=2, states=two, slot_stream=np.array([1, 1], np.int32))     # one state, two writers
    refused(t=np.concatenate([t, t]), B=2)                                          # two slots, one state
    _check(c, _run(gpu, c, 1, 1), "after the refusals")                             # and the library is as it was
