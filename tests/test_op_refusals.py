"""What the in-the-pass operator hooks (csrc/vt_ops.hip) refuse, and in which words: the slot maps, the winner tables, the
policy words and one range case per hook that keeps its own check. Every refusal comes before the hook looks for a device,
and every call names device 1 << 20: a case that is not refused ends in VT_ERR_NO_DEVICE, never in a launch. So no case
needs a GPU or starts work on one. The frames carry a made-up plane address that nothing dereferences."""
import numpy as np
import pytest

DEVICE = 1 << 20
INVALID, NO_DEVICE = -1, -2
NORM = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)
T, PATCH, KPAD = 16, 16, 768        # one template token of 3 * 16 * 16 columns

# the policy words of the five hooks that read them through a key table (csrc/vt_feature_keys.hpp), written out:
# (the wrapper's parameter, key, word, lo, hi)
TABLES = {
    "motion_prior": [("on", "motion_prior", 0, 0, 1), ("gain_pct", "motion_gain_pct", 1, 1, 100), ("coast", "motion_coast", 2, 0, 60),
                     ("max_pct", "motion_max_pct", 3, 0, 200)],
    "camera_motion": [("mode", "camera_motion", 0, 0, 2), ("cell", "camera_motion_cell", 1, 0, 32), ("rng", "camera_motion_range", 2, 2, 16),
                      ("conf_pm", "camera_motion_conf_pm", 3, 0, 1000), ("max_cells", "camera_motion_max_cells", 4, 4096, 1048576)],
    "frame_health": [("on", "health", 0, 0, 1), ("period", "health_period", 1, 1, 1000000), ("cell", "health_cell", 2, 0, 32),
                     ("still_run", "health_still_run", 3, 1, 1000), ("flat_q", "health_flat_q", 4, 0, 4080),
                     ("cut_pm", "health_cut_pm", 5, 0, 1000), ("gate", "health_gate", 6, 0, 1),
                     ("max_cells", "health_max_cells", 7, 4096, 262144)],
    "arbitrate": [("on", "arbitrate", 0, 0, 1), ("max_peaks", "arbitrate_max", 1, 2, 4), ("radius", "arbitrate_radius", 2, 1, 4),
                  ("min_resp_pm", "arbitrate_min_resp_pm", 3, 0, 1000), ("low_pm", "arbitrate_low_pm", 4, 0, 1000),
                  ("high_pm", "arbitrate_high_pm", 5, 0, 1000)],
    "stream_conflicts": [("on", "conflicts", 0, 0, 1), ("iou_pm", "conflicts_iou_pm", 1, 1, 1000), ("gate", "conflicts_gate", 2, 0, 1)],
}
# which hooks take which operand, and what they call the records a slot's stream indexes
MAPPED = {"head_decode": "states", "response_peaks": "states", "result_overlay": "streams", "motion_prior": "streams",
          "proposals": "streams", "camera_motion": "streams", "arbitrate": "streams", "frame_health": "streams",
          "stream_conflicts": "streams"}
WINNERS = ("response_peaks", "result_overlay", "motion_prior", "proposals", "arbitrate", "stream_conflicts")


def _call(vt, hook, n, n_streams, **kw):
    """the hook's wrapper on the smallest legal operands of n slots and n_streams streams, kw on top"""
    st = np.zeros(n_streams, vt.snapshot.STATE)
    res = np.zeros(n, vt.RESULT_DTYPE)
    frames = [vt.CFrame(plane0=0x10000, width=16, height=16, stride0=48, format=vt.PIX_RGB8) for _ in range(n)]
    ho, hann = np.zeros((n, 8), np.float32), np.ones(1, np.float32)      # a 1 x 1 grid
    if hook == "head_decode":
        return vt.op_head_decode(np.zeros((n, 2), np.uint16), np.zeros((8, 2), np.float32), np.zeros(8, np.float32), hann, st, n, 1,
                                 device=DEVICE, **kw)
    if hook == "response_peaks":
        return vt.op_response_peaks(ho, hann, st, kw.pop("policies", (2, 1, 0.0)), n, 1, device=DEVICE, **kw)
    if hook == "result_overlay":
        return vt.op_result_overlay(frames, res, n_streams=n_streams, device=DEVICE, **kw)
    if hook == "motion_prior":
        if "winner" in kw:      # the candidate form: the map is the slots' streams
            cd = np.zeros(n, vt.CANDIDATE_DTYPE)
            cd["stream"] = kw.pop("slot_stream", np.arange(n) % n_streams)
            kw["cands"] = cd
        return vt.op_motion_prior(st, np.zeros(n_streams, vt.MOTION_REC_DTYPE), res, device=DEVICE, **kw)
    if hook == "proposals":
        kw.setdefault("max_cells", 256)
        return vt.op_proposals(frames, st, res, np.zeros((n_streams, 1, 1, KPAD), np.uint16), T, PATCH, NORM, device=DEVICE, **kw)
    if hook == "camera_motion":
        kw.setdefault("max_cells", 4096)
        return vt.op_camera_motion(frames, st, device=DEVICE, **kw)
    if hook == "frame_health":
        kw.setdefault("max_cells", 4096)
        return vt.op_frame_health(frames, st, device=DEVICE, **kw)
    if hook == "arbitrate":
        return vt.op_arbitrate(ho, hann, frames, st, res, np.zeros((n_streams, 1, KPAD), np.uint16), 1, T, 2 * T, PATCH, NORM, 0.5,
                               device=DEVICE, **kw)
    assert hook == "stream_conflicts"
    return vt.op_stream_conflicts(st, res, np.zeros(n_streams, np.int32), device=DEVICE, **kw)


def _cases():
    out = []        # (hook, n, n_streams, kw, text)
    for hook, noun in MAPPED.items():
        out.append((hook, 3, 2, {}, f"{hook}: 2 {noun} for 3 slots"))
        out.append((hook, 2, 1, {}, f"{hook}: 1 {noun} for 2 slots"))
        out.append((hook, 2, 2, dict(slot_stream=[0, -1]), f"{hook}: slot 1 names stream -1 of 2"))
        out.append((hook, 3, 2, dict(slot_stream=[1, 0, 2]), f"{hook}: slot 2 names stream 2 of 2"))
        out.append((hook, 1, 1, dict(slot_stream=[1]), f"{hook}: slot 0 names stream 1 of 1"))
    for hook in WINNERS:
        out.append((hook, 2, 2, dict(winner=[0, 2]), f"{hook}: winner[1] = 2 of 2 slots"))
        out.append((hook, 1, 1, dict(winner=[-1]), f"{hook}: winner[0] = -1 of 1 slots"))
        out.append((hook, 3, 2, dict(slot_stream=[1, 0, 1], winner=[3, 0, 0]), f"{hook}: winner[0] = 3 of 3 slots"))
    # no stream has two writers: the decode always, the arbitration outside a candidate pass
    out.append(("head_decode", 2, 2, dict(slot_stream=[1, 1]), "head_decode: stream 1 listed twice"))
    out.append(("head_decode", 3, 3, dict(slot_stream=[2, 0, 2]), "head_decode: stream 2 listed twice"))
    out.append(("arbitrate", 2, 2, dict(slot_stream=[1, 1]), "arbitrate: stream 1 is named by two slots"))
    out.append(("arbitrate", 3, 2, dict(slot_stream=[0, 1, 0]), "arbitrate: stream 0 is named by two slots"))
    for hook, rows in TABLES.items():
        for name, key, word, lo, hi in rows:        # one past each bound; lo - 1 == -1: a negative word, which no hook takes
            for v in (lo - 1, hi + 1):
                out.append((hook, 2, 2, {name: v}, f"{hook}: policy word {word} ({key}) = {v} refused"))
        name, key, word = rows[2][:3]
        out.append((hook, 1, 1, {name: -7}, f"{hook}: policy word {word} ({key}) = -7 refused"))
        a, b = rows[1], rows[-1]                     # two bad words: the lower row is named
        out.append((hook, 1, 1, {a[0]: a[4] + 1, b[0]: b[4] + 1}, f"{hook}: policy word {a[2]} ({a[1]}) = {a[4] + 1} refused"))
    out.append(("camera_motion", 1, 1, dict(cell=5), "camera_motion: policy word 1 (camera_motion_cell) = 5 refused"))
    out.append(("frame_health", 1, 1, dict(cell=5), "frame_health: policy word 2 (health_cell) = 5 refused"))
    # the policy is refused before the maps
    out.append(("stream_conflicts", 2, 2, dict(iou_pm=0, slot_stream=[0, 2]), "stream_conflicts: policy word 1 (conflicts_iou_pm) = 0 refused"))
    out.append(("camera_motion", 2, 2, dict(rng=17, slot_stream=[0, 2]), "camera_motion: policy word 2 (camera_motion_range) = 17 refused"))
    # the three hooks with range checks of their own
    out.append(("result_overlay", 1, 1, dict(thickness=17), "result_overlay: policy out of range"))
    out.append(("result_overlay", 1, 1, dict(scale=0), "result_overlay: policy out of range"))
    out.append(("proposals", 1, 1, dict(max_n=9), "proposals: policy out of range"))
    out.append(("proposals", 1, 1, dict(max_cells=255), "proposals: policy out of range"))
    out.append(("response_peaks", 2, 2, dict(policies=(2, 5, 0.0)), "response_peaks: policy 0: max_peaks 2, radius 5"))
    return out


CASES = _cases()


@pytest.mark.parametrize("hook,n,n_streams,kw,text", CASES,
                         ids=[f"{c[0]}-{c[1]}x{c[2]}-" + "-".join(f"{k}={v}" for k, v in c[3].items()).replace(" ", "") for c in CASES])
def test_refusal(vt, hook, n, n_streams, kw, text):
    with pytest.raises(vt.VtError) as ei:
        _call(vt, hook, n, n_streams, **dict(kw))
    assert ei.value.code == INVALID, str(ei.value)
    assert str(ei.value) == f"vittrack_hip error {INVALID}: {text}"


@pytest.mark.parametrize("hook", list(MAPPED))
def test_legal_operands_reach_the_device_check(vt, hook):
    """the base operands of the cases above are legal: what stops them is the made-up device, and nothing before it"""
    with pytest.raises(vt.VtError) as ei:
        _call(vt, hook, 2, 2, slot_stream=[1, 0])
    assert ei.value.code == NO_DEVICE, str(ei.value)
