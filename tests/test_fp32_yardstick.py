"""The float32 yardstick, CPU side: the committed float32 trajectories are sound, and the bf16
specification's own distance from them is on record.

tests/golden/fp32_traj_*.npz are closed loops of the float32 tracker (oracle/cpu_fp32.py: torch-CPU network, no rounding
emulation) on the clips of the bf16-oracle trajectories traj_*.npz, with one teacher-forced bf16-oracle update on every
recorded float32 state (oracle_fbox / oracle_idx / oracle_score); generator: tests/golden/make_traj.py fp32. The GPU tests
(tests/test_gpu_fp32_yardstick.py) hold the HIP path to these files with bars derived from the oracle's distance recorded
here - not from a HIP run - so a change of the numerical specification made in the oracle and the kernels together still
has to meet them. The fixtures change only with the weights or the clip (weights_sha256 below), never with the kernels."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import iou
from test_gpu_trajectories import MARGIN_EPS, _clip, _fixture, _same_input, _sha256

# float32 fixture -> the bf16-oracle trajectory of the same clip (cfg5: the first 100 frames of its 300)
FP32_TWINS = {"fp32_traj_cfg3_300.npz": "traj_cfg3_300.npz", "fp32_traj_cfg2_300.npz": "traj_cfg2_300.npz",
              "fp32_traj_cfg3_300_b.npz": "traj_cfg3_300_b.npz", "fp32_traj_cfg5_100.npz": "traj_cfg5_300.npz"}
FP32_FIXTURES = list(FP32_TWINS)

# The bf16 oracle against float32, closed loop (both trajectories on their own), MEASURED on the committed fixtures:
# boxes identical, max px, frames below IoU 0.99, frames on another argmax cell, max |score| on frames with the same
# input and cell, max |score| on any frame (0.09 on cfg3_b: the frame whose cell flips)
ORACLE_CLOSED_LOOP = {
    "fp32_traj_cfg3_300.npz": dict(identical=299, px=1, low_iou=1, flips=0, score_same_input=0.0015, score_max=0.0070),
    "fp32_traj_cfg2_300.npz": dict(identical=299, px=1, low_iou=1, flips=0, score_same_input=0.0010, score_max=0.0115),
    "fp32_traj_cfg3_300_b.npz": dict(identical=294, px=1, low_iou=6, flips=1, score_same_input=0.0026, score_max=0.0916),
    "fp32_traj_cfg5_100.npz": dict(identical=89, px=1, low_iou=4, flips=0, score_same_input=0.0047, score_max=0.0692)}
# Teacher-forced (the oracle on every recorded float32 state), frames where both pick the same cell: MEASURED worst
# |oracle float box - float box| per fixture (px) and |oracle score - score| (all fixtures: 0.0047, cfg5)
ORACLE_TF_FBOX_PX = {"fp32_traj_cfg3_300.npz": 0.045, "fp32_traj_cfg2_300.npz": 0.059,
                     "fp32_traj_cfg3_300_b.npz": 0.070, "fp32_traj_cfg5_100.npz": 0.121}
ORACLE_TF_SCORE = 0.0047
# the GPU bars, set from the two lines above by the rule "about 2 x the specification's own distance"
FP32_FBOX_BAR_PX = 0.25
FP32_SCORE_BAR = 0.01
# per frame, on the same cell: |HIP - float32| <= |oracle - float32| + this. HIP and the oracle are themselves up to 0.095 px
# apart on a frame (cfg5, test_gpu_trajectories); measured on MI355X: largest excess 0.052 px (cfg5, 33-stream engine)
TF_FBOX_SLACK_PX = 0.1
# mean |HIP - float32| / mean |oracle - float32| of the float box over a fixture's same-cell frames: measured on MI355X
# 0.96-1.04 (every fixture, both kernel families); with the pair's low byte zero in the kernels 1.06-1.64 (cfg2 - cfg3)
TF_FBOX_MEAN_RATIO = 1.2


def twin(name):
    return _fixture(FP32_TWINS[name])


def run_distance(boxes, succ, scores, idx, fx):
    """a trajectory (boxes [n][4], success flags, scores, argmax cells; n <= the fixture's frames) against the fixture's
    first n frames: the closed-loop distances the GPU bars are made of"""
    n = len(boxes)
    ref = {k: (v[:n] if np.ndim(v) else v) for k, v in fx.items()}
    boxes, succ, scores, idx = np.asarray(boxes), np.asarray(succ).astype(int), np.asarray(scores), np.asarray(idx)
    d = np.abs(boxes - ref["bbox"])
    ious = np.array([iou(tuple(a), tuple(b)) for a, b in zip(boxes, ref["bbox"])])
    same = _same_input(boxes, succ, ref) & (idx == ref["idx"])
    ds = np.abs(scores - ref["score"])
    return dict(px=int(d.max()), identical=int((d.max(axis=1) == 0).sum()), low_iou=int((ious < 0.99).sum()),
                mean_iou=float(ious.mean()), min_iou=float(ious.min()),
                succ_differ=int((succ != ref["success"].astype(int)).sum()), flips=int((idx != ref["idx"]).sum()),
                same_input=int(same.sum()), score_same_input=float(ds[same].max()), score_max=float(ds.max()))


@pytest.mark.parametrize("name", FP32_FIXTURES)
def test_fp32_fixture_is_the_float32_run_on_its_twins_clip(vt, name):
    fx, tw = _fixture(name), twin(name)
    assert str(fx["generator"]) == "fp32" and str(fx["torch_version"]) and int(fx["threads"]) >= 1
    weights = vt.weights.ensure_weights(str(fx["config"]))
    assert _sha256(weights) == str(fx["weights_sha256"]) == str(tw["weights_sha256"]), \
        "the weights changed: regenerate with tests/golden/make_traj.py fp32 (never together with a kernel change)"
    for k in ("config", "frame_w", "frame_h", "square", "seed", "hide"):
        assert np.array_equal(fx[k], tw[k]), k
    n = int(fx["frames"])
    assert n >= 100 and np.array_equal(fx["gt"], tw["gt"][:n])
    for k, shape in (("state", (n, 4)), ("bbox", (n, 4)), ("fbox", (n, 4)), ("oracle_fbox", (n, 4)), ("score", (n,)),
                     ("success", (n,)), ("idx", (n,)), ("idx2", (n,)), ("margin", (n,)), ("oracle_idx", (n,)),
                     ("oracle_score", (n,))):
        assert fx[k].shape == shape, k
    # closed loop: the state of frame t + 1 is the integer box of frame t wherever that one succeeded
    ok = fx["success"][:-1].astype(bool)
    assert np.array_equal(fx["state"][1:][ok], fx["bbox"][:-1][ok].astype(np.float32))


@pytest.mark.parametrize("name", FP32_FIXTURES)
def test_fp32_fixture_reproduces_from_its_recorded_state(vt, oracle, name):
    """a few frames with a clear float32 margin re-evaluated from the recorded state: same cell and integer box, float box
    within 1e-3 px, score within 1e-4 (tolerances, not bits: torch-CPU's reduction order may follow the thread count)"""
    from oracle import cpu_fp32
    fx = _fixture(name)
    weights = vt.weights.ensure_weights(str(fx["config"]))
    clear = np.flatnonzero(fx["margin"] >= MARGIN_EPS)
    frames = [int(clear[0]), int(clear[-1])] if str(fx["config"]) == "cfg5" else \
        [int(clear[0]), int(clear[1]), int(clear[-2]), int(clear[-1])]
    sc = _clip(vt, fx)
    trk = cpu_fp32.VitTrackFp32(weights)
    fr0 = oracle.Frame.nv12(sc.frame_nv12(0), sc.w, sc.h)
    trk.init(fr0, sc.gt_box(0))
    hann = trk.m.t["hann"].reshape(-1)
    for t in frames:
        trk.box = fx["state"][t].astype(np.float32).copy()
        r = trk.update(oracle.Frame.nv12(sc.frame_nv12(t), sc.w, sc.h), taps=True)
        resp = (1.0 / (1.0 + np.exp(-trk.last["head_out"][:, 0].astype(np.float64)))) * hann
        o = np.argsort(-resp, kind="stable")
        assert r.idx == int(fx["idx"][t]) and int(o[1]) == int(fx["idx2"][t]), t
        assert tuple(r.bbox) == tuple(int(v) for v in fx["bbox"][t]), t
        assert np.abs(np.asarray(r.fbox) - fx["fbox"][t]).max() <= 1e-3, t
        assert abs(r.score - float(fx["score"][t])) <= 1e-4 and abs(resp[o[0]] - resp[o[1]] - fx["margin"][t]) <= 1e-4, t
    if str(fx["config"]) != "cfg5":     # the oracle fields on one frame (one bf16-oracle forward: ~1-3 s)
        ref = oracle.VitTrackRef(weights)
        ref.init(fr0, sc.gt_box(0))
        t = frames[-1]
        ref.box = fx["state"][t].astype(np.float32).copy()
        r = ref.update(oracle.Frame.nv12(sc.frame_nv12(t), sc.w, sc.h))
        assert r.idx == int(fx["oracle_idx"][t]) and np.abs(np.asarray(r.fbox) - fx["oracle_fbox"][t]).max() <= 1e-3
        assert abs(r.score - float(fx["oracle_score"][t])) <= 1e-4


def test_the_oracles_distance_from_float32_is_on_record(capsys):
    """the three-way record's first leg, from the committed files only: the bf16 oracle's committed closed loop (traj_*)
    against its float32 twin, and the oracle teacher-forced on the float32 states (oracle_* fields). The GPU bars of
    tests/test_gpu_fp32_yardstick.py are derived from these numbers."""
    worst_f, worst_s = 0.0, 0.0
    for name in FP32_FIXTURES:
        fx, tw = _fixture(name), twin(name)
        n = int(fx["frames"])
        d = run_distance(tw["bbox"][:n], tw["success"][:n], tw["score"][:n], tw["idx"][:n], fx)
        same = fx["oracle_idx"] == fx["idx"]
        df = np.abs(fx["oracle_fbox"] - fx["fbox"]).max(axis=1)
        ds = np.abs(fx["oracle_score"] - fx["score"])
        with capsys.disabled():
            print(f"\n[float32 <-> bf16 oracle, {name}] closed loop, {n} frames: identical boxes {d['identical']}, max "
                  f"{d['px']} px, IoU min {d['min_iou']:.4f} mean {d['mean_iou']:.5f}, frames below 0.99: {d['low_iou']}, "
                  f"success flags differ on {d['succ_differ']}, argmax cell differs on {d['flips']}, |score| max "
                  f"{d['score_max']:.4f} ({d['score_same_input']:.4f} on the {d['same_input']} frames with the same input "
                  f"and cell); teacher-forced: cell differs on {(~same).sum()} frames (float32 margins "
                  f"{np.round(fx['margin'][~same], 4).tolist()}), float box max {df[same].max():.4f} px mean "
                  f"{df[same].mean():.4f} px, |score| max {ds[same].max():.4f} on the same cell")
        rec = ORACLE_CLOSED_LOOP[name]
        assert d["px"] <= rec["px"] and d["identical"] >= rec["identical"] and d["low_iou"] <= rec["low_iou"]
        assert d["flips"] <= rec["flips"] and d["succ_differ"] == 0 and d["mean_iou"] >= 0.99
        assert d["score_same_input"] <= rec["score_same_input"] + 1e-4 and d["score_max"] <= rec["score_max"] + 1e-4
        assert not (~same & (fx["margin"] >= MARGIN_EPS)).any(), "the oracle leaves float32's cell at a clear margin"
        assert df[same].max() <= ORACLE_TF_FBOX_PX[name] + 1e-3 and ds[same].max() <= ORACLE_TF_SCORE + 1e-4
        worst_f, worst_s = max(worst_f, float(df[same].max())), max(worst_s, float(ds[same].max()))
    # the GPU bars follow the rule "about 2 x the specification's own distance", and no looser
    assert 1.5 * worst_f <= FP32_FBOX_BAR_PX <= 2.5 * worst_f and 1.5 * worst_s <= FP32_SCORE_BAR <= 2.5 * worst_s


def test_make_traj_fp32_mode_writes_the_float32_loop_and_the_oracles_distance(vt, oracle, tmp_path):
    """tests/golden/make_traj.py fp32 on three frames of the tiny model: the float32 closed loop, its margins, and the
    bf16 oracle teacher-forced on every recorded state"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_traj", os.path.join(root, "tests", "golden", "make_traj.py"))
    mt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mt)
    out = str(tmp_path / "fp32_traj_tiny_3.npz")
    mt.run_fp32("tiny", 3, 4, out, threads=2)
    with np.load(out) as z:
        fx = {k: z[k] for k in z.files}
    assert str(fx["generator"]) == "fp32" and int(fx["threads"]) == 2 and (fx["margin"] >= 0).all()
    assert not np.array_equal(fx["fbox"], fx["oracle_fbox"])        # two implementations, not one recorded twice
    weights = vt.weights.ensure_weights("tiny")
    sc = vt.synth.MovingSquare(640, 480, 64, seed=4)
    ref = oracle.VitTrackRef(weights)
    for t in range(3):
        f = oracle.Frame.nv12(sc.frame_nv12(t), 640, 480)
        if t == 0:
            ref.init(f, sc.gt_box(0))
        ref.box = fx["state"][t].copy()
        r = ref.update(f)
        assert r.idx == fx["oracle_idx"][t] and np.array_equal(np.float32(r.fbox), fx["oracle_fbox"][t])
        assert np.float32(r.score) == fx["oracle_score"][t]
