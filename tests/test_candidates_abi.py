"""Candidate passes, the part that needs no GPU: the three new functions of include/vittrack_hip.h are exported and
bound (C, ctypes, Rust) with one layout, vt_scan_windows tiles a frame as the header says, and the committed
re-acquisition fixtures (tests/golden/make_reacquire.py) keep the conditions that stop the GPU test
(tests/test_gpu_candidates.py) from being vacuous."""
import ctypes
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

from test_rust_binding import _size, parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vt_group_update_device_candidates", "vt_group_update_host_candidates", "vt_scan_windows")


def test_the_three_functions_are_exported_and_bound(vt):
    L = ctypes.CDLL(vt.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in vt.EXPORTS
    _, cf = parse_header()
    _, rf, _ = parse_sys_rs()
    for name in NEW:
        assert name in cf and rf[name] == cf[name], name
    lib_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "lib.rs")).read()
    assert "pub unsafe fn group_reacquire_host(" in lib_rs and "sys::vt_group_update_host_candidates(" in lib_rs


def test_vt_candidate_is_24_bytes_in_c_ctypes_and_rust(vt):
    assert ctypes.sizeof(vt.CCandidate) == 24
    assert [f[0] for f in vt.CCandidate._fields_] == ["stream", "has_box", "box"]
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = subprocess.run([b.build_c_client(), "sizes"], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[0::2], (int(x) for x in out[1::2])))
    assert got["vt_candidate"] == 24
    cs, _ = parse_header()
    rs, _, _ = parse_sys_rs()
    assert cs["vt_candidate"] == [("stream", "i32", 0), ("has_box", "i32", 0), ("box", "f32", 4)]
    assert rs["VtCandidate"] == cs["vt_candidate"] and _size(rs["VtCandidate"], cs) == 24


# ---- vt_scan_windows against a restatement -------------------------------------------------------------------------

def _axis(L, side, stride):
    if L <= side:
        return [L / 2.0]
    n = int(math.ceil((L - side) / stride)) + 1
    return [side / 2.0 + i * (L - side) / (n - 1) for i in range(n)]


def _restated(w, h, bw, bh, overlap):
    side = 4.0 * math.sqrt(float(bw) * float(bh))
    stride = side * (100 - overlap) / 100.0
    return np.array([(cx - bw / 2.0, cy - bh / 2.0, bw, bh) for cy in _axis(float(h), side, stride)
                     for cx in _axis(float(w), side, stride)], np.float64), side, stride


@pytest.mark.parametrize("w,h,bw,bh,overlap,count", [(1920, 1080, 64, 64, 50, 112), (640, 480, 48, 48, 50, 24),
                                                     (1920, 1080, 80, 50, 50, None), (3840, 2160, 160, 160, 25, None),
                                                     (1280, 720, 33.5, 71.25, 0, None), (640, 480, 64, 64, 90, None)])
def test_scan_windows_matches_its_definition(vt, w, h, bw, bh, overlap, count):
    got = vt.scan_windows(w, h, bw, bh, overlap)
    want, side, stride = _restated(w, h, bw, bh, overlap)
    if count is not None:
        assert len(got) == count
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.abs(got.astype(np.float64) - want).max() <= 1e-3
    # windows flush with the frame edges, spacing never above the stride, boxes of the requested size
    cx, cy = got[:, 0] + got[:, 2] / 2.0, got[:, 1] + got[:, 3] / 2.0
    assert abs(cx.min() - side / 2) <= 1e-3 and abs(cx.max() + side / 2 - w) <= 1e-3
    assert abs(cy.min() - side / 2) <= 1e-3 and abs(cy.max() + side / 2 - h) <= 1e-3
    ux, uy = np.unique(np.round(cx, 3)), np.unique(np.round(cy, 3))
    assert len(ux) * len(uy) == len(got)
    assert np.diff(ux).max() <= stride + 1e-3 and np.diff(uy).max() <= stride + 1e-3
    assert np.all(got[:, 2] == np.float32(bw)) and np.all(got[:, 3] == np.float32(bh))
    # row by row, y outer
    assert np.all(np.diff(cy) >= -1e-3) and np.allclose(cx[:len(ux)], ux, atol=2e-3)


def test_scan_windows_small_frames_caps_and_bad_arguments(vt):
    L = vt.lib()
    one = vt.scan_windows(200, 120, 64, 64)             # the frame is smaller than one window: one centred window
    assert one.shape == (1, 4) and np.allclose(one[0], [100 - 32, 60 - 32, 64, 64])
    wide = vt.scan_windows(1920, 200, 64, 64)           # one row of windows
    assert len(wide) == 14 and np.allclose(wide[:, 1], 100 - 32)
    # cap smaller than the count: the count is returned, only `cap` boxes are written
    buf = np.full((6, 4), -7.0, np.float32)
    n = L.vt_scan_windows(1920, 1080, 64.0, 64.0, 50, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 5)
    assert n == 112 and np.array_equal(buf[:5], vt.scan_windows(1920, 1080, 64, 64)[:5]) and np.all(buf[5] == -7.0)
    assert L.vt_scan_windows(1920, 1080, 64.0, 64.0, 50, None, 0) == 112
    nan, inf = float("nan"), float("inf")
    for bad in [(1920, 1080, 64, 64, -1), (1920, 1080, 64, 64, 91), (15, 1080, 64, 64, 50), (1920, 15, 64, 64, 50),
                (1920, 1080, 0.5, 64, 50), (1920, 1080, 64, 0.5, 50), (1920, 1080, 40000, 64, 50),
                (1920, 1080, nan, 64, 50), (1920, 1080, 64, inf, 50)]:
        assert L.vt_scan_windows(bad[0], bad[1], bad[2], bad[3], bad[4], None, 0) == 0, bad
        with pytest.raises(ValueError):
            vt.scan_windows(*bad)


# ---- the committed fixtures -----------------------------------------------------------------------------------------

def _generator():
    spec = importlib.util.spec_from_file_location("make_reacquire", os.path.join(ROOT, "tests", "golden", "make_reacquire.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.mark.parametrize("cfg", ["cfg2", "cfg3"])
def test_reacquire_fixture_keeps_the_gpu_test_honest(vt, cfg):
    gen = _generator()
    with np.load(os.path.join(ROOT, "tests", "golden", f"reacquire_{cfg}.npz")) as z:
        fx = {k: z[k] for k in z.files}
    assert str(fx["config"]) == cfg
    assert gen.sha256_file(vt.weights.ensure_weights(cfg)) == str(fx["weights_sha256"]), "fixture made with other weights"
    thr = float(fx["threshold"])
    # no oracle slot score within 0.05 of the success threshold
    assert np.abs(fx["slot_score"] - thr).min() > 0.05
    assert np.array_equal(fx["slot_success"] != 0, fx["slot_score"] >= thr)
    # at least one succeeding slot, whose box is within 1 px of the ground truth
    ok = fx["slot_success"] != 0
    assert ok.any() and np.abs(fx["slot_bbox"][ok] - fx["gt_jump"][None, :]).max() <= 1
    # the plain update fails
    assert int(fx["plain_success"]) == 0 and float(fx["plain_score"]) < thr - 0.05
    # the oracle keeps IoU > 0.5 against the ground truth on all 20 tracked frames
    ious = [gen.iou(tuple(b), tuple(g)) for b, g in zip(fx["track_bbox"], fx["track_gt"])]
    assert len(ious) == 20 and min(ious) > 0.5 and np.all(fx["track_success"] != 0)
    # the scan: the library's grid, chunks of 30, winners by the rule, the stop chunk the first that succeeds
    boxes = vt.scan_windows(int(fx["frame_w"]), int(fx["frame_h"]), float(fx["state_before"][2]), float(fx["state_before"][3]))
    assert len(boxes) == 112 and np.abs(boxes - fx["boxes"]).max() <= 1e-3
    chunk, stop = int(fx["chunk"]), int(fx["stop_chunk"])
    assert chunk == 30 and len(fx["slot_score"]) == min((stop + 1) * chunk, len(boxes)) and len(fx["chunk_winner"]) == stop + 1
    for c, wi in enumerate(fx["chunk_winner"]):
        sc = fx["slot_score"][c * chunk:(c + 1) * chunk]
        assert int(wi) == c * chunk + int(np.argmax(sc)), f"chunk {c}"      # argmax: the first maximum
        assert bool(fx["slot_success"][wi]) == (c == stop)
    gen.check(fx)
    # the clip is the one the GPU test replays
    _, gt = gen.clip()
    assert tuple(fx["gt_jump"]) == tuple(gt(int(fx["jump_at"]))) and np.array_equal(fx["track_gt"][0], gt(int(fx["jump_at"]) + 1))
