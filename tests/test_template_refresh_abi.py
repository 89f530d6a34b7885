"""Template refresh, the part that needs no GPU: the four new functions of include/vittrack_hip.h are exported and bound
(C, ctypes, Rust) with one layout, and the oracle driven through the restated rule (tests/template_refresh_util.py) on the
clips of tests/test_gpu_template_refresh.py - which pins that those clips fire, skip and fail where the GPU tests need
them to, so that their bit-for-bit comparisons are not vacuous."""
import ctypes
import importlib.util
import os
import re
import subprocess

from conftest import iou
from template_refresh_util import OracleTracker, Rule, clip_frames, drive
from test_rust_binding import _size, parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vt_set_template_refresh", "vt_template_refresh_stats", "vt_group_set_template_refresh",
       "vt_group_template_refresh_stats")


def test_the_four_functions_are_exported_and_bound(vt):
    L = ctypes.CDLL(vt.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in vt.EXPORTS
    _, cf = parse_header()
    _, rf, consts = parse_sys_rs()
    for name in NEW:
        assert name in cf and rf[name] == cf[name], name
    assert cf["vt_group_set_template_refresh"] == ("i32", ["ptr", "i32", "i32", "f32"])
    lib_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "lib.rs")).read()
    assert "pub fn set_template_refresh(&mut self, period: i32, min_score: f32)" in lib_rs
    assert "sys::vt_set_template_refresh(" in lib_rs and "sys::vt_group_set_template_refresh(" in lib_rs
    for cls in (vt.Group, vt.VitTrack):
        assert callable(cls.set_template_refresh) and callable(cls.template_refresh_stats)
    # additions only: the version stays
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    assert int(re.search(r"#define VT_ABI_VERSION (\d+)", hdr).group(1)) == 5 and int(consts["VT_ABI_VERSION"]) == 5
    assert L.vt_abi_version() == 5


def test_vt_refresh_stats_is_32_bytes_in_c_ctypes_and_rust(vt):
    assert ctypes.sizeof(vt.CRefreshStats) == 32
    assert [f[0] for f in vt.CRefreshStats._fields_] == ["period", "min_score", "generation", "last_frame",
                                                         "skipped_geometry", "reserved"]
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = subprocess.run([b.build_c_client(), "sizes"], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[0::2], (int(x) for x in out[1::2])))
    assert got["vt_refresh_stats"] == 32 and got["abi"] == 5
    cs, _ = parse_header()
    rs, _, _ = parse_sys_rs()
    assert cs["vt_refresh_stats"] == [("period", "i32", 0), ("min_score", "f32", 0), ("generation", "i32", 0),
                                      ("last_frame", "i32", 0), ("skipped_geometry", "i32", 0), ("reserved", "i32", 3)]
    assert rs["VtRefreshStats"] == cs["vt_refresh_stats"] and _size(rs["VtRefreshStats"], cs) == 32


def test_state_words_keep_the_record_at_88_bytes(vt):
    src = open(os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc", "vt_frame.hpp")).read()
    body = re.search(r"struct StreamState \{(.*?)\n\};", src, flags=re.S).group(1)
    assert "int32_t tpl_gen;" in body and "int32_t tpl_frame;" in body and "pad[" not in body
    assert "static_assert(sizeof(StreamState) == 88" in src


# ---- the oracle under the rule: the clips of the GPU tests ---------------------------------------------------------------

def _oracle_run(vt, weights, n, period, seed=0, step=1, hide=None):
    sc = vt.synth.MovingSquare(640, 480, 64, seed=seed, hide=hide)
    ts, frames = clip_frames(sc, n, step)
    trk = OracleTracker(weights)
    rule = Rule(trk.ref.m.T, trk.ref.m.S, period, 0.0)
    res = drive(trk, frames, sc.gt_box(ts[0]), rule)
    return res, rule, [iou(r.bbox, sc.gt_box(t)) for r, t in zip(res, ts)]


def test_clip_a_fires_every_fifth_update_and_keeps_the_target(vt, oracle, weights_tiny):
    res, rule, gt_iou = _oracle_run(vt, weights_tiny, 60, 5)
    assert rule.fired == list(range(5, 61, 5)) and rule.skipped == []
    assert all(r.success for r in res)
    assert min(gt_iou) > 0.5, min(gt_iou)


def test_clip_b_skips_by_geometry(vt, oracle, weights_tiny):
    res, rule, _ = _oracle_run(vt, weights_tiny, 16, 2, seed=3, step=20)
    assert rule.fired == [3, 5, 7, 9, 11, 14, 16]
    assert rule.skipped == [2, 13]
    assert all(r.success for r in res)


def test_clip_c_does_not_refresh_while_the_target_is_hidden(vt, oracle, weights_tiny):
    res, rule, _ = _oracle_run(vt, weights_tiny, 30, 4, hide=(10, 16))
    assert [i + 1 for i, r in enumerate(res) if not r.success] == list(range(11, 17))
    assert rule.fired == [4, 8, 17, 21, 25, 29] and rule.generation == 6 and rule.last_frame == 29

