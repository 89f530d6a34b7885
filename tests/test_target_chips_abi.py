"""Target chips, the part that needs no GPU: the seven new functions of include/vittrack_hip.h are exported and bound (C,
ctypes, Rust) with one layout; the numpy restatement of the chip (tests/target_chips_util.py) equals the oracle bit for bit;
and the oracle tracker driven under the restated gate on the clips of tests/test_gpu_target_chips.py - which pins which
updates cut, skip by geometry and fail there, so that the GPU tests' bit-for-bit comparisons are not vacuous. The pinned
numbers are the oracle's alone (measured on the CPU)."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

import target_chips_util as u
from template_refresh_util import clip_frames
from test_rust_binding import _size, parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vt_group_enable_chips", "vt_group_set_chips", "vt_group_read_chips", "vt_group_chips_device", "vt_enable_chip",
       "vt_set_chip", "vt_read_chip")
INFO = [("status", "i32", 0), ("frames_done", "i32", 0), ("success", "i32", 0), ("score", "f32", 0), ("box", "i32", 4),
        ("geo", "f32", 3), ("reserved", "i32", 1)]

# the clips of the GPU tests: MovingSquare(640, 480, 64, ...) keyword arguments, updates, every step-th clip frame
CLIPS = {"a": (dict(seed=0), 12, 1), "b": (dict(seed=3), 12, 20), "c": (dict(seed=0, hide=(10, 16)), 18, 1)}


def test_the_seven_functions_are_exported_and_bound(vt):
    L = ctypes.CDLL(vt.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in vt.EXPORTS
    _, cf = parse_header()
    _, rf, consts = parse_sys_rs()
    for name in NEW:
        assert name in cf and rf[name] == cf[name], name
    assert cf["vt_group_enable_chips"] == ("i32", ["ptr", "i32", "i32", "ptr", "ptr"])
    assert cf["vt_group_set_chips"] == ("i32", ["ptr", "i32", "f32", "i32", "i32"])
    assert cf["vt_group_read_chips"] == ("i32", ["ptr", "ptr", "i32", "ptr", "usize", "ptr"])
    assert cf["vt_group_chips_device"] == ("i32", ["ptr", "ptr", "ptr", "ptr"])
    lib_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "lib.rs")).read()
    for needle in ("pub fn enable_chip(&mut self, size: i32, kind: i32, norm_a: &[f32; 3], norm_b: &[f32; 3])",
                   "pub fn set_chip(&mut self, factor: f32, period: i32, phase: i32)", "pub fn read_chip(&mut self,",
                   "sys::vt_enable_chip(", "sys::vt_set_chip(", "sys::vt_read_chip(", "sys::vt_group_set_chips("):
        assert needle in lib_rs, needle
    for cls in (vt.Group, vt.VitTrack):
        for m in ("enable_chips", "set_chips", "read_chips", "chips_device"):
            assert callable(getattr(cls, m)), m
    assert (vt.CHIP_NORM_BF16, vt.CHIP_RGB8) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    assert re.search(r"VT_CHIP_NORM_BF16 = 0, VT_CHIP_RGB8 = 1", hdr)
    # additions only: the version stays
    assert int(re.search(r"#define VT_ABI_VERSION (\d+)", hdr).group(1)) == 5 and int(consts["VT_ABI_VERSION"]) == 5
    assert L.vt_abi_version() == 5


def test_vt_chip_info_is_48_bytes_in_c_ctypes_and_rust(vt):
    assert ctypes.sizeof(vt.CChipInfo) == 48
    assert [f[0] for f in vt.CChipInfo._fields_] == [f[0] for f in INFO]
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = subprocess.run([b.build_c_client(), "sizes"], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[0::2], (int(x) for x in out[1::2])))
    assert got["vt_chip_info"] == 48 and got["abi"] == 5
    cs, _ = parse_header()
    rs, _, _ = parse_sys_rs()
    assert cs["vt_chip_info"] == INFO
    assert rs["VtChipInfo"] == cs["vt_chip_info"] and _size(rs["VtChipInfo"], cs) == 48


def test_the_stream_state_is_untouched_and_the_kernel_is_built_like_the_crop_kernels():
    src = open(os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc", "vt_frame.hpp")).read()
    assert "static_assert(sizeof(StreamState) == 88" in src
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "k_chip.hip" in b.HIP_SOURCES and "k_chip.hip" not in b.FAST_CONTRACT      # -ffp-contract=off


# ---- the restatement against the oracle -------------------------------------------------------------------------------------

BOXES = [(288, 208, 64, 64), (300, 200, 41, 77), (5, 3, 50, 40), (600, 440, 30, 30), (100, 100, 333, 201),
         (250, 180, 100, 70), (-20, 400, 90, 120)]


def test_restated_chip_equals_vto_preproc_bit_for_bit(vt, oracle):
    """boxes in the middle, in the corners (black taps) and over the edge; factors over the allowed range; sizes of both
    kernel bodies (multiples of 64 and not), on an even and on an odd-width frame"""
    sc = vt.synth.MovingSquare(640, 480, 64, seed=1)
    rgb = sc.frame_rgb8(0)
    n = 0
    for img in (rgb, np.ascontiguousarray(rgb[:, :637])):
        fr = oracle.Frame.rgb8(img)
        for box in BOXES:
            for factor in (0.5, 1.0, 2.0, 3.3, 4.0):
                for C in (32, 40, 64, 200):
                    got = u.chip_bf16(u.bilinear(img, box, factor, C), (1, 1, 1), (0, 0, 0))
                    want = u.oracle_chip_bf16(fr, box, factor, C, (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
                    assert np.array_equal(got, want), (img.shape, box, factor, C)
                    n += 1
    assert n == 2 * 7 * 5 * 4
    # the caller's norms: the one multiply-add of the body, on the restated v
    a, b = (1 / 58.395, 1 / 57.12, 1 / 57.375), (-2.1179, -2.0357, -1.8044)
    got = u.chip_bf16(u.bilinear(rgb, BOXES[1], 2.0, 40), a, b)
    assert np.array_equal(got, u.oracle_chip_bf16(oracle.Frame.rgb8(rgb), BOXES[1], 2.0, 40, a, b))


def test_u8_rounding_is_round_half_to_even_and_saturates():
    v = np.array([[[0.5, 1.5, 2.5, 254.5, 255.49, 255.5, 300.0, -0.4, -3.0, 127.49999]]] * 3, np.float32)
    want = [0, 2, 2, 254, 255, 255, 255, 0, 0, 127]
    assert u.chip_u8(v).shape == (1, 10, 3)
    assert u.chip_u8(v)[0, :, 0].tolist() == want and u.chip_u8(v)[0, :, 2].tolist() == want
    # a flat frame: every in-frame bilinear value is the pixel itself, so the u8 chip is the frame's colour and black outside
    img = np.full((48, 64, 3), (10, 200, 77), np.uint8)
    chip = u.chip_u8(u.bilinear(img, (0, 0, 20, 20), 2.0, 32))
    assert chip.shape == (32, 32, 3) and (chip[-1, -1] == (10, 200, 77)).all() and (chip[0, 0] == 0).all()


# ---- the oracle under the gate: the clips of the GPU tests -------------------------------------------------------------------

def _rules(S):
    return {"f2": u.ChipRule(64, S, 2.0), "f4": u.ChipRule(64, S, 4.0), "f2c40": u.ChipRule(40, S, 2.0),
            "f2p3": u.ChipRule(64, S, 2.0, 3, 1)}


@pytest.fixture(scope="module")
def runs(vt, oracle, weights_tiny):
    S = oracle.Model(weights_tiny).S
    out = {}
    for name, (kw, n, step) in CLIPS.items():
        sc = vt.synth.MovingSquare(640, 480, 64, **kw)
        ts, frames = clip_frames(sc, n, step)
        rules = _rules(S)
        out[name] = (u.drive_oracle(weights_tiny, frames, sc.gt_box(ts[0]), rules), rules)
    return out


def test_clip_a_cuts_on_every_due_update(runs):
    res, rules = runs["a"]
    assert all(r.success for r, _, _ in res)
    assert rules["f2"].cut == list(range(1, 13)) and rules["f2"].skipped == []
    assert rules["f2c40"].cut == list(range(1, 13))
    assert rules["f2p3"].cut == [1, 4, 7, 10] and rules["f2p3"].skipped == []
    # factor 4 is the search crop's own factor: any motion of the centre leaves its tap rectangle
    assert rules["f4"].cut == [1] and rules["f4"].skipped == list(range(2, 13))


def test_clip_b_skips_by_geometry_at_factor_2(runs):
    res, rules = runs["b"]
    assert all(r.success for r, _, _ in res)
    assert rules["f2"].skipped == [2, 6] and rules["f2"].cut == [1, 3, 4, 5, 7, 8, 9, 10, 11, 12]
    assert rules["f2c40"].skipped == [2, 6]
    assert [st["f2"] for _, _, st in res][:3] == [u.CUT, u.SKIPPED, u.CUT]


def test_clip_c_cuts_at_the_last_good_box_while_the_update_fails(runs):
    res, rules = runs["c"]
    failed = [i + 1 for i, (r, _, _) in enumerate(res) if not r.success]
    assert failed == [11, 12, 13, 14, 15, 16]
    assert rules["f2"].cut == list(range(1, 19)) and rules["f2"].skipped == []
    boxes = [b for _, b, _ in res]
    assert all(boxes[i - 1] == boxes[9] for i in failed), "a failed update moved the box"
    # with the box frozen the chip at factor 4 fits the search crop again
    assert rules["f4"].cut == [1, 11, 12, 13, 14, 15, 16]
