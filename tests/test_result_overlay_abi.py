"""Result overlay, the boundary (no GPU): the feature adds NO function to include/vittrack_hip.h - it goes through the keys of
vt_group_set_tuning and a tensor name of vt_group_read_tensor, which the header documents - the operator hook lives in the
ops library only, the kernel is built with the decode's flags beside the existing overlay kernels on ONE set of coverage
predicates, and the command-list builder the GPU tests draw their references with gives hand-written known answers."""
import importlib.util
import os
import re
import subprocess

import numpy as np

import result_overlay_util as ro
from test_rust_binding import parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("result_overlay", "result_overlay_style", "result_overlay_luma", "result_overlay_rgb", "result_overlay_min_score_pct")


def _build_py():
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_keys_and_tensor_name_are_in_the_header_and_nothing_else_moved(vt):
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    for k in KEYS:
        assert f'"{k}"' in hdr, f"key {k} is not documented in the header"
    # the tensor name: documented with vt_group_read_tensor, behind its declaration comment's start
    doc = hdr[hdr.index("Copy an intermediate tensor of the last pass"):hdr.index("int64_t vt_group_read_tensor(")]
    assert '"result_overlay" [6]' in doc
    assert "engine options and diagnostics" in hdr.lower()
    assert "WRITES the frames" in hdr, "the caller's new rule (a device pass writes its frames) is not in the header"
    _, cf = parse_header()
    _, _, consts = parse_sys_rs()
    assert len(cf) == 91 == len(vt.EXPORTS)
    assert int(re.search(r"#define VT_ABI_VERSION (\d+)", hdr).group(1)) == 5 and int(consts["VT_ABI_VERSION"]) == 5
    assert vt.lib().vt_abi_version() == 5
    assert not [n for n in cf if "result_overlay" in n], "the product header declares an overlay function"


def test_the_hook_is_in_the_ops_library_only(vt):
    ops_hdr = open(os.path.join(ROOT, "include", "vittrack_hip_ops.h")).read()
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    assert "int vt_op_result_overlay(" in ops_hdr and "vt_op_result_overlay" not in hdr
    assert "vt_op_result_overlay" in vt.OPS_EXPORTS and "vt_op_result_overlay" not in vt.EXPORTS
    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    prod = exported(vt.LIB_PATH)
    assert "vt_op_result_overlay" not in prod and len([n for n in prod if n.startswith("vt_")]) == 91
    assert "vt_op_result_overlay" in exported(vt.ops_lib()._name)
    assert callable(vt.op_result_overlay)
    for cls in (vt.Group, vt.VitTrack):
        for m in ("set_result_overlay", "result_overlay_stats"):
            assert callable(getattr(cls, m)), m
    assert vt.OVERLAY_POLICY_DTYPE.itemsize == 32 and vt.OVERLAY_STATS_DTYPE.itemsize == 32


def test_one_set_of_predicates_and_the_decodes_flags():
    b = _build_py()
    assert "k_result_overlay.hip" in b.HIP_SOURCES and "k_result_overlay.hip" not in b.FAST_CONTRACT
    csrc = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")
    dev = open(os.path.join(csrc, "k_overlay_dev.hpp")).read()
    for fn in ("bool covers(", "bool covers_rgb(", "bool glyph_bit(", "kGlyphs[40][8]"):
        assert fn in dev, fn
    for name in ("k_overlay.hip", "k_result_overlay.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "k_overlay_dev.hpp"' in src, name
        assert "bool covers(" not in src and "kGlyphs[40]" not in src, f"{name} has predicates of its own"


def test_command_list_known_answers():
    # centre by C integer division: odd sizes, and a negative width truncates towards zero
    assert ro.commands((10, 20, 31, 41), 0.5, "luma", flags=2) == [(3, 25, 40, 0, 0, 15, 255, "")]
    assert ro.commands((10, 20, -3, -5), 0.5, "rgb", flags=2, size=7) == [(3, 9, 18, 0, 0, 7, 0x00FF00, "")]
    assert ro.commands((-8, -6, 30, 30), 0.5, "luma", flags=1, thickness=5, luma=200) == [(2, -8, -6, 30, 30, 5, 200, "")]
    # the label: above the box (y - 7 * scale - 4) while that is >= 0, else below it (y + h + 4); x clamped at 0
    assert ro.commands((40, 50, 20, 10), 0.5, "luma", flags=4) == [(1, 40, 32, 0, 0, 2, 255, "score: 50%")]
    assert ro.commands((40, 18, 20, 10), 0.5, "luma", flags=4) == [(1, 40, 0, 0, 0, 2, 255, "score: 50%")]
    assert ro.commands((40, 17, 20, 10), 0.5, "luma", flags=4) == [(1, 40, 31, 0, 0, 2, 255, "score: 50%")]
    assert ro.commands((-5, 3, 20, 10), 0.5, "rgb", flags=4, scale=3, luma=9) == [(1, 0, 17, 0, 0, 3, 9, "score: 50%")]
    # order and values on both surfaces: text takes the luma key everywhere
    full = ro.commands((1, 40, 4, 6), 0.75, "rgb", rgb=0x102030, luma=77)
    assert full == [(2, 1, 40, 4, 6, 3, 0x102030, ""), (3, 3, 43, 0, 0, 15, 0x102030, ""), (1, 1, 22, 0, 0, 2, 77, "score: 75%")]
    # N: one binary32 multiply, ties to even, clamped
    assert [ro.label_n(s) for s in (0.125, 0.375, 0.995, 1.0, 0.0, float("nan"))] == [12, 38, 100, 100, 0, 0]
    assert ro.label_n(1.7) == 100 and ro.label_n(-0.3) == 0 and ro.label_n(0.004) == 0 and ro.label_n(0.0051) == 1
    # the gate is strict, in binary32
    assert not ro.draws(1, 0.25) and ro.draws(1, np.nextafter(np.float32(0.25), np.float32(1))) and not ro.draws(0, 0.9)
    assert not ro.draws(1, float("nan")) and ro.draws(1, 0.0001, 0) and not ro.draws(1, 0.0, 0) and not ro.draws(1, 1.0, 100)


def test_expected_frame_on_every_surface(oracle):
    """the reference builder itself: the luma formats change luma bytes only, the RGB formats never their pad byte, P010
    nothing - and the same pixels are lit whatever the byte layout"""
    w, h = 96, 64
    rng = np.random.default_rng(3)
    slot = [(1, 0.8, (20, 24, 30, 20))]
    lit = None
    for fmt in ro.DRAWABLE + ("p010",):
        buf = rng.integers(0, 200, ro.frame_bytes(fmt, w, h), dtype=np.uint8)
        out = ro.expected(oracle, fmt, buf, w, h, slot, luma=255, rgb=0xFFFFFF)
        ch = out != buf
        if fmt == "p010":
            assert not ch.any()
            continue
        if ro.surface(fmt) == "luma":
            m = np.zeros_like(ch)
            ro.luma_view(fmt, m, w, h)[...] = True
            assert not (ch & ~m).any(), f"{fmt}: a byte outside the luma changed"
            px = ro.luma_view(fmt, out, w, h) == 255
        else:
            m = np.zeros_like(ch)
            ro.rgb_view(fmt, m, w, h)[...] = True
            assert not (ch & ~m).any(), f"{fmt}: a pad byte changed"
            px = np.all(ro.rgb_view(fmt, out, w, h) == 255, axis=2)
        assert px.sum() > 300
        # luma rectangles include x + w and y + h, the RGB ones do not: the lit sets agree inside each family
        key = ro.surface(fmt)
        lit = lit or {}
        if key in lit:
            assert np.array_equal(lit[key], px), fmt
        lit[key] = px
