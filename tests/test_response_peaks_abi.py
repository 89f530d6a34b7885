"""Response peaks, the boundary (no GPU): the four new functions of include/vittrack_hip.h are exported by the built library
and bound in ctypes and Rust with one signature, vt_peak / vt_peaks have one layout (32 / 272 bytes) on every side, the ABI
version stays 5 (additions only), and the kernel is built with the decode's flags."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np

from test_rust_binding import _size, parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vt_group_set_peaks", "vt_group_last_peaks", "vt_set_peaks", "vt_last_peaks")
PEAK = [("score", "f32", 0), ("resp", "f32", 0), ("box", "f32", 4), ("cell", "i32", 0), ("reserved", "i32", 0)]
PEAKS = [("n", "i32", 0), ("stream", "i32", 0), ("frames_done", "i32", 0), ("radius", "i32", 0), ("peak", "vt_peak", 8)]


def _build_py():
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_the_four_functions_are_exported_and_bound(vt):
    out = subprocess.run(["nm", "-D", "--defined-only", vt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for name in NEW:
        assert name in exported, f"{name} is not exported by {os.path.basename(vt.LIB_PATH)}"
        assert name in vt.EXPORTS and hasattr(vt.lib(), name)
    assert "vt_op_response_peaks" not in exported and "vt_op_response_peaks" in vt.OPS_EXPORTS
    assert len([n for n in exported if n.startswith("vt_")]) == 91 == len(vt.EXPORTS)
    _, cf = parse_header()
    _, rf, consts = parse_sys_rs()
    assert len(cf) == 91
    for name in NEW:
        assert rf[name] == cf[name], name
    assert cf["vt_group_set_peaks"] == ("i32", ["ptr", "i32", "i32", "i32", "f32"])
    assert cf["vt_group_last_peaks"] == ("i32", ["ptr", "ptr", "i32"])
    assert cf["vt_set_peaks"] == ("i32", ["ptr", "i32", "i32", "f32"])
    assert cf["vt_last_peaks"] == ("i32", ["ptr", "ptr"])
    # header order, in sys.rs too
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    for txt, decl in ((hdr, "int {}("), (sys_rs, "pub fn {}(")):
        pos = [txt.index(decl.format(n)) for n in NEW]
        assert pos == sorted(pos)
    lib_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "lib.rs")).read()
    for needle in ("pub fn set_peaks(&mut self, max_peaks: i32, radius: i32, min_resp: f32)", "pub fn last_peaks(&mut self)",
                   "sys::vt_set_peaks(", "sys::vt_last_peaks(", "sys::vt_group_set_peaks(", "sys::vt_group_last_peaks("):
        assert needle in lib_rs, needle
    for cls in (vt.Group, vt.VitTrack):
        for m in ("set_peaks", "last_peaks"):
            assert callable(getattr(cls, m)), m
    assert callable(vt.op_response_peaks)
    # additions only: the version stays
    assert int(re.search(r"#define VT_ABI_VERSION (\d+)", hdr).group(1)) == 5 and int(consts["VT_ABI_VERSION"]) == 5
    assert vt.lib().vt_abi_version() == 5


def test_the_records_are_32_and_272_bytes_on_every_side(vt, tmp_path):
    assert ctypes.sizeof(vt.CPeak) == 32 and ctypes.sizeof(vt.CPeaks) == 272
    assert vt.PEAK_DTYPE.itemsize == 32 and vt.PEAKS_DTYPE.itemsize == 272 and vt.PEAKS_POLICY_DTYPE.itemsize == 16
    assert [f[0] for f in vt.CPeak._fields_] == [f[0] for f in PEAK] == list(vt.PEAK_DTYPE.names)
    assert [f[0] for f in vt.CPeaks._fields_] == [f[0] for f in PEAKS] == list(vt.PEAKS_DTYPE.names)
    for f in PEAKS:
        assert getattr(vt.CPeaks, f[0]).offset == vt.PEAKS_DTYPE.fields[f[0]][1]
    for f in PEAK:
        assert getattr(vt.CPeak, f[0]).offset == vt.PEAK_DTYPE.fields[f[0]][1]
    cs, _ = parse_header()
    assert cs["vt_peak"] == PEAK and cs["vt_peaks"] == PEAKS
    assert _size(cs["vt_peak"], cs) == 32 and _size(cs["vt_peaks"], cs) == 272
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    assert int(re.search(r"#define VT_PEAKS_MAX (\d+)", hdr).group(1)) == 8 == vt.PEAKS_MAX
    # Rust: the array of records is `[VtPeak; VT_PEAKS_MAX]` with the constant 8
    sys_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    rs, _, _ = parse_sys_rs()
    assert rs["VtPeak"] == PEAK and _size(rs["VtPeak"], cs) == 32
    assert re.search(r"pub const VT_PEAKS_MAX: usize = 8;", sys_rs)
    assert [f[0] for f in rs["VtPeaks"]] == [f[0] for f in PEAKS] and rs["VtPeaks"][:4] == PEAKS[:4]
    assert re.search(r"pub peak: \[VtPeak; VT_PEAKS_MAX\],", sys_rs)
    # a C99 compiler, strict flags: sizes and offsets
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vittrack_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d\\n", sizeof(vt_peak), sizeof(vt_peaks), offsetof(vt_peaks, peak), '
                   'offsetof(vt_peak, cell), VT_PEAKS_MAX);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    "-o", str(exe), str(src)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["32", "272", "16", "24", "8"]


def test_the_stream_state_is_untouched_and_the_kernel_is_built_like_the_decode():
    src = open(os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc", "vt_frame.hpp")).read()
    assert "static_assert(sizeof(StreamState) == 88" in src
    b = _build_py()
    assert "k_peaks.hip" in b.HIP_SOURCES and "k_peaks.hip" not in b.FAST_CONTRACT and "k_head.hip" not in b.FAST_CONTRACT
    assert b.EXTRA_FLAGS.get("k_peaks.hip") == b.EXTRA_FLAGS.get("k_head.hip")
    ops = open(os.path.join(ROOT, "include", "vittrack_hip_ops.h")).read()
    assert "int vt_op_response_peaks(" in ops


def test_argument_checks_need_no_device(vt):
    """null handles and null outputs are refused before anything touches a device"""
    L = vt.lib()
    rec = np.zeros(1, vt.PEAKS_DTYPE)
    assert L.vt_group_set_peaks(None, 0, 1, 2, ctypes.c_float(0.0)) == -1
    assert L.vt_group_last_peaks(None, rec.ctypes.data, 1) == -1
    assert L.vt_set_peaks(None, 1, 2, ctypes.c_float(0.0)) == -1
    assert L.vt_last_peaks(None, rec.ctypes.data) == -1
    assert not rec.view(np.uint8).any()
