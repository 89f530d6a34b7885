"""Frame health: what the change adds to the boundary - keys and tensors of existing functions, one operator hook with its
Python binding - and what it does not: a product function or a new ABI version."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("health", "health_period", "health_cell", "health_still_run", "health_flat_q", "health_cut_pm", "health_gate",
        "health_max_cells")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("vt_")}


def test_the_header_still_declares_91_functions_and_the_library_exports_exactly_them(vt):
    txt = re.sub(r"/\*.*?\*/", "", _header("vittrack_hip.h"), flags=re.S)
    names = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", txt))
    assert len(names) == 91 and set(vt.EXPORTS) == names
    assert "#define VT_ABI_VERSION 5" in _header("vittrack_hip.h").replace("  ", " ")
    assert _exports(vt.LIB_PATH) == names


def test_the_hook_is_declared_and_carried_by_the_ops_library_only(vt):
    ops = re.sub(r"/\*.*?\*/", "", _header("vittrack_hip_ops.h"), flags=re.S)
    assert re.search(r"\bint\s+vt_op_frame_health\s*\(", ops)
    assert "vt_op_frame_health" in vt.OPS_EXPORTS and "vt_op_frame_health" not in vt.EXPORTS
    assert "vt_op_frame_health" in _exports(vt.OPS_LIB_PATH) and "vt_op_frame_health" not in _exports(vt.LIB_PATH)


def test_python_names(vt):
    assert callable(vt.op_frame_health) and callable(vt.Group.set_health) and callable(vt.Group.frame_health)
    for k in KEYS + ("health_words",):
        assert f'"{k}"' in _header("vittrack_hip.h"), k
    assert vt.HEALTH_REC_DTYPE.itemsize == 104 and vt.HEALTH_REC_DTYPE.fields["S1"][1] == 32
    assert vt.HEALTH_REC_DTYPE.fields["has_prev"][1] == 80 and vt.HEALTH_COUNT_DTYPE.itemsize == 16
    assert vt.HEALTH_HEAD_DTYPE.itemsize == 32


def test_the_ops_header_states_the_rule():
    txt = _header("vittrack_hip_ops.h")
    for k in KEYS:
        assert f'"{k}"' in txt, k
    for word in ("THE RULE, to the bit", "n * S2 - S1 * S1 <= flat_q * flat_q * n * n", "HD * 1000\n * >= cut_pm * 2 * n",
                 "min(still + 1, 1 << 30)", "t >> 7 == b", "G_ref := G at status 5 and at a CUT"):
        assert word in txt, word


def test_the_kernel_file_and_the_shared_cell_header_are_built():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "k_health.hip" in b.HIP_SOURCES and "k_health.hip" not in b.FAST_CONTRACT
    src = open(os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py")).read()
    assert '"k_thumb_dev.hpp"' in src           # a change of the shared cell rebuilds both kernel files
    csrc = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")
    for f in ("k_health.hip", "k_camera_motion.hip"):
        assert '#include "k_thumb_dev.hpp"' in open(os.path.join(csrc, f)).read(), f
    text = open(os.path.join(csrc, "k_health.hip")).read()
    # the measures, the flags and every sum: no floating-point type in this file. The taps are not covered by this: they reach
    # thumb_cell (k_thumb_dev.hpp) as fetch_rgb's float values, exact integers 0..255, and are converted there
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", text)), "a floating-point type in k_health.hip"
