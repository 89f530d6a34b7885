"""Stream conflicts: what the change adds to the boundary - four keys, one tensor, one operator hook, Python methods - and
what it does not: a product function or a new ABI version."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("conflicts", "conflicts_iou_pm", "conflicts_gate", "conflicts_scene")


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
    assert re.search(r"\bint\s+vt_op_stream_conflicts\s*\(", ops)
    assert "vt_op_stream_conflicts" in vt.OPS_EXPORTS and "vt_op_stream_conflicts" not in vt.EXPORTS
    assert "vt_op_stream_conflicts" in _exports(vt.OPS_LIB_PATH) and "vt_op_stream_conflicts" not in _exports(vt.LIB_PATH)


def test_python_methods(vt):
    assert callable(vt.op_stream_conflicts)
    for name in ("set_conflicts", "set_scene", "conflicts"):
        assert callable(getattr(vt.Group, name)) and callable(getattr(vt.VitTrack, name)), name
    assert vt.CONFLICT_REC_DTYPE.itemsize == 48 and vt.CONFLICT_REC_DTYPE.fields["partner"][1] == 16
    assert vt.CONFLICT_REC_DTYPE.fields["iou"][1] == 32 and vt.CONFLICT_COUNT_DTYPE.itemsize == 16


def test_the_product_header_states_the_rule():
    txt = _header("vittrack_hip.h")
    for k in KEYS:
        assert f'"{k}"' in txt, k
    for word in ("THE RULE, to the bit", "ix = fminf(x_s + w_s, x_t + w_t) - fmaxf(x_s, x_t)", "uni = (w_s * h_s + w_t * h_t) - inter",
                 "iou = inter / uni", "iou >= tau", "(iou descending, stream index ascending)", "REFRESH RULE 9",
                 "OF THE SAME PASS", "st.window_miss != st.frames_done", '"conflicts" [16]'):
        assert word in txt, word
    assert "camera_motion" not in txt


def test_the_kernel_file_is_built_like_the_motion_rule():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "k_conflicts.hip" in b.HIP_SOURCES and "k_conflicts.hip" not in b.FAST_CONTRACT
    assert "-ffp-contract=off" in b.HIP_FLAGS and "-fhip-fp32-correctly-rounded-divide-sqrt" in b.HIP_FLAGS
    src = open(os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc", "k_conflicts.hip")).read()
    assert "#pragma clang fp contract(off)" in src
