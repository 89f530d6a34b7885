"""The layout of csrc's headers, read as text (no compiler, no GPU): a kernel file's host-visible ABI lives in the header of the
same name, vt_common.hpp holds only what the math kernels also need, the build identity of k_gemm256.hip covers exactly its
include closure, and build.py's staleness check knows every header."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gstreamer-vit-tracker_amd")
CSRC = os.path.join(PKG, "csrc")
INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)

# what the math kernels may see: the core, the GEMM, LayerNorm and attention APIs and the device helpers they share
MATH = {"k_gemm.hip", "k_gemm256.hip", "k_attn.hip", "k_misc.hip"}
MATH_HEADERS = {"vt_common.hpp", "k_gemm.hpp", "k_gemm_util.hpp", "k_ln_dev.hpp", "k_attn.hpp", "k_misc.hpp"}
# the decode writes StreamState: k_head.hip also sees the frame and state header (and through it the public header)
HEAD_HEADERS = MATH_HEADERS | {"k_head.hpp", "vt_frame.hpp", "../include/vittrack_hip.h"}
FEATURES = {"k_refresh.hpp", "k_chip.hpp", "k_peaks.hpp", "k_motion.hpp", "k_appearance.hpp", "k_arbitrate.hpp", "k_proposals.hpp",
            "k_camera_motion.hpp", "k_conflicts.hpp", "k_health.hpp", "k_result_overlay.hpp"}
FRAME_WORDS = re.compile(r"\b(FrameDesc|StreamState|PixFamily|PIXF_\w+|PIXL_\w+|pix_[a-z0-9_]+)\b")


def _build_py():
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(PKG, "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _name(path):
    """a file of csrc/ by its name, anything else by its path from the package"""
    return os.path.basename(path) if os.path.dirname(path) == CSRC else os.path.relpath(path, PKG)


def _includes(path):
    return [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in INCLUDE.findall(open(path).read())]


def closure(name):
    """the file and every project header reachable from it through #include "..." lines"""
    seen, todo = [], [os.path.join(CSRC, name)]
    while todo:
        p = todo.pop()
        if p not in seen:
            seen.append(p)
            todo += _includes(p)
    return {_name(p) for p in seen}


def _hip_files():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def test_every_source_is_followed_and_every_include_exists():
    b = _build_py()
    assert set(b.HIP_SOURCES + b.OPS_SOURCES) == set(_hip_files())
    for f in _hip_files():
        for n in closure(f):
            assert os.path.exists(os.path.join(CSRC, n) if os.sep not in n else os.path.join(PKG, n)), (f, n)


def test_math_kernels_see_no_feature_no_pixel_format_and_no_stream_state():
    for f in sorted(MATH):
        c = closure(f)
        assert not c & FEATURES, (f, sorted(c & FEATURES))
        assert c - {f} <= MATH_HEADERS, (f, sorted(c - {f} - MATH_HEADERS))
        for n in sorted(c):
            found = FRAME_WORDS.search(open(os.path.join(CSRC, n)).read())
            assert found is None, (f, n, found.group(0))


def test_the_head_sees_the_frame_header_and_no_feature():
    c = closure("k_head.hip")
    assert not c & FEATURES, sorted(c & FEATURES)
    assert c - {"k_head.hip"} <= HEAD_HEADERS, sorted(c - {"k_head.hip"} - HEAD_HEADERS)


def test_a_kernel_files_header_is_its_first_project_include():
    """so every ordinary build proves that the header is self-contained"""
    for f in _hip_files():
        own = f.replace(".hip", ".hpp")
        if os.path.exists(os.path.join(CSRC, own)):
            first = INCLUDE.search(open(os.path.join(CSRC, f)).read())
            assert first is not None and first.group(1) == own, (f, first and first.group(1))
    assert INCLUDE.search(open(os.path.join(CSRC, "k_gemm256.hip")).read()).group(1) == "k_gemm.hpp"
    # the ten optional features of the pass keep their ABI in the header named after their kernel file
    for h in sorted(FEATURES):
        assert os.path.exists(os.path.join(CSRC, h.replace(".hpp", ".hip"))), h


def test_the_stamped_identity_is_exactly_the_include_closure():
    b = _build_py()
    for src, files in b.STAMPED.items():
        assert len(files) == len(set(files)), files
        assert set(files) == closure(src), (src, sorted(set(files) ^ closure(src)))
    assert "k_gemm256.hip" in b.STAMPED


def test_the_staleness_check_knows_every_header():
    b = _build_py()
    on_disk = {f for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc", ".h"))}
    assert on_disk == set(b.HEADERS), sorted(on_disk ^ set(b.HEADERS))
    assert len(b.HEADERS) == len(set(b.HEADERS))
    # build_hip checks that very list, for every translation unit alike
    txt = " ".join(open(os.path.join(PKG, "build.py")).read().split())
    assert "headers = [os.path.join(CSRC, h) for h in HEADERS] + [" in txt and "_newer(obj, [src] + headers)" in txt
