"""The colour bits of vt_frame.format: what the change adds to the boundary - two enums and one macro, mirrored in the Rust
crate and in Python - and what it does not: a function, an export, a pixel-format constant or a new ABI version."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")
NAMES = {"VT_COLOR_BT601": 0, "VT_COLOR_BT709": 1, "VT_COLOR_BT2020": 2, "VT_RANGE_LIMITED": 0, "VT_RANGE_FULL": 1}


def _header():
    return open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("vt_")}


def test_the_header_declares_the_two_enums_and_the_macro():
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"typedef\s+enum\s+vt_color_matrix\s*\{(.*?)\}\s*vt_color_matrix\s*;", txt, flags=re.S)
    r = re.search(r"typedef\s+enum\s+vt_color_range\s*\{(.*?)\}\s*vt_color_range\s*;", txt, flags=re.S)
    assert m and r
    got = {k: int(v) for k, v in re.findall(r"(VT_\w+)\s*=\s*(\d+)", m.group(1) + "," + r.group(1))}
    assert got == NAMES
    assert re.search(r"#define\s+VT_FRAME_FORMAT\(pix, matrix, range\)\s+\(\(int32_t\)\(pix\) \| \(\(int32_t\)\(matrix\) << 8\) \| "
                     r"\(\(int32_t\)\(range\) << 12\)\)", txt)


def test_the_macro_compiles_as_c99_and_a_plain_format_is_itself(tmp_path):
    src = tmp_path / "m.c"
    src.write_text('#include "vittrack_hip.h"\n'
                   "_Static_assert(VT_FRAME_FORMAT(VT_PIX_NV12, VT_COLOR_BT601, VT_RANGE_LIMITED) == VT_PIX_NV12, \"plain\");\n"
                   "_Static_assert(VT_FRAME_FORMAT(VT_PIX2_I420, VT_COLOR_BT2020, VT_RANGE_FULL) == 0x1210, \"word\");\n"
                   "_Static_assert(VT_FRAME_FORMAT(VT_PIX_NV12, VT_COLOR_BT709, VT_RANGE_LIMITED) == 0x0101, \"word\");\n"
                   "int main(void) { vt_frame f; f.format = VT_FRAME_FORMAT(VT_PIX_YUY2, VT_COLOR_BT709, VT_RANGE_FULL); return f.format != 0x1102; }\n")
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-o", str(exe),
                    str(src)], check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_still_91_functions_abi_5_and_the_same_exports(vt):
    txt = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", txt))
    assert len(names) == 91 and set(vt.EXPORTS) == names
    assert "#define VT_ABI_VERSION 5" in _header().replace("  ", " ")
    assert _exports(vt.LIB_PATH) == names
    # with the comments left in (some tests count that way): the new text spells no lower-case vt_...( of its own - the two
    # extra matches are the older comments' "vt_pixfmt2 (" and "vt_groups ("
    assert set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", _header())) == names | {"vt_pixfmt2", "vt_groups"}


def test_header_rust_and_python_agree_on_the_five_values(vt):
    rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    consts = dict(re.findall(r"pub const (\w+): i32 = (-?\d+);", rs))
    for k, v in NAMES.items():
        assert int(consts[k]) == v, k
        assert getattr(vt, k[3:]) == v, k
    fn = re.search(r"pub const fn vt_frame_format\(pix: i32, matrix: i32, range: i32\) -> i32 \{(.*?)\}", rs, flags=re.S)
    assert fn and fn.group(1).strip() == "pix | (matrix << 8) | (range << 12)"
    for banned in ("assert", "unwrap", "expect", "panic", "[", "checked_", "/", "%"):      # nothing that can panic
        assert banned not in fn.group(1), banned
    lib_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "lib.rs")).read()
    assert "vt_frame_format as frame_format" in lib_rs
    assert vt.frame_format(vt.PIX_I420, vt.COLOR_BT2020, True) == 0x1210


def test_no_new_constant_is_a_pixel_format():
    for txt in (_header(), open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()):
        pix = set(re.findall(r"\b(VT_PIX2?_\w+)\b", txt))
        assert len(pix) == 15, sorted(pix)
    assert not [k for k in NAMES if k.startswith("VT_PIX")]


def test_the_table_exists_once_in_a_header_the_build_knows():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    holders = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".inc"))
               and re.search(r"\b459\b.*\b541\b", open(os.path.join(CSRC, f)).read())]
    assert holders == ["k_preproc_dev.hpp"], holders
    assert set(f for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))) == set(b.HEADERS)
    frame = open(os.path.join(CSRC, "vt_frame.hpp")).read()
    assert re.search(r"#define PIX_LEVELS 4\b", frame)


def test_the_documents_state_the_rule():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for txt in (_header(), design):
        for row in ("298", "459", "541", "403", "475", "430", "548", "377", "482", "0xffff"):
            assert row in txt, row
    assert "colorimetry" in integ and "bt709" in integ and "BT.601" in integ
    assert os.path.exists(os.path.join(ROOT, "profiles", "colorimetry.txt"))
