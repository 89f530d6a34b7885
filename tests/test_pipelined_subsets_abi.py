"""The pipelined subset pass and the queued init (vt_group_enqueue_host_streams, vt_group_enqueue_init_host) exist at
every layer without a GPU: declared in include/vittrack_hip.h, exported by libvittrack_hip.so, listed in the Python
binding's EXPORTS with ctypes prototypes that match the header's argument lists, declared in the Rust crate's sys.rs;
a null handle is refused before anything touches a device."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
# name -> the header's argument types, in order
ARGS = {
    "vt_group_enqueue_host_streams": ["vt_group*", "const int32_t*", "const vt_frame*", "int"],
    "vt_group_enqueue_init_host": ["vt_group*", "int", "const vt_frame*", "vt_bbox"],
}


def _header_args(name):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vittrack_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, f"{name} is not declared in include/vittrack_hip.h"
    types = []
    for a in m.group(1).split(","):
        mm = re.match(r"\s*(.*?)\s*(\w+)\s*$", a)          # type, then the parameter's name
        assert mm, a
        types.append(re.sub(r"\s*\*", "*", " ".join(mm.group(1).split())))
    return types


def test_the_header_declares_both_with_the_agreed_arguments():
    for name, want in ARGS.items():
        assert _header_args(name) == want, name


def test_the_product_library_exports_both(vt):
    assert os.path.exists(vt.LIB_PATH), "run python __graft_entry__.py first"
    out = subprocess.run(["nm", "-D", "--defined-only", vt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ARGS) <= exported, sorted(set(ARGS) - exported)


def test_the_python_binding_lists_and_prototypes_both(vt):
    ctype_of = {"vt_group*": ctypes.c_void_p, "const int32_t*": ctypes.POINTER(ctypes.c_int32),
                "const vt_frame*": ctypes.POINTER(vt.CFrame), "int": ctypes.c_int, "vt_bbox": vt.CBBox}
    L = vt.lib()
    for name in ARGS:
        assert name in vt.EXPORTS
        assert list(getattr(L, name).argtypes) == [ctype_of[t] for t in _header_args(name)], name
    assert L.vt_abi_version() == 5          # additions only: the ABI version stays
    assert callable(vt.Group.enqueue_init_host)
    import inspect
    assert "streams" in inspect.signature(vt.Group.enqueue_host).parameters


def test_the_rust_crate_declares_both():
    sys_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    lib_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "lib.rs")).read()
    for name in ARGS:
        assert f"pub fn {name}(" in sys_rs
        assert f"sys::{name}(" in lib_rs, f"no safe wrapper around {name} in lib.rs"


def test_a_null_handle_is_refused_without_a_gpu(vt):
    L = vt.lib()
    ids = (ctypes.c_int32 * 1)(0)
    frames = (vt.CFrame * 1)()
    assert L.vt_group_enqueue_host_streams(None, ids, frames, 1) == INVALID
    assert L.vt_last_error()
    assert L.vt_group_enqueue_init_host(None, 0, frames, vt.CBBox(0, 0, 8, 8)) == INVALID
    assert L.vt_last_error()
