"""The subset-pass entry points (vt_group_*_streams) exist at every layer without a GPU: exported by
libvittrack_hip.so, declared in include/vittrack_hip.h, listed in the Python binding's EXPORTS with their
argument types, and declared in the Rust crate's sys.rs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["vt_group_enqueue_device_streams", "vt_group_update_device_streams", "vt_group_update_host_streams"]


def test_the_product_library_exports_the_subset_pass_entry_points(vt):
    assert os.path.exists(vt.LIB_PATH), "run python __graft_entry__.py first"
    out = subprocess.run(["nm", "-D", "--defined-only", vt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(NAMES) <= exported, sorted(set(NAMES) - exported)


def test_every_layer_declares_them(vt):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vittrack_hip.h")).read(), flags=re.S)
    sys_rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    L = vt.lib()
    for n in NAMES:
        # (group, const int32_t* streams, const vt_frame* frames, int n [, vt_result* out])
        m = re.search(n + r"\s*\(\s*vt_group\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*streams\s*,", header)
        assert m, f"{n} not declared as (vt_group*, const int32_t* streams, ...)"
        assert n in vt.EXPORTS
        assert f"pub fn {n}(" in sys_rs
        assert len(getattr(L, n).argtypes) == (4 if "enqueue" in n else 5)
    assert L.vt_abi_version() == 5          # additions only: the ABI version stays
