"""Motion prior, the boundary (no GPU): the feature adds NO function to include/vittrack_hip.h - it goes through four keys of
vt_group_set_tuning and a tensor name of vt_group_read_tensor, which the header documents with the rule - the operator hook
lives in the ops library only, the kernels are built with the decode's flags (one IEEE operation per source operation), and
the per-stream record is no part of the 88-byte state."""
import importlib.util
import os
import re
import subprocess

from test_rust_binding import parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("motion_prior", "motion_gain_pct", "motion_coast", "motion_max_pct")


def _build_py():
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_keys_and_tensor_name_are_in_the_header_and_nothing_else_moved(vt):
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    for k in KEYS:
        assert f'"{k}"' in hdr, f"key {k} is not documented in the header"
    doc = hdr[hdr.index("Copy an intermediate tensor of the last pass"):hdr.index("int64_t vt_group_read_tensor(")]
    assert '"motion" [8]' in doc
    rule = hdr[hdr.index("ENGINE OPTIONS - the motion prior"):hdr.index("DIAGNOSTICS (A/B")]
    for word in ("PLACE", "SETTLE", "THE TWIN IDENTITY", "vt_group_set_state_box", "binary32", "v = v + a*(d - v)", "fminf(fmaxf(v, -lim), lim)"):
        assert word in rule, f"the rule in the header does not say '{word}'"
    _, cf = parse_header()
    _, _, consts = parse_sys_rs()
    assert len(cf) == 91 == len(vt.EXPORTS)
    assert int(re.search(r"#define VT_ABI_VERSION (\d+)", hdr).group(1)) == 5 and int(consts["VT_ABI_VERSION"]) == 5
    assert vt.lib().vt_abi_version() == 5
    assert not [n for n in cf if "motion" in n], "the product header declares a motion function"


def test_the_hook_is_in_the_ops_library_only(vt):
    ops_hdr = open(os.path.join(ROOT, "include", "vittrack_hip_ops.h")).read()
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    assert "int vt_op_motion_prior(" in ops_hdr and "vt_op_motion_prior" not in hdr
    assert "vt_op_motion_prior" in vt.OPS_EXPORTS and "vt_op_motion_prior" not in vt.EXPORTS

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    prod = exported(vt.LIB_PATH)
    assert "vt_op_motion_prior" not in prod and len([n for n in prod if n.startswith("vt_")]) == 91
    assert "vt_op_motion_prior" in exported(vt.ops_lib()._name)
    assert callable(vt.op_motion_prior)
    for cls in (vt.Group, vt.VitTrack):
        for m in ("set_motion_prior", "motion"):
            assert callable(getattr(cls, m)), m
    assert vt.MOTION_REC_DTYPE.itemsize == 48 and vt.CANDIDATE_DTYPE.itemsize == 24


def test_the_kernels_keep_one_operation_per_operation_and_the_state_stays_88_bytes(vt):
    b = _build_py()
    assert "k_motion.hip" in b.HIP_SOURCES and "k_motion.hip" not in b.FAST_CONTRACT
    assert "vt_ingest.hip" not in b.FAST_CONTRACT, "the host's window planning repeats the place rule: same flags"
    assert "-ffp-contract=off" in b.HIP_FLAGS
    csrc = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")
    common = open(os.path.join(csrc, "vt_frame.hpp")).read() + open(os.path.join(csrc, "k_motion.hpp")).read()   # the state; the feature
    assert "static_assert(sizeof(StreamState) == 88" in common and "static_assert(sizeof(MotionRec) == 48" in common
    for decl in ("hipError_t launch_motion_place(", "hipError_t launch_motion_settle(", "bool motion_predict("):
        assert decl in common, decl
    state = common[common.index("struct StreamState {"):common.index("static_assert(sizeof(StreamState)")]
    assert "motion" not in state.lower() and "prior" not in state
    from gstreamer_vit_tracker_amd.snapshot import STATE
    assert STATE.itemsize == 88
    # the crop kernels, the decode and the crop body are not part of the feature: they name nothing of it
    for name in ("k_preproc.hip", "k_preproc_body.inc", "k_head.hip"):
        assert "otion" not in open(os.path.join(csrc, name)).read(), name
