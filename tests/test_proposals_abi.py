"""Reacquire proposals: what the option adds to the boundary - keys and tensors of existing functions, one operator hook,
Python methods - and what it does not: a product function."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("proposals", "proposals_period", "proposals_max", "proposals_min_sim_pm", "proposals_max_cells")
TENSORS = ("proposals", "proposals_pattern", "proposals_map")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_header_still_declares_91_functions(vt):
    txt = re.sub(r"/\*.*?\*/", "", _header("vittrack_hip.h"), flags=re.S)
    names = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", txt))
    assert len(names) == 91 and len(vt.EXPORTS) == 91 and set(vt.EXPORTS) == names
    assert "#define VT_ABI_VERSION 5" in _header("vittrack_hip.h").replace("  ", " ")


def test_the_hook_is_an_ops_export(vt):
    ops = re.sub(r"/\*.*?\*/", "", _header("vittrack_hip_ops.h"), flags=re.S)
    assert re.search(r"\bint\s+vt_op_proposals\s*\(", ops)
    assert "vt_op_proposals" in vt.OPS_EXPORTS and "vt_op_proposals" not in vt.EXPORTS


def test_python_methods(vt):
    for name in ("set_proposals", "proposals", "proposals_pattern", "proposals_map"):
        assert callable(getattr(vt.Group, name))
    assert callable(vt.VitTrack.set_proposals) and callable(vt.VitTrack.proposals) and callable(vt.op_proposals)
    sig = inspect.signature(vt.Group.reacquire)
    assert sig.parameters["proposals"].default is False
    assert vt.PROPOSALS_REC_DTYPE.itemsize == 224 and vt.PROPOSAL_DTYPE.itemsize == 24


def test_the_header_names_every_key_and_tensor():
    txt = _header("vittrack_hip.h")
    for k in KEYS + TENSORS:
        assert f'"{k}"' in txt, k
    for word in ("THE TWIN IDENTITY: the option only reads", "Chebyshev distance M / 2", "4096.0f / 48.0f"):
        assert word in txt, word
