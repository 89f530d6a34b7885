"""Stream snapshots, the part that needs no GPU: the byte format of include/vittrack_hip.h as snapshot.py states it a
second time, read back by vt_snapshot_info; the size formula; every class of malformed snapshot that can be told without an
engine is VT_ERR_FORMAT and never a crash; the eight new functions are exported and bound (C, ctypes, Rust)."""
import ctypes
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest

from test_rust_binding import _size, parse_header, parse_sys_rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, FORMAT = -1, -4
NEW = ("vt_snapshot_bytes", "vt_group_snapshot_bytes", "vt_snapshot_info", "vt_group_export_stream",
       "vt_group_import_stream", "vt_group_copy_stream", "vt_export_state", "vt_import_state")


def _state(**kw):
    """a state a pass could have left: 7 updates of a 640x480 stream, 6 of them successful, one refresh at update 4"""
    st = dict(box=(301.0, 207.0, 64.0, 66.0), geo=(204.5, 110.25, 2.03125, 260.0), frame_w=640, frame_h=480, initialized=1,
              frames_done=7, success_count=6, last_idx=27, last_fbox=(301.25, 206.75, 64.5, 65.5), last_score=0.8125,
              window_miss=3, tpl_gen=1, tpl_frame=4)
    st.update(kw)
    return st


def _tiny(vt, state=None, policy=None, flags=0, rows=None):
    S = vt.snapshot
    geo = S.geometry_of("tiny")
    if rows is None:
        rng = np.random.default_rng(5)
        rows = vt.weights.f32_to_bf16_bits(rng.standard_normal((geo["tokens_template"], geo["kpad"])).astype(np.float32))
    return S.pack(geo, state or _state(), policy if policy is not None else dict(period=4, min_score=0.25, skipped_geometry=2),
                  rows, flags), rows


def _code(vt, blob):
    """vt_snapshot_info's status for these bytes (the error text must be set on failure)"""
    d = vt.CSnapshotDesc()
    rc = vt.lib().vt_snapshot_info(bytes(blob), len(blob), ctypes.byref(d))
    if rc != 0:
        assert vt.lib().vt_last_error().decode().startswith("snapshot:"), vt.lib().vt_last_error()
    return rc


def _edit(vt, blob, dtype, off, restamp=True, **fields):
    """the snapshot with fields of the record at `off` overwritten, the checksum recomputed unless told otherwise"""
    b = bytearray(blob)
    rec = np.frombuffer(bytes(b[off:off + dtype.itemsize]), dtype).copy()
    for k, v in fields.items():
        rec[k] = v
    b[off:off + dtype.itemsize] = rec.tobytes()
    return vt.snapshot.restamp(bytes(b)) if restamp else bytes(b)


def test_a_packed_snapshot_is_read_back_field_for_field(vt):
    S = vt.snapshot
    blob, rows = _tiny(vt, flags=S.FLAG_ANY_GRAPHS)
    geo, st = S.geometry_of("tiny"), _state()
    assert len(blob) == 256 + 24576 and blob[:8] == b"VTSS0001"
    info = vt.snapshot_info(blob)
    assert info["total_bytes"] == len(blob) and info["header_bytes"] == 152 and info["state_bytes"] == 88
    assert info["policy_bytes"] == 16 and info["rows_bytes"] == 24576 and info["flags"] == 1
    for k in ("patch", "template_size", "search_size", "kpad", "tokens_template"):
        assert info[k] == geo[k], k
    assert np.array_equal(np.array(info["norm_a"], np.float32), geo["norm_a"])
    assert np.array_equal(np.array(info["norm_b"], np.float32), geo["norm_b"])
    assert tuple(info["box"]) == st["box"] and (info["frame_width"], info["frame_height"]) == (640, 480)
    assert info["frames_done"] == 7 and info["success_count"] == 6 and info["last_score"] == 0.8125
    assert (info["period"], info["min_score"], info["skipped_geometry"]) == (4, 0.25, 2)
    assert info["generation"] == 1 and info["last_frame"] == 4
    # and snapshot.py reads its own bytes back
    p = S.parse(blob)
    assert p["checksum_ok"] and np.array_equal(p["rows"], rows) and int(p["state"]["last_idx"]) == 27
    assert int(p["header"]["checksum"]) == S.checksum(blob)
    # a freshly initialised stream (all counters zero, no policy) is a valid snapshot too
    fresh = dict(box=(10.0, 20.0, 30.0, 40.0), frame_w=640, frame_h=480, initialized=1)
    assert _code(vt, S.pack(geo, fresh, None, rows)) == 0


@pytest.mark.parametrize("cfg,rows_bytes", [("tiny", 24576), ("cfg2", 2 * 64 * 768), ("cfg3", 221184), ("cfg5", 2 * 196 * 640)])
def test_the_size_formula_agrees_with_snapshot_py(vt, cfg, rows_bytes):
    c = vt.weights.get_config(cfg)
    want = vt.snapshot.snapshot_bytes(c.n_t, c.kpad)
    assert want == 256 + rows_bytes
    assert vt.snapshot_bytes(vt.model_info_for(cfg)) == want
    assert vt.lib().vt_snapshot_bytes(None) == 0
    bad = vt.model_info_for(cfg)
    bad.kpad = 100
    assert vt.snapshot_bytes(bad) == 0


def test_truncation_magic_version_and_sizes(vt):
    S = vt.snapshot
    blob, _ = _tiny(vt)
    assert _code(vt, blob) == 0
    for n in (0, 7, 8, S.HEADER_BYTES - 1, S.HEADER_BYTES, S.POLICY_OFF, S.ROWS_OFF, len(blob) - 1):
        assert _code(vt, blob[:n]) == FORMAT, f"truncated to {n}"
    assert _code(vt, blob + b"\0") == FORMAT
    for off in (0, 3):
        b = bytearray(blob); b[off] ^= 0x20
        assert _code(vt, S.restamp(bytes(b))) == FORMAT, "magic"
    for off in (4, 7):
        b = bytearray(blob); b[off] ^= 0x01
        assert _code(vt, S.restamp(bytes(b))) == FORMAT, "version"
    # sizes that do not add up, with a good checksum each
    for field, v in (("total_bytes", len(blob) + 16), ("header_bytes", 160), ("state_bytes", 92), ("policy_bytes", 12),
                     ("rows_bytes", 24576 - 128), ("rows_bytes", 0xfffffff0), ("tokens_template", 15), ("kpad", 704),
                     ("patch", 0), ("patch", 17), ("template_size", 1 << 20), ("search_size", 100)):
        assert _code(vt, _edit(vt, blob, S.HEADER, 0, **{field: v})) == FORMAT, (field, v)


def test_one_flipped_bit_anywhere_is_a_checksum_mismatch(vt):
    S = vt.snapshot
    blob, _ = _tiny(vt)
    for off in (S.STATE_OFF + 2, S.STATE_OFF + 87, S.POLICY_OFF + 5, S.ROWS_OFF, S.ROWS_OFF + 12345, len(blob) - 1, 53,
                S.CHECKSUM_OFF + 3):         # 53: a mantissa byte of norm_a[0]
        b = bytearray(blob); b[off] ^= 0x04
        assert _code(vt, bytes(b)) == FORMAT, off
        assert "checksum" in vt.lib().vt_last_error().decode(), off


def test_reserved_words_and_flag_bits_must_be_zero(vt):
    S = vt.snapshot
    blob, _ = _tiny(vt)
    res = np.zeros(16, np.uint32); res[9] = 1
    assert _code(vt, _edit(vt, blob, S.HEADER, 0, reserved=res)) == FORMAT
    assert _code(vt, _edit(vt, blob, S.HEADER, 0, reserved0=7)) == FORMAT
    assert _code(vt, _edit(vt, blob, S.HEADER, 0, flags=2)) == FORMAT
    assert _code(vt, _edit(vt, blob, S.HEADER, 0, flags=1)) == 0
    assert _code(vt, _edit(vt, blob, S.POLICY, S.POLICY_OFF, reserved=1)) == FORMAT


INF, NAN = float("inf"), float("nan")
BAD_STATES = [dict(initialized=0), dict(initialized=2), dict(box=(NAN, 0, 10, 10)), dict(box=(0, 0, 0.5, 10)),
              dict(box=(0, 0, 10, 40000)), dict(box=(70000, 0, 10, 10)), dict(geo=(0, INF, 1, 1)), dict(last_fbox=(0, 0, NAN, 1)),
              dict(last_score=NAN), dict(last_score=-INF), dict(frame_w=15), dict(frame_h=65537), dict(frames_done=-1),
              dict(success_count=8), dict(success_count=-1), dict(last_idx=64), dict(last_idx=-1), dict(tpl_gen=-1),
              dict(tpl_frame=8), dict(tpl_frame=-1), dict(window_miss=9), dict(window_miss=-1)]


@pytest.mark.parametrize("bad", BAD_STATES, ids=[f"{i}-" + "-".join(d) for i, d in enumerate(BAD_STATES)])
def test_a_state_no_pass_could_have_left_is_refused_with_a_good_checksum(vt, bad):
    blob, _ = _tiny(vt, state=_state(**bad))
    assert vt.snapshot.parse(blob)["checksum_ok"]
    assert _code(vt, blob) == FORMAT, bad


def test_state_values_on_the_edge_of_the_ranges_are_accepted(vt):
    for ok in (dict(success_count=7), dict(last_idx=63), dict(tpl_frame=7), dict(window_miss=8), dict(window_miss=0),
               dict(frame_w=16, frame_h=65536), dict(box=(-65536.0, 65536.0, 1.0, 32768.0))):
        assert _code(vt, _tiny(vt, state=_state(**ok))[0]) == 0, ok


@pytest.mark.parametrize("pol", [dict(period=1), dict(period=-2), dict(period=1000001), dict(period=2, min_score=NAN),
                                 dict(period=2, min_score=1.5), dict(period=0, min_score=-0.25), dict(period=3, skipped_geometry=-1)],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_a_policy_set_refresh_would_refuse_is_refused(vt, pol):
    assert _code(vt, _tiny(vt, policy=pol)[0]) == FORMAT
    assert _code(vt, _tiny(vt, policy=dict(period=1000000, min_score=1.0))[0]) == 0


def test_a_non_finite_row_element_is_refused(vt):
    _, rows = _tiny(vt)
    for bits, where in ((0x7fc0, (3, 100)), (0x7f80, (0, 0)), (0xff80, (15, 767)), (0xffff, (7, 1))):
        r = rows.copy()
        r[where] = bits
        assert _code(vt, _tiny(vt, rows=r)[0]) == FORMAT, hex(bits)
    r = rows.copy()
    r[0, 0], r[1, 1] = 0x7f7f, 0x8000          # the largest finite bf16 and minus zero are values like any other
    assert _code(vt, _tiny(vt, rows=r)[0]) == 0


def test_null_pointers_are_invalid_arguments(vt):
    L = vt.lib()
    blob, _ = _tiny(vt)
    d = vt.CSnapshotDesc()
    assert L.vt_snapshot_info(None, len(blob), ctypes.byref(d)) == INVALID
    assert L.vt_snapshot_info(blob, len(blob), None) == INVALID
    n = ctypes.c_size_t(0)
    assert L.vt_group_export_stream(None, 0, None, 0, ctypes.byref(n)) == INVALID
    assert L.vt_group_import_stream(None, 0, blob, len(blob)) == INVALID
    assert L.vt_group_copy_stream(None, 0, None, 1) == INVALID
    assert L.vt_export_state(None, None, 0, None) == INVALID
    assert L.vt_import_state(None, blob, len(blob)) == INVALID
    assert L.vt_group_snapshot_bytes(None) == 0
    with pytest.raises(vt.VtError) as e:
        vt.snapshot_info(blob[:100])
    assert e.value.code == FORMAT


def test_the_new_functions_are_exported_and_bound_everywhere(vt):
    L = ctypes.CDLL(vt.LIB_PATH)
    _, cf = parse_header()
    rs, rf, consts = parse_sys_rs()
    for name in NEW:
        assert hasattr(L, name) and name in vt.EXPORTS, name
        assert rf[name] == cf[name], name
    assert cf["vt_group_export_stream"] == ("i32", ["ptr", "i32", "ptr", "usize", "ptr"])
    assert cf["vt_group_copy_stream"] == ("i32", ["ptr", "i32", "ptr", "i32"])
    assert cf["vt_group_snapshot_bytes"] == ("usize", ["ptr"])
    # one layout of vt_snapshot_desc in C, ctypes and Rust
    cs, _ = parse_header()
    assert ctypes.sizeof(vt.CSnapshotDesc) == 128 and rs["VtSnapshotDesc"] == cs["vt_snapshot_desc"]
    assert _size(rs["VtSnapshotDesc"], cs) == 128
    assert [f[0] for f in vt.CSnapshotDesc._fields_] == [f[0] for f in cs["vt_snapshot_desc"]]
    spec = importlib.util.spec_from_file_location("_vt_build", os.path.join(ROOT, "gstreamer-vit-tracker_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    out = subprocess.run([b.build_c_client(), "sizes"], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[0::2], (int(x) for x in out[1::2])))
    assert got["vt_snapshot_desc"] == 128 and got["abi"] == 5
    # additions only: the version stays
    hdr = open(os.path.join(ROOT, "include", "vittrack_hip.h")).read()
    assert int(re.search(r"#define VT_ABI_VERSION (\d+)", hdr).group(1)) == 5 and int(consts["VT_ABI_VERSION"]) == 5
    for cls, names in ((vt.Group, ("export_stream", "import_stream", "copy_stream")), (vt.VitTrack, ("export_state", "import_state"))):
        for n in names:
            assert callable(getattr(cls, n)), n
