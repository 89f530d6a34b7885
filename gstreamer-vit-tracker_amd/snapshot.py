"""Stream snapshots in NumPy: the byte format of include/vittrack_hip.h ("stream snapshots") stated a second time.

`pack` builds the byte string vt_group_export_stream writes, `parse` takes one apart, `checksum` is its FNV-1a-64.
Nothing here touches the GPU or the library: the CPU tests pack snapshots with it and hand them to vt_snapshot_info, a
host tool can inspect or re-stamp a snapshot with it. It validates nothing but the sizes it needs to slice - the
library's vt_snapshot_info is the validator.
"""
from __future__ import annotations

import numpy as np

MAGIC = b"VTSS"
VERSION = b"0001"
HEADER_BYTES = 152
STATE_BYTES = 88
POLICY_BYTES = 16
STATE_OFF = HEADER_BYTES
POLICY_OFF = STATE_OFF + STATE_BYTES
ROWS_OFF = POLICY_OFF + POLICY_BYTES          # 256
CHECKSUM_OFF = 80
FLAG_ANY_GRAPHS = 1

HEADER = np.dtype([("magic", "S4"), ("version", "S4"), ("total_bytes", "<u4"), ("header_bytes", "<u4"),
                   ("state_bytes", "<u4"), ("policy_bytes", "<u4"), ("rows_bytes", "<u4"), ("flags", "<u4"),
                   ("patch", "<i4"), ("template_size", "<i4"), ("search_size", "<i4"), ("kpad", "<i4"),
                   ("tokens_template", "<i4"), ("norm_a", "<f4", 3), ("norm_b", "<f4", 3), ("reserved0", "<u4"),
                   ("checksum", "<u8"), ("reserved", "<u4", 16)])
# the device's StreamState record (csrc/vt_frame.hpp), 22 words
STATE = np.dtype([("box", "<f4", 4), ("geo", "<f4", 4), ("frame_w", "<i4"), ("frame_h", "<i4"), ("initialized", "<i4"),
                  ("frames_done", "<i4"), ("success_count", "<i4"), ("last_idx", "<i4"), ("last_fbox", "<f4", 4),
                  ("last_score", "<f4"), ("window_miss", "<i4"), ("tpl_gen", "<i4"), ("tpl_frame", "<i4")])
POLICY = np.dtype([("period", "<i4"), ("min_score", "<f4"), ("skipped_geometry", "<i4"), ("reserved", "<i4")])
assert HEADER.itemsize == HEADER_BYTES and STATE.itemsize == STATE_BYTES and POLICY.itemsize == POLICY_BYTES
assert HEADER.fields["checksum"][1] == CHECKSUM_OFF


def snapshot_bytes(tokens_template: int, kpad: int) -> int:
    """size of a snapshot of a model with that many template tokens and that padded patch length"""
    return ROWS_OFF + 2 * int(tokens_template) * int(kpad)


def checksum(blob: bytes) -> int:
    """FNV-1a-64 over the whole string with the checksum field read as zero"""
    b = np.frombuffer(bytes(blob), np.uint8).copy()
    if len(b) >= CHECKSUM_OFF + 8:
        b[CHECKSUM_OFF:CHECKSUM_OFF + 8] = 0
    h, prime, mask = 0xcbf29ce484222325, 0x100000001b3, (1 << 64) - 1
    for v in b.tolist():
        h = ((h ^ v) * prime) & mask
    return h


def restamp(blob: bytes) -> bytes:
    """the same bytes with the checksum recomputed (after editing a field)"""
    b = bytearray(blob)
    b[CHECKSUM_OFF:CHECKSUM_OFF + 8] = int(checksum(bytes(b))).to_bytes(8, "little")
    return bytes(b)


def pack(geometry: dict, state, policy, rows, flags: int = 0) -> bytes:
    """geometry: patch, template_size, search_size, kpad, tokens_template, norm_a[3], norm_b[3]; state: a STATE record
    (or a dict of its fields, missing ones zero); policy: a POLICY record, a dict or None (all zero); rows: the template
    rows as bf16 bit patterns, tokens_template x kpad uint16"""
    rows = np.ascontiguousarray(rows, "<u2").reshape(-1)
    nt, kpad = int(geometry["tokens_template"]), int(geometry["kpad"])
    if rows.size != nt * kpad:
        raise ValueError(f"{rows.size} row elements for {nt} x {kpad}")
    h = np.zeros((), HEADER)
    h["magic"], h["version"] = MAGIC, VERSION
    h["header_bytes"], h["state_bytes"], h["policy_bytes"], h["rows_bytes"] = HEADER_BYTES, STATE_BYTES, POLICY_BYTES, 2 * rows.size
    h["total_bytes"] = snapshot_bytes(nt, kpad)
    h["flags"] = flags
    for k in ("patch", "template_size", "search_size", "kpad", "tokens_template", "norm_a", "norm_b"):
        h[k] = geometry[k]
    blob = h.tobytes() + _record(state, STATE).tobytes() + _record(policy, POLICY).tobytes() + rows.tobytes()
    return restamp(blob)


def _record(v, dtype):
    if isinstance(v, np.ndarray) and v.dtype == dtype:
        return v.reshape(())
    r = np.zeros((), dtype)
    for k, x in (v or {}).items():
        r[k] = x
    return r


def parse(blob: bytes) -> dict:
    """header, state and policy as NumPy records, rows as uint16 [tokens_template, kpad], checksum_ok"""
    blob = bytes(blob)
    if len(blob) < ROWS_OFF:
        raise ValueError("snapshot shorter than its fixed part")
    h = np.frombuffer(blob, HEADER, 1)[0]
    if int(h["total_bytes"]) != len(blob) or int(h["rows_bytes"]) != len(blob) - ROWS_OFF:
        raise ValueError("snapshot sizes do not add up")
    rows = np.frombuffer(blob, "<u2", int(h["rows_bytes"]) // 2, ROWS_OFF)
    if int(h["tokens_template"]) > 0 and rows.size % int(h["tokens_template"]) == 0:
        rows = rows.reshape(int(h["tokens_template"]), -1)
    return dict(header=h, state=np.frombuffer(blob, STATE, 1, STATE_OFF)[0], policy=np.frombuffer(blob, POLICY, 1, POLICY_OFF)[0],
                rows=rows, checksum_ok=int(h["checksum"]) == checksum(blob))


def geometry_of(cfg) -> dict:
    """the geometry block of a weights.ModelConfig (or its name)"""
    from . import weights
    if isinstance(cfg, str):
        cfg = weights.get_config(cfg)
    a, b = weights.norm_constants()
    return dict(patch=cfg.patch, template_size=cfg.template, search_size=cfg.search, kpad=cfg.kpad, tokens_template=cfg.n_t,
                norm_a=a, norm_b=b)
