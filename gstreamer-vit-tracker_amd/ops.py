"""Operator-level test hooks — Python bindings over include/vittrack_hip_ops.h (libvittrack_hip_ops.so: the product's
objects + csrc/vt_ops.hip). For numerics tests and tuning tools only: the product path (VitTrack, Group, bench.py, the
harness) never loads this library. The package re-exports every name here, so callers write vt.op_*.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_float, c_int, c_int8, c_int32, c_uint16, c_uint32, c_void_p

import numpy as np

from . import (PKG_DIR, PEAKS_DTYPE, CFrame, VtError, lib, _f32, _u16)
from .snapshot import STATE

# a library of its own; a tuning build named by VITTRACK_HIP_LIB carries the entry points too
OPS_LIB_PATH = os.environ.get("VITTRACK_HIP_OPS_LIB") or os.environ.get("VITTRACK_HIP_LIB") or \
    os.path.join(PKG_DIR, "libvittrack_hip_ops.so")

# every symbol include/vittrack_hip_ops.h declares (libvittrack_hip_ops.so; the product library exports none of them)
OPS_EXPORTS = [
    "vt_op_gemm_bench", "vt_op_qkv_bf16", "vt_op_attention_bf16",
    "vt_op_attention_bench", "vt_op_layernorm", "vt_op_nv12_to_rgb8_bench", "vt_op_nv12_to_rgb8_batch_bench", "vt_op_conv3x3_relu_bf16", "vt_op_headconv_bf16",
    "vt_op_gemm_bf16_lo", "vt_op_headconv_ln_bf16_lo",
    "vt_op_gemm_resid_seg_bf16", "vt_op_attention_queries_bf16", "vt_op_head_decode", "vt_op_response_peaks", "vt_op_result_overlay",
    "vt_op_motion_prior", "vt_op_appearance_score", "vt_op_proposals", "vt_op_camera_motion", "vt_op_ln_chain_bf16",
    "vt_op_stream_conflicts", "vt_op_frame_health", "vt_op_arbitrate", "vt_op_movers",
]

_ops = None


def ops_lib():
    """Load libvittrack_hip_ops.so: the product's objects + the operator-level entry points (tests, tuning tools)."""
    global _ops
    if _ops is not None:
        return _ops
    if not os.path.exists(OPS_LIB_PATH):
        raise VtError(-2, f"{OPS_LIB_PATH} not built: run `python __graft_entry__.py`")
    lib()       # torch / HIP runtime first, as in lib()
    L = ctypes.CDLL(OPS_LIB_PATH)
    L.vt_last_error.restype = c_char_p
    u16p, fp, i8p, i32p = POINTER(c_uint16), POINTER(c_float), POINTER(c_int8), POINTER(c_int32)
    L.vt_op_gemm_bf16_lo.argtypes = [c_int, u16p, u16p, fp, fp, c_int, c_int, c_int, c_int, c_int, fp, fp, fp, c_float, c_int]
    L.vt_op_gemm_bench.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, c_int, fp]
    L.vt_op_qkv_bf16.argtypes = [c_int, u16p, u16p, fp, fp, fp, c_int, c_int, c_int, c_int, c_int, fp, fp]
    L.vt_op_attention_bf16.argtypes = [c_int, u16p, u16p, u16p, fp, c_int, c_int, c_int, c_int]
    L.vt_op_attention_bench.argtypes = [c_int, c_int, c_int, c_int, c_int, c_int, fp]
    L.vt_op_attention_queries_bf16.argtypes = [c_int, u16p, u16p, u16p, fp, c_int, c_int, c_int, c_int, c_int]
    L.vt_op_gemm_resid_seg_bf16.argtypes = [c_int, u16p, u16p, fp, u16p, i8p, c_int, u16p, i8p, fp, fp, c_int, c_int, c_int,
                                            c_int, c_int, c_float, c_int]
    L.vt_op_layernorm.argtypes = [c_int, fp, fp, fp, fp, c_int, c_int]
    L.vt_op_ln_chain_bf16.argtypes = [c_int, fp, c_int, c_int, c_int, u16p, fp, fp, fp, c_int, c_int, c_int, c_int, c_int, c_float,
                                      c_int, c_int, fp, fp, u16p, i8p, fp, fp, u16p, fp, fp]
    L.vt_op_conv3x3_relu_bf16.argtypes = [c_int, u16p, u16p, fp, fp, c_int, c_int, c_int, c_int, c_int]
    L.vt_op_nv12_to_rgb8_bench.argtypes = [c_int, c_int, c_int, c_int, fp]
    L.vt_op_nv12_to_rgb8_batch_bench.argtypes = [c_int, c_int, c_int, c_int, c_int, fp]
    L.vt_op_head_decode.argtypes = [c_int, c_int, u16p, u16p, fp, fp, fp, fp, c_void_p, c_int, i32p, c_float,
                                    c_int, c_int, c_int, c_int, c_int, c_int, fp, c_void_p, c_void_p, c_void_p,
                                    POINTER(c_uint32)]
    L.vt_op_response_peaks.argtypes = [c_int, fp, fp, c_void_p, c_int, c_void_p, i32p, i32p, c_int,
                                       c_int, c_void_p, c_void_p]
    L.vt_op_motion_prior.argtypes = [c_int, c_void_p, c_void_p, c_int, i32p, c_void_p, i32p, i32p,
                                     c_void_p, c_int, c_int, c_void_p, c_void_p]
    L.vt_op_appearance_score.argtypes = [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]
    L.vt_op_proposals.argtypes = [c_int, POINTER(CFrame), c_void_p, c_int, c_void_p, i32p, i32p, c_int,
                                  c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]
    L.vt_op_camera_motion.argtypes = [c_int, POINTER(CFrame), c_void_p, c_int, i32p, c_int, i32p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]
    L.vt_op_frame_health.argtypes = [c_int, POINTER(CFrame), c_void_p, c_int, i32p, c_int, i32p, c_int, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]
    L.vt_op_movers.argtypes = [c_int, POINTER(CFrame), c_void_p, c_int, i32p, c_int, i32p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
    L.vt_op_arbitrate.argtypes = [c_int, fp, fp, POINTER(CFrame), c_void_p, c_int, c_void_p, i32p, i32p, c_int, c_int, c_void_p,
                                  c_int, c_int, c_int, c_int, fp, c_float, i32p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p]
    L.vt_op_stream_conflicts.argtypes = [c_int, c_void_p, c_int, c_void_p, i32p, i32p, c_int, i32p, i32p, c_void_p, c_void_p,
                                         c_void_p]
    L.vt_op_result_overlay.argtypes = [c_int, POINTER(CFrame), c_void_p, i32p, i32p, c_int, c_void_p, c_void_p,
                                       c_int, c_int]
    _ops = L
    return L


def _check_op(rc):
    if rc < 0:
        raise VtError(rc, ops_lib().vt_last_error().decode(errors="replace"))
    return rc


def _i8(a):
    return a.ctypes.data_as(POINTER(c_int8))


def _i32(a):
    return a.ctypes.data_as(POINTER(c_int32))


def _vp(a):
    return a.ctypes.data_as(c_void_p)


def _opt(a, conv=_f32):
    """the pointer of an optional operand: None stays None (a null pointer)"""
    return None if a is None else conv(a)


def _arr(a, dtype):
    """an optional operand as a contiguous array of dtype"""
    return None if a is None else np.ascontiguousarray(a, dtype)


def _frames(frames):
    """the frames of the slots as one C array -> (n, array)"""
    n = len(frames)
    return n, (CFrame * n)(*frames)


def _maps(n, slot_stream, winner=None):
    """the two optional maps of n slots: slot -> stream, and a candidate pass's winner table"""
    smap, win = _arr(slot_stream, np.int32), _arr(winner, np.int32)
    assert (smap is None or smap.shape == (n,)) and (win is None or win.shape == (n,))
    return smap, win


def _start(a, dtype, shape=None, fill=0):
    """an array a hook starts from and writes into, as a copy of the caller's a or (None) every byte `fill`. shape (n,): n
    records, flattened from whatever shape they come in; shape None: records, however many"""
    if a is None:
        return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, fill, np.uint8).view(dtype).reshape(shape)
    r = np.ascontiguousarray(a, dtype).copy()
    if shape is None or len(shape) == 1:
        r = r.reshape(-1)
    assert shape is None or r.shape == tuple(shape)
    return r


def _mirror(host, dtype, n):
    """what a pinned mirror of n records holds before the call; None: that mirror is null"""
    return None if host is None else _start(host, dtype, (n,))


def _timed(fn, *args) -> float:
    """a timing hook's value: its trailing us_out"""
    us = c_float()
    _check_op(fn(*args, byref(us)))
    return float(us.value)


# ---- the GEMMs and their epilogues -----------------------------------------------------------------

def op_gemm_bf16(a_bits, w_bits, bias, c_init=None, epilogue=0, device=0, cfg=-1, rowstat=None,
                 colsum=None, want_rowstat=False, eps=1e-6, lo_shift=12):
    """vt_op_gemm_bf16_lo. epilogue 0 / 1 / 4: the X-epilogues (x comes back as the value of the 3-byte pair the
    engine stores, its quantum 2^-lo_shift; want_rowstat: also the finalized (rstd, -mean * rstd) per row -> (x, rowstat));
    2 / 3: GELU / ReLU to bf16, with a folded LayerNorm if rowstat [M,2] and colsum [N] are given"""
    a_bits = np.ascontiguousarray(a_bits, np.uint16)
    w_bits = np.ascontiguousarray(w_bits, np.uint16)
    M, K = a_bits.shape
    N = w_bits.shape[0]
    c = np.zeros((M, N), np.float32) if c_init is None else np.ascontiguousarray(c_init,
                                                                                 np.float32).copy()
    b, rs, cs = _arr(bias, np.float32), _arr(rowstat, np.float32), _arr(colsum, np.float32)
    ro = np.zeros((M, 2), np.float32) if want_rowstat else None
    _check_op(ops_lib().vt_op_gemm_bf16_lo(device, _u16(a_bits), _u16(w_bits), _opt(b), _f32(c), M, N, K, epilogue, cfg,
                                           _opt(rs), _opt(cs), _opt(ro), eps, int(lo_shift)))
    return (c, ro) if want_rowstat else c


def op_ln_chain_bf16(x, B, tokens, w_bits, gamma, beta, bias, consumer, route=0, producer_cfg=-1, consumer_cfg=-1,
                     eps=1e-6, lo_shift=12, launches=1, device=0, check=True):
    """vt_op_ln_chain_bf16: the folded LayerNorm as the engine runs it - X-epilogue producer on x [B * tokens, D], row terms
    by route (0 finalize launch, 1 inside the 256x256 producer, 2 combined in the consumer), the fold of w_bits [N, D] /
    gamma / beta / bias, then the consumer (2 GELU, 3 ReLU, 4 QKV; 0: the fold alone, x may be None). Returns a dict of
    rc, out, vt, xh (uint16), xl (int8), cstat [M, D // 32, 2], rowstat [M, 2], wf (uint16), colsum, cvec; every array
    starts as 0xff bytes, and stays so when the call is refused (check=False returns rc instead of raising)"""
    w_bits = np.ascontiguousarray(w_bits, np.uint16)
    N, D = w_bits.shape
    g, be, bi = (np.ascontiguousarray(v, np.float32) for v in (gamma, beta, bias))
    assert g.shape == (D,) and be.shape == (D,) and bi.shape == (N,)
    M = B * tokens if consumer else 0
    xx = None
    if consumer:
        xx = np.ascontiguousarray(x, np.float32)
        assert xx.shape == (M, D)
    npad = (tokens + 63) // 64 * 64
    def ff(shape, dt):
        return np.full(int(np.prod(shape)) * np.dtype(dt).itemsize, 0xff, np.uint8).view(dt).reshape(shape)
    r = dict(out=ff((M, 2 * D if consumer == 4 else N), np.float32),
             vt=ff((B * (D // 64), 64, npad) if consumer == 4 else (0, 64, npad), np.float32),
             xh=ff((M, D), np.uint16), xl=ff((M, D), np.int8), cstat=ff((M, max(D // 32, 1), 2), np.float32),
             rowstat=ff((M, 2), np.float32), wf=ff((N, D), np.uint16), colsum=ff((N,), np.float32), cvec=ff((N,), np.float32))
    p = lambda a, conv: conv(a) if a.size else None
    rc = ops_lib().vt_op_ln_chain_bf16(device, _opt(xx), B, tokens, D, _u16(w_bits), _f32(g), _f32(be),
                                       _f32(bi), N, consumer, route, producer_cfg, consumer_cfg, eps, int(lo_shift), launches,
                                       p(r["out"], _f32), p(r["vt"], _f32), p(r["xh"], _u16), p(r["xl"], _i8),
                                       p(r["cstat"], _f32), p(r["rowstat"], _f32), _u16(r["wf"]), _f32(r["colsum"]),
                                       _f32(r["cvec"]))
    if check:
        _check_op(rc)
    r["rc"] = rc
    return r


def op_gemm_bench(M, N, K, epilogue, cfg=-1, iters=50, device=0) -> float:
    return _timed(ops_lib().vt_op_gemm_bench, device, M, N, K, epilogue, cfg, iters)


def op_qkv_bf16(a_bits, w_bits, bias, B, tokens, D, device=0, cfg=-1, vt_perm=0, rowstat=None,
                colsum=None):
    a_bits = np.ascontiguousarray(a_bits, np.uint16)
    w_bits = np.ascontiguousarray(w_bits, np.uint16)
    bias = np.ascontiguousarray(bias, np.float32)
    npad = (tokens + 63) // 64 * 64
    qk = np.empty((B * tokens, 2 * D), np.float32)
    vt = np.empty((B * (D // 64), 64, npad), np.float32)
    rs, cs = _arr(rowstat, np.float32), _arr(colsum, np.float32)
    _check_op(ops_lib().vt_op_qkv_bf16(device, _u16(a_bits), _u16(w_bits), _f32(bias), _f32(qk),
                                       _f32(vt), B, tokens, D, cfg, vt_perm, _opt(rs), _opt(cs)))
    return qk, vt


def op_gemm_resid_seg(a_bits, w_bits, bias, xh_bits, xl_lo8, M, seg_rows=0, seg_skip=0, eps=1e-6, lo_shift=12, device=0):
    """vt_op_gemm_resid_seg_bf16: the residual GEMM of the 256x256 kernel on the stored pair xh_bits (uint16) / xl_lo8 (int8)
    [rows_in, N], output row m taking its addend from input row m + (m // seg_rows + 1) * seg_skip (seg_rows = 0: rows
    0 .. M-1, in place) -> (xh [M, N] uint16, xl [M, N] int8, chunk partials [M, N // 32, 2], row terms [M, 2])"""
    a_bits = np.ascontiguousarray(a_bits, np.uint16)
    w_bits = np.ascontiguousarray(w_bits, np.uint16)
    xh = np.ascontiguousarray(xh_bits, np.uint16)
    xl = np.ascontiguousarray(xl_lo8, np.int8)
    K, N = a_bits.shape[1], w_bits.shape[0]
    assert a_bits.shape[0] == M and xh.shape == xl.shape and xh.shape[1] == N
    b = _arr(bias, np.float32)
    oh, ol = np.empty((M, N), np.uint16), np.empty((M, N), np.int8)
    cst, ro = np.empty((M, N // 32, 2), np.float32), np.empty((M, 2), np.float32)
    _check_op(ops_lib().vt_op_gemm_resid_seg_bf16(device, _u16(a_bits), _u16(w_bits), _opt(b), _u16(xh), _i8(xl), xh.shape[0],
                                                  _u16(oh), _i8(ol), _f32(cst), _f32(ro), M, N, K, int(seg_rows),
                                                  int(seg_skip), c_float(eps), int(lo_shift)))
    return oh, ol, cst, ro


# ---- attention, pixel conversion, LayerNorm ------------------------------------------------------------

def op_attention_bf16(q_bits, k_bits, v_bits, B, N, H, device=0, mode=-1):
    q_bits, k_bits, v_bits = (np.ascontiguousarray(x, np.uint16) for x in (q_bits, k_bits, v_bits))
    out = np.empty((B * N, H * 64), np.float32)
    _check_op(ops_lib().vt_op_attention_bf16(device, _u16(q_bits), _u16(k_bits), _u16(v_bits), _f32(out),
                                             B, N, H, mode))
    return out


def op_attention_queries(q_bits, k_bits, v_bits, B, N, H, q0, nq, device=0):
    """vt_op_attention_queries_bf16: attention mode 3 on the queries q0 .. q0 + nq - 1 of every stream -> [B * nq, H * 64]"""
    q_bits, k_bits, v_bits = (np.ascontiguousarray(x, np.uint16) for x in (q_bits, k_bits, v_bits))
    out = np.empty((B * nq, H * 64), np.float32)
    _check_op(ops_lib().vt_op_attention_queries_bf16(device, _u16(q_bits), _u16(k_bits), _u16(v_bits), _f32(out),
                                                     B, N, H, int(q0), int(nq)))
    return out


def op_attention_bench(B, N, H, mode=-1, iters=30, device=0) -> float:
    return _timed(ops_lib().vt_op_attention_bench, device, B, N, H, mode, iters)


def op_nv12_to_rgb8_bench(w, h, iters=50, device=0) -> float:
    """mean microseconds per launch of the whole-frame NV12 -> RGB8 converter (device-resident)"""
    return _timed(ops_lib().vt_op_nv12_to_rgb8_bench, device, w, h, iters)


def op_nv12_to_rgb8_batch_bench(w, h, n, iters=20, device=0) -> float:
    """mean microseconds per launch of the n-frames-per-launch converter on device-resident random frames"""
    return _timed(ops_lib().vt_op_nv12_to_rgb8_batch_bench, device, w, h, n, iters)


def op_layernorm(x, gamma, beta, device=0):
    x = np.ascontiguousarray(x, np.float32)
    g = np.ascontiguousarray(gamma, np.float32)
    b = np.ascontiguousarray(beta, np.float32)
    y = np.empty_like(x)
    _check_op(ops_lib().vt_op_layernorm(device, _f32(x), _f32(g), _f32(b), _f32(y), x.shape[0],
                                        x.shape[1]))
    return y


# ---- the head -----------------------------------------------------------------------------------------

def op_conv3x3_relu(t_bf16_bits, w_bf16_bits, bias, B, grid, cfg=-1, device=0):
    """vt_op_conv3x3_relu_bf16: relu(conv3x3(t) + bias) as the implicit GEMM of the head; t [B*grid*grid][C],
    w [N][9*C] as uint16 bf16 bit patterns -> [B*grid*grid][N] float32 (bf16 values)"""
    t = np.ascontiguousarray(t_bf16_bits, np.uint16)
    w = np.ascontiguousarray(w_bf16_bits, np.uint16)
    C, N = t.shape[1], w.shape[0]
    out = np.empty((t.shape[0], N), np.float32)
    _check_op(ops_lib().vt_op_conv3x3_relu_bf16(device, _u16(t), _u16(w), _f32(np.ascontiguousarray(bias, np.float32)),
                                                _f32(out), B, grid, C, N, cfg))
    return out


def op_headconv(t_bf16_bits, w_bf16_bits, bias, B, grid, conv3x3=True, R=0, ncb=0, device=0):
    """vt_op_headconv_bf16: the head's band kernel (k_head.hip) on given operands -> [B*grid*grid][N] float32"""
    t = np.ascontiguousarray(t_bf16_bits, np.uint16)
    w = np.ascontiguousarray(w_bf16_bits, np.uint16)
    Cin, N = t.shape[1], w.shape[0]
    out = np.empty((t.shape[0], N), np.float32)
    _check_op(ops_lib().vt_op_headconv_bf16(device, _u16(t), _u16(w), _f32(np.ascontiguousarray(bias, np.float32)), _f32(out),
                                            B, grid, Cin, N, 1 if conv3x3 else 0, R, ncb, 0, None))
    return out


def op_headconv_bench(B, grid, Cin, N, conv3x3=True, R=0, ncb=0, iters=50, device=0) -> float:
    """mean microseconds per launch of the band kernel on pseudo-random operands"""
    return _timed(ops_lib().vt_op_headconv_bf16, device, None, None, None, None, B, grid, Cin, N, 1 if conv3x3 else 0, R, ncb,
                  iters)


def op_headconv_ln(xh_bits, xl_lo8, gamma, beta, w_bf16_bits, bias, B, grid, ntok, off, fused=True, eps=1e-6, R=0, ncb=0,
                   device=0, lo_shift=12):
    """vt_op_headconv_ln_bf16_lo: relu(LayerNorm(xh + lo8 * 2^-lo_shift)[search rows] . w^T + bias) -> [B*grid*grid][N] float32 (the
    residual pair of specification v3: bf16 bits + signed bytes); fused: one launch (the band kernel normalises its rows
    itself), else the LayerNorm kernel followed by the band kernel"""
    xh = np.ascontiguousarray(xh_bits, np.uint16)
    xl = np.ascontiguousarray(xl_lo8, np.int8)
    w = np.ascontiguousarray(w_bf16_bits, np.uint16)
    D, N = xh.shape[1], w.shape[0]
    assert xh.shape == xl.shape == (B * ntok, D) and w.shape[1] == D
    out = np.empty((B * grid * grid, N), np.float32)
    _check_op(ops_lib().vt_op_headconv_ln_bf16_lo(device, _u16(xh), _i8(xl), _f32(np.ascontiguousarray(gamma, np.float32)),
                                                  _f32(np.ascontiguousarray(beta, np.float32)), c_float(eps), ntok, off,
                                                  _u16(w), _f32(np.ascontiguousarray(bias, np.float32)), _f32(out),
                                                  B, grid, D, N, 1 if fused else 0, R, ncb, 0, None, int(lo_shift)))
    return out


def op_headconv_ln_bench(B, grid, D, N, ntok, off, fused=True, R=0, ncb=0, iters=50, device=0) -> float:
    """mean microseconds of the head's first layer with the final LayerNorm (fused: one launch, else two)"""
    us = c_float()
    _check_op(ops_lib().vt_op_headconv_ln_bf16_lo(device, None, None, None, None, c_float(1e-6), ntok, off, None, None, None, B,
                                                  grid, D, N, 1 if fused else 0, R, ncb, iters, byref(us), 12))
    return float(us.value)


# vt_result as the decode writes it (include/vittrack_hip.h), 6 words
RESULT_DTYPE = np.dtype([("success", "<i4"), ("score", "<f4"), ("bbox", "<i4", 4)])


def op_head_decode(t_bf16_bits, w4, b4, hann, states, B, grid, form=0, w3_bf16_bits=None, b3=None, slot_stream=None,
                   success_threshold=0.5, R=0, launches=1, host_results=True, host_states=True, mirror_fill=0xA5, device=0):
    """vt_op_head_decode: the decode stage (k_head.hip) on given operands. form 0: head_out_kernel + decode_kernel on
    t = t3 [B*grid*grid][C]; form 1: the last 3x3 layer (w3 [C][9C], b3 [C]) on the band kernel with the fused tail, R rows
    per band (<= 0: the launcher's plan), `launches` launches on the same buffers. states: snapshot.STATE records (raw 88-byte
    StreamState), indexed by stream; slot_stream [B]: slot -> stream (None: the identity). The two pinned host mirrors start
    filled with the byte mirror_fill; host_results / host_states False runs with that mirror null. -> dict(head_out
    [B*ns][8] float32, results / host_results [B] RESULT_DTYPE, states / host_states [n_states] snapshot.STATE, band_cnt [B]
    uint32)"""
    t = np.ascontiguousarray(t_bf16_bits, np.uint16)
    ns, C = grid * grid, t.shape[1]
    assert t.shape == (B * ns, C)
    w4 = np.ascontiguousarray(w4, np.float32)
    b4 = np.ascontiguousarray(b4, np.float32)
    hann = np.ascontiguousarray(hann, np.float32).reshape(-1)
    assert w4.shape == (8, C) and b4.shape == (8,) and hann.shape == (ns,)
    st = _start(states, STATE)
    w3 = b3a = None
    if form == 1:
        w3 = np.ascontiguousarray(w3_bf16_bits, np.uint16)
        b3a = np.ascontiguousarray(b3, np.float32)
        assert w3.shape == (C, 9 * C) and b3a.shape == (C,)
    smap, _ = _maps(B, slot_stream)
    out = dict(head_out=np.empty((B * ns, 8), np.float32), results=np.zeros(B, RESULT_DTYPE),
               host_results=_start(None, RESULT_DTYPE, (B,), mirror_fill), host_states=_start(None, STATE, (len(st),), mirror_fill),
               band_cnt=np.full(B, 0xFFFFFFFF, np.uint32))
    flags = (0 if host_results else 1) | (0 if host_states else 2)
    _check_op(ops_lib().vt_op_head_decode(
        device, int(form), _u16(t), _opt(w3, _u16), _opt(b3a), _f32(w4), _f32(b4),
        _f32(hann), _vp(st), len(st), _opt(smap, _i32),
        c_float(success_threshold), B, grid, C, int(R), int(launches), flags, _f32(out["head_out"]),
        _vp(out["results"]), _vp(out["host_results"]),
        _vp(out["host_states"]), out["band_cnt"].ctypes.data_as(POINTER(c_uint32))))
    out["states"] = st
    return out


# ---- the in-the-pass launches -------------------------------------------------------------------------

# vt_peaks_policy: the 16-byte per-stream policy record (vt_peak / vt_peaks: PEAK_DTYPE / PEAKS_DTYPE of the package)
PEAKS_POLICY_DTYPE = np.dtype([("max_peaks", "<i4"), ("radius", "<i4"), ("min_resp", "<f4"), ("reserved", "<i4")])


def op_response_peaks(head_out, hann, states, policies, B, grid, slot_stream=None, winner=None, mirror_fill=0xA5, device=0):
    """vt_op_response_peaks: the response-peaks launch (k_peaks.hip) on given operands, nothing else. head_out [B*ns][8]
    float32 logits by slot, hann [ns], states: snapshot.STATE records by stream, policies: PEAKS_POLICY_DTYPE records by
    stream (or (max_peaks, radius, min_resp) for all), slot_stream [B]: slot -> stream (None: the identity), winner [B]: a
    candidate pass's winner table (None: every slot lists). Device records and pinned mirror start filled with the byte
    mirror_fill. -> dict(records / host_records [B] PEAKS_DTYPE, states [n_states] as they came back)"""
    ho = np.ascontiguousarray(head_out, np.float32)
    ns = grid * grid
    assert ho.shape == (B * ns, 8)
    hann = np.ascontiguousarray(hann, np.float32).reshape(-1)
    assert hann.shape == (ns,)
    st = _start(states, STATE)
    if isinstance(policies, tuple):
        pol = np.zeros(len(st), PEAKS_POLICY_DTYPE)
        pol["max_peaks"], pol["radius"], pol["min_resp"] = policies
    else:
        pol = np.ascontiguousarray(policies, PEAKS_POLICY_DTYPE).reshape(-1)
    assert len(pol) == len(st)
    smap, win = _maps(B, slot_stream, winner)
    out = dict(records=_start(None, PEAKS_DTYPE, (B,), mirror_fill), host_records=_start(None, PEAKS_DTYPE, (B,), mirror_fill))
    _check_op(ops_lib().vt_op_response_peaks(
        device, _f32(ho), _f32(hann), _vp(st), len(st), _vp(pol), _opt(smap, _i32), _opt(win, _i32),
        B, grid, _vp(out["records"]), _vp(out["host_records"])))
    out["states"] = st
    return out


# the motion prior's records (csrc/k_motion.hpp: MotionRec 48 bytes by stream, MotionPolicy 16 bytes per engine)
MOTION_REC_DTYPE = np.dtype([("v", "<f4", 2), ("prior", "<f4", 4), ("shift", "<f4", 2), ("live", "<i4"), ("n_shift", "<i4"),
                             ("n_coast", "<i4"), ("reserved", "<i4")])
CANDIDATE_DTYPE = np.dtype([("stream", "<i4"), ("has_box", "<i4"), ("box", "<f4", 4)])


def op_motion_prior(states, records, results, on=1, gain_pct=50, coast=5, max_pct=100, slot_stream=None, cands=None, winner=None,
                    stages=3, host_states=None, host_records=None, device=0):
    """vt_op_motion_prior: the place (stages & 1) and settle (stages & 2) launches of k_motion.hip on given operands,
    nothing else. states: snapshot.STATE records by stream, records: MOTION_REC_DTYPE by stream, results [n] RESULT_DTYPE by
    slot, slot_stream [n]: slot -> stream (None: the identity); the candidate form: cands [n] CANDIDATE_DTYPE + winner [n].
    host_states / host_records: what the pinned mirrors hold before (None: that mirror is null). -> dict(states, records,
    host_states, host_records) as they came back"""
    st = _start(states, STATE)
    rec = _start(records, MOTION_REC_DTYPE, (len(st),))
    res = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
    n = len(res)
    smap, win = _maps(n, slot_stream, winner)
    cd = None if cands is None else np.ascontiguousarray(cands, CANDIDATE_DTYPE).reshape(-1)
    assert cd is None or cd.shape == (n,)
    hst, hrec = _mirror(host_states, STATE, len(st)), _mirror(host_records, MOTION_REC_DTYPE, len(st))
    pol = np.array([on, gain_pct, coast, max_pct], np.int32)
    _check_op(ops_lib().vt_op_motion_prior(
        device, _vp(st), _vp(rec), len(st), _i32(pol), _vp(res), _opt(smap, _i32), _opt(win, _i32), _opt(cd, _vp), n, stages,
        _opt(hst, _vp), _opt(hrec, _vp)))
    return dict(states=st, records=rec, host_states=hst, host_records=hrec)


def op_appearance_score(anchor, probe, cols, device=0):
    """vt_op_appearance_score: the score launch of k_appearance.hip on given rows, nothing else. anchor, probe:
    [n_slots, nt, kpad] uint16 bf16 bit patterns; the sums run over columns [0, cols). -> dict(sums [n_slots, 5] float64 =
    Sa, Sp, Saa, Spp, Sap, similarity [n_slots] float32, status [n_slots] int32)"""
    a = np.ascontiguousarray(anchor, np.uint16)
    p = np.ascontiguousarray(probe, np.uint16)
    assert a.ndim == 3 and a.shape == p.shape
    n, nt, kpad = a.shape
    sums = np.empty((n, 5), np.float64)
    sim = np.empty(n, np.float32)
    status = np.empty(n, np.int32)
    _check_op(ops_lib().vt_op_appearance_score(device, _vp(a), _vp(p), n, nt, kpad, int(cols), _vp(sums), _vp(sim), _vp(status)))
    return dict(sums=sums, similarity=sim, status=status)


# the 224-byte record of the reacquire proposals (csrc/k_proposals.hpp: PropRec)
PROPOSAL_DTYPE = np.dtype([("sim", "<f4"), ("box", "<f4", 4), ("pos", "<i4")])
PROPOSALS_REC_DTYPE = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("n", "<i4"), ("c", "<f4"), ("Wg", "<i4"), ("Hg", "<i4"),
                                ("reserved", "<i4", 2), ("p", PROPOSAL_DTYPE, 8)])


def op_proposals(frames, states, results, tpl, T, patch, norm, mode=2, period=1, max_n=4, min_sim_pm=500, max_cells=16384,
                 slot_stream=None, winner=None, tpl_bufs=1, device_frames=True, evaluated=None, device=0):
    """vt_op_proposals: the four launches of k_proposals.hip on given operands, nothing else. frames: CFrame per slot with
    DEVICE planes; states: snapshot.STATE records by stream; results [n] RESULT_DTYPE by slot; tpl [n_streams, tpl_bufs,
    nt, kpad] uint16 bf16 bit patterns; norm: (a0, a1, a2, b0, b1, b2). -> dict(pattern [n, 256] int16, thumb [n, max_cells]
    int16, map [n, max_cells] float32, records [n_streams] PROPOSALS_REC_DTYPE, evaluated [n_streams] int32); what no
    launch stored is 0xff bytes"""
    n, arr = _frames(frames)
    st = _start(states, STATE)
    ns = len(st)
    res = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
    assert res.shape == (n,)
    t = np.ascontiguousarray(tpl, np.uint16)
    kpad = t.shape[-1]
    assert t.size == ns * tpl_bufs * (T // patch) ** 2 * kpad
    smap, win = _maps(n, slot_stream, winner)
    nrm = np.ascontiguousarray(norm, np.float32).reshape(6)
    pol = np.array([mode, period, max_n, min_sim_pm, 0, max_cells, 0, 0], np.int32)
    pattern = np.empty((n, 256), np.int16)
    thumb = np.empty((n, max_cells), np.int16)
    smap_out = np.empty((n, max_cells), np.float32)
    recs = np.empty(ns, PROPOSALS_REC_DTYPE)
    ev = _start(evaluated, np.int32, (ns,))
    _check_op(ops_lib().vt_op_proposals(
        device, arr, _vp(st), ns, _vp(res), _opt(smap, _i32), _opt(win, _i32), n, _vp(t), tpl_bufs, T, patch, kpad, _vp(nrm),
        _vp(pol), 1 if device_frames else 0, _vp(pattern), _vp(thumb), _vp(smap_out), _vp(recs), _vp(ev)))
    return dict(pattern=pattern, thumb=thumb, map=smap_out, records=recs, evaluated=ev)


# the 104-byte record of the camera motion (csrc/k_camera_motion.hpp: CamRec) and the entries of a stream's SAD table
CAMERA_REC_DTYPE = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("c", "<i4"), ("Wg", "<i4"), ("Hg", "<i4"), ("R", "<i4"),
                             ("dx", "<i4"), ("dy", "<i4"), ("shift", "<f4", 2), ("applied", "<i4"), ("n", "<i4"), ("S_best", "<i8"),
                             ("S0", "<i8"), ("S2", "<i8"), ("evaluated", "<i4"), ("moved", "<i4"), ("has_prev", "<i4"), ("cur", "<i4"),
                             ("pW", "<i4"), ("pH", "<i4"), ("pc", "<i4"), ("reserved", "<i4")])
CAMERA_TABLE = 33 * 33
assert CAMERA_REC_DTYPE.itemsize == 104


def op_camera_motion(frames, states, mode=2, cell=0, rng=8, conf_pm=800, max_cells=65536, slot_stream=None, thumbs=None, records=None,
                     device_frames=True, host_states=None, host_records=None, device=0):
    """vt_op_camera_motion: the four launches of k_camera_motion.hip on given operands, nothing else. frames: CFrame per slot
    with DEVICE planes; states: snapshot.STATE records by stream; slot_stream [n]: slot -> stream (None: the identity);
    thumbs [n_streams, 2, max_cells] uint16 and records [n_streams] CAMERA_REC_DTYPE to start from (None: zeros - no
    previous thumbnail); host_states / host_records: what the pinned mirrors hold before (None: that mirror is null).
    -> dict(states, thumbs, records, sad [n_streams, 1089] int64 - what no launch stored is 0xff bytes -, host_states,
    host_records) as they came back; feed thumbs and records to the next call to go on"""
    n, arr = _frames(frames)
    st = _start(states, STATE)
    ns = len(st)
    smap, _ = _maps(n, slot_stream)
    th = _start(thumbs, np.uint16, (ns, 2, max_cells))
    rec = _start(records, CAMERA_REC_DTYPE, (ns,))
    hst, hrec = _mirror(host_states, STATE, ns), _mirror(host_records, CAMERA_REC_DTYPE, ns)
    pol = np.array([mode, cell, rng, conf_pm, max_cells, 0, 0, 0], np.int32)
    sad = np.empty((ns, CAMERA_TABLE), np.int64)
    _check_op(ops_lib().vt_op_camera_motion(
        device, arr, _vp(st), ns, _opt(smap, _i32), n, _i32(pol), 1 if device_frames else 0, _vp(th), _vp(rec), _vp(sad),
        _opt(hst, _vp), _opt(hrec, _vp)))
    return dict(states=st, thumbs=th, records=rec, sad=sad, host_states=hst, host_records=hrec)


# the frame health's arrays (csrc/k_health.hpp: HealthRec 104 bytes and HealthCount 16 bytes by stream, HealthHead 32 bytes by slot)
HEALTH_REC_DTYPE = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("flags", "<i4"), ("c", "<i4"), ("Wg", "<i4"), ("Hg", "<i4"),
                             ("still", "<i4"), ("reserved0", "<i4"), ("S1", "<i8"), ("S2", "<i8"), ("G", "<i8"), ("D", "<i8"),
                             ("HD", "<i8"), ("G_ref", "<i8"), ("has_prev", "<i4"), ("cur", "<i4"), ("pW", "<i4"), ("pH", "<i4"),
                             ("pc", "<i4"), ("reserved1", "<i4")])
HEALTH_COUNT_DTYPE = np.dtype([("evaluated", "<i4"), ("flagged", "<i4"), ("gated", "<i4"), ("reserved", "<i4")])
HEALTH_HEAD_DTYPE = np.dtype([("status", "<i4"), ("stream", "<i4"), ("frames_done", "<i4"), ("c", "<i4"), ("Wg", "<i4"), ("Hg", "<i4"),
                              ("cur", "<i4"), ("reserved", "<i4")])
_HEALTH_BINS = 32      # a record's flags: 1 FROZEN, 2 FLAT, 4 CUT
assert HEALTH_REC_DTYPE.itemsize == 104 and HEALTH_HEAD_DTYPE.itemsize == 32


def op_frame_health(frames, states, on=1, period=1, cell=0, still_run=3, flat_q=32, cut_pm=500, gate=0, max_cells=65536,
                    slot_stream=None, thumbs=None, hist=None, records=None, counts=None, device_frames=True, host_records=None,
                    device=0):
    """vt_op_frame_health: the four launches of k_health.hip on given operands, nothing else. frames: CFrame per slot with
    DEVICE planes; states: snapshot.STATE records by stream; slot_stream [n]: slot -> stream (None: the identity). The
    store to start from: thumbs [n_streams, 2, max_cells] uint16 and hist [n_streams, 2, 32] int32 (None: 0xff bytes - what
    no launch stores shows), records [n_streams] HEALTH_REC_DTYPE and counts [n_streams] HEALTH_COUNT_DTYPE (None: zeros - no
    previous thumbnail); host_records: what the pinned mirror holds before (None: the mirror is null). -> dict(states,
    thumbs, hist, records, counts, accs [n_streams, 4] int64 = S1, S2, G, D - 0xff bytes where no launch stored -, heads [n]
    HEALTH_HEAD_DTYPE, host_records) as they came back; feed thumbs, hist, records and counts to the next call to go on"""
    n, arr = _frames(frames)
    st = _start(states, STATE)
    ns = len(st)
    smap, _ = _maps(n, slot_stream)
    th, hi = _start(thumbs, np.uint16, (ns, 2, max_cells), 0xff), _start(hist, np.int32, (ns, 2, _HEALTH_BINS), 0xff)
    rec, cnt = _start(records, HEALTH_REC_DTYPE, (ns,)), _start(counts, HEALTH_COUNT_DTYPE, (ns,))
    hrec = _mirror(host_records, HEALTH_REC_DTYPE, ns)
    pol = np.array([on, period, cell, still_run, flat_q, cut_pm, gate, max_cells], np.int32)
    accs = np.empty((ns, 4), np.int64)
    heads = np.empty(n, HEALTH_HEAD_DTYPE)
    _check_op(ops_lib().vt_op_frame_health(
        device, arr, _vp(st), ns, _opt(smap, _i32), n, _i32(pol), 1 if device_frames else 0, _vp(th), _vp(accs), _vp(hi),
        _vp(heads), _vp(rec), _vp(cnt), _opt(hrec, _vp)))
    return dict(states=st, thumbs=th, hist=hi, records=rec, counts=cnt, accs=accs, heads=heads, host_records=hrec)


# the moving regions' arrays (csrc/k_movers.hpp: MoverRec 256 bytes and MoverCount 16 bytes by stream, MoverHead 32 bytes by slot)
MOVERS_BOX_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("area", "<i4"), ("label", "<i4")])
MOVERS_REC_DTYPE = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("c", "<i4"), ("Wg", "<i4"), ("Hg", "<i4"), ("n", "<i4"),
                             ("moving", "<i4"), ("kept", "<i4"), ("components", "<i4"), ("own_cells", "<i4"), ("own_kept", "<i4"),
                             ("still", "<i4"), ("has_bg", "<i4"), ("pW", "<i4"), ("pH", "<i4"), ("pc", "<i4"),
                             ("box", MOVERS_BOX_DTYPE, 8)])
MOVERS_COUNT_DTYPE = np.dtype([("evaluated", "<i4"), ("listed", "<i4"), ("reserved", "<i4", 2)])
MOVERS_HEAD_DTYPE = np.dtype([("status", "<i4"), ("stream", "<i4"), ("frames_done", "<i4"), ("c", "<i4"), ("Wg", "<i4"), ("Hg", "<i4"),
                              ("reserved", "<i4", 2)])
assert MOVERS_REC_DTYPE.itemsize == 256 and MOVERS_HEAD_DTYPE.itemsize == 32 and MOVERS_COUNT_DTYPE.itemsize == 16


def movers_shape(learn, min_nb, max_n):
    """the policy word that carries "movers_learn", "movers_min_nb" and "movers_max" (csrc/vt_feature_keys.hpp: MV_SHAPE)"""
    return int(learn) | int(min_nb) << 4 | int(max_n) << 8


def op_movers(frames, states, on=1, period=1, cell=0, thr=96, min_area=4, global_pm=400, learn=4, min_nb=3, max_n=4, max_cells=65536,
              slot_stream=None, bg=None, mask=None, records=None, counts=None, device_frames=True, host_records=None, shape=None,
              device=0):
    """vt_op_movers: the launches of k_movers.hip on given operands, nothing else. frames: CFrame per slot with DEVICE planes;
    states: snapshot.STATE records by stream; slot_stream [n]: slot -> stream (None: the identity). The store to start from: bg
    [n_streams, max_cells] uint16 and mask [n_streams, max_cells] uint8 (None: 0xff bytes - what no launch stores shows),
    records [n_streams] MOVERS_REC_DTYPE and counts [n_streams] MOVERS_COUNT_DTYPE (None: zeros - no background);
    host_records: what the pinned mirror holds before (None: the mirror is null); shape: the raw policy word instead of learn,
    min_nb and max_n. -> dict(states, bg, thumbs, mask, labels [n_streams, max_cells] int32, exts [n_streams, 4, max_cells]
    int32 = i0, i1, j1, area, accs [n_streams, 4] int32 = moving, kept - 0xff bytes where no launch stored -, heads [n]
    MOVERS_HEAD_DTYPE, records, counts, host_records) as they came back; feed bg, mask, records and counts to the next call"""
    n, arr = _frames(frames)
    st = _start(states, STATE)
    ns = len(st)
    smap, _ = _maps(n, slot_stream)
    b, m = _start(bg, np.uint16, (ns, max_cells), 0xff), _start(mask, np.uint8, (ns, max_cells), 0xff)
    rec, cnt = _start(records, MOVERS_REC_DTYPE, (ns,)), _start(counts, MOVERS_COUNT_DTYPE, (ns,))
    hrec = _mirror(host_records, MOVERS_REC_DTYPE, ns)
    pol = np.array([on, period, cell, thr, min_area, global_pm, movers_shape(learn, min_nb, max_n) if shape is None else shape,
                    max_cells], np.int32)
    thumbs = np.empty((ns, max_cells), np.uint16)
    labels, exts = np.empty((ns, max_cells), np.int32), np.empty((ns, 4, max_cells), np.int32)
    accs = np.empty((ns, 4), np.int32)
    heads = np.empty(n, MOVERS_HEAD_DTYPE)
    _check_op(ops_lib().vt_op_movers(
        device, arr, _vp(st), ns, _opt(smap, _i32), n, _i32(pol), 1 if device_frames else 0, _vp(b), _vp(thumbs), _vp(m), _vp(labels),
        _vp(exts), _vp(accs), _vp(heads), _vp(rec), _vp(cnt), _opt(hrec, _vp)))
    return dict(states=st, bg=b, thumbs=thumbs, mask=m, labels=labels, exts=exts, accs=accs, heads=heads, records=rec, counts=cnt,
                host_records=hrec)


# the peak arbitration's records (csrc/k_arbitrate.hpp: ArbRec 176 bytes and ArbCount 8 bytes, both by stream)
ARBITRATE_PEAK_DTYPE = np.dtype([("cell", "<i4"), ("status", "<i4"), ("score", "<f4"), ("resp", "<f4"), ("similarity", "<f4"),
                                 ("reserved", "<i4"), ("box", "<f4", 4)])
ARBITRATE_REC_DTYPE = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("n", "<i4"), ("chosen", "<i4"),
                                ("peak", ARBITRATE_PEAK_DTYPE, 4)])
ARBITRATE_COUNT_DTYPE = np.dtype([("evaluated", "<i4"), ("switched", "<i4")])
assert ARBITRATE_REC_DTYPE.itemsize == 176


def op_arbitrate(head_out, hann, frames, states, results, anchor, grid, T, S, patch, norm, success_threshold, on=1, max_peaks=3,
                 radius=2, min_resp_pm=50, low_pm=300, high_pm=500, slot_stream=None, winner=None, counts=None, tier=0,
                 host_results=None, host_states=None, host_records=None, device=0):
    """vt_op_arbitrate: the four launches of k_arbitrate.hip on given operands, nothing else. head_out [n * grid^2][8] float32
    logits by slot, hann [grid^2], frames: CFrame per slot with DEVICE planes; states: snapshot.STATE records by stream;
    results [n] RESULT_DTYPE by slot; anchor [n_streams, nt, kpad] uint16 bf16 bit patterns; norm: (a0, a1, a2, b0, b1, b2);
    slot_stream [n]: slot -> stream (None: the identity); winner [n]: not None marks a candidate pass; counts [n_streams]
    ARBITRATE_COUNT_DTYPE to start from (None: zeros); host_*: what the pinned mirrors hold before (None: that mirror is null).
    -> dict(states, results, records [n_streams] ARBITRATE_REC_DTYPE, probe [n_streams, 4, nt, kpad] uint16 - both 0xff bytes
    where no launch stored -, counts, host_results, host_states, host_records) as they came back"""
    n, arr = _frames(frames)
    ns = grid * grid
    ho = np.ascontiguousarray(head_out, np.float32)
    assert ho.shape == (n * ns, 8)
    hn = np.ascontiguousarray(hann, np.float32).reshape(-1)
    assert hn.shape == (ns,)
    st = _start(states, STATE)
    nst = len(st)
    res = _start(results, RESULT_DTYPE, (n,))
    an = np.ascontiguousarray(anchor, np.uint16)
    nt = (T // patch) ** 2
    assert an.ndim == 3 and an.shape[:2] == (nst, nt)
    kpad = an.shape[2]
    smap, win = _maps(n, slot_stream, winner)
    nrm = np.ascontiguousarray(norm, np.float32).reshape(6)
    pol = np.array([on, max_peaks, radius, min_resp_pm, low_pm, high_pm, 0, 0], np.int32)
    rec = np.empty(nst, ARBITRATE_REC_DTYPE)
    cnt = _start(counts, ARBITRATE_COUNT_DTYPE, (nst,))
    probe = np.empty((nst, 4, nt, kpad), np.uint16)
    hres, hst = _mirror(host_results, RESULT_DTYPE, n), _mirror(host_states, STATE, nst)
    hrec = _mirror(host_records, ARBITRATE_REC_DTYPE, nst)
    _check_op(ops_lib().vt_op_arbitrate(
        device, _f32(ho), _f32(hn), arr, _vp(st), nst, _vp(res), _opt(smap, _i32), _opt(win, _i32), n, grid, _vp(an), T, S, patch,
        kpad, _f32(nrm), c_float(success_threshold), _i32(pol), tier, _vp(rec), _vp(cnt), _vp(probe), _opt(hres, _vp),
        _opt(hst, _vp), _opt(hrec, _vp)))
    return dict(states=st, results=res, records=rec, probe=probe, counts=cnt, host_results=hres, host_states=hst, host_records=hrec)


# the stream conflicts' records (csrc/k_conflicts.hpp: ConflictRec 48 bytes and ConflictCount 16 bytes, both by stream)
CONFLICT_REC_DTYPE = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("n_over", "<i4"), ("reserved", "<i4"),
                               ("partner", "<i4", 4), ("iou", "<f4", 4)])
CONFLICT_COUNT_DTYPE = np.dtype([("evaluated", "<i4"), ("conflicting", "<i4"), ("gated", "<i4"), ("reserved", "<i4")])
assert CONFLICT_REC_DTYPE.itemsize == 48


def op_stream_conflicts(states, results, scenes, on=1, iou_pm=300, gate=0, slot_stream=None, winner=None, records=None, counts=None,
                        host_records=None, fill=0xA5, device=0):
    """vt_op_stream_conflicts: the one launch of k_conflicts.hip on given operands, nothing else. states: snapshot.STATE
    records by stream; results [n] RESULT_DTYPE by slot; scenes [n_streams] int32; slot_stream [n]: slot -> stream (None: the
    identity); winner [n]: the winning slot of slot i's stream (None: the first slot naming a stream works for it). records
    [n_streams] CONFLICT_REC_DTYPE and counts [n_streams] CONFLICT_COUNT_DTYPE to start from (None: every byte `fill`);
    host_records: what the pinned mirror holds before (None: the mirror is null). -> dict(records, counts, host_records) as
    they came back"""
    st = _start(states, STATE)
    ns = len(st)
    res = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
    n = len(res)
    sc = np.ascontiguousarray(scenes, np.int32).reshape(-1)
    smap, win = _maps(n, slot_stream, winner)
    assert sc.shape == (ns,)
    rec, cnt = _start(records, CONFLICT_REC_DTYPE, (ns,), fill), _start(counts, CONFLICT_COUNT_DTYPE, (ns,), fill)
    hrec = _mirror(host_records, CONFLICT_REC_DTYPE, ns)
    pol = np.array([on, iou_pm, gate, 0, 0, 0, 0, 0], np.int32)
    _check_op(ops_lib().vt_op_stream_conflicts(
        device, _vp(st), ns, _vp(res), _opt(smap, _i32), _opt(win, _i32), n, _i32(sc), _i32(pol), _vp(rec), _vp(cnt),
        _opt(hrec, _vp)))
    return dict(records=rec, counts=cnt, host_records=hrec)


# the 32-byte records of the result overlay (csrc/k_result_overlay.hpp)
OVERLAY_POLICY_DTYPE = np.dtype([("flags", "<i4"), ("thickness", "<i4"), ("size", "<i4"), ("scale", "<i4"), ("luma", "<i4"),
                                 ("rgb", "<i4"), ("min_score_pct", "<i4"), ("reserved", "<i4")])
OVERLAY_STATS_DTYPE = np.dtype([("drawn", "<i4"), ("n_drawn", "<i4"), ("n_gated", "<i4"), ("n_unsupported", "<i4"),
                                ("last_n", "<i4"), ("reserved", "<i4", 3)])


def op_result_overlay(frames, results, flags=7, thickness=3, size=15, scale=2, luma=255, rgb=0x00FF00, min_score_pct=25,
                      slot_stream=None, winner=None, stats=None, n_streams=None, device_frames=True, device=0):
    """vt_op_result_overlay: the result-overlay launch (k_result_overlay.hip) on given operands, nothing else. frames: CFrame
    per slot with DEVICE planes (they are drawn into), results [n] RESULT_DTYPE by slot, slot_stream [n]: slot -> stream
    (None: the identity), winner [n]: a candidate pass's winner table (None: every slot may draw), stats: OVERLAY_STATS_DTYPE
    records by stream to start from (None: zeros), device_frames False: the launch of a host pass. -> the stats as they
    came back"""
    n, arr = _frames(frames)
    res = np.ascontiguousarray(results, RESULT_DTYPE).reshape(-1)
    assert res.shape == (n,)
    smap, win = _maps(n, slot_stream, winner)
    if n_streams is None:
        n_streams = n if stats is None else len(stats)
    st = _start(stats, OVERLAY_STATS_DTYPE, (n_streams,))
    pol = np.zeros(1, OVERLAY_POLICY_DTYPE)
    pol[0] = (flags, thickness, size, scale, luma, rgb, min_score_pct, 0)
    _check_op(ops_lib().vt_op_result_overlay(
        device, arr, _vp(res), _opt(smap, _i32), _opt(win, _i32), n, _vp(pol), _vp(st), n_streams, 1 if device_frames else 0))
    return st


__all__ = [n for n in dir() if n.startswith("op_") or n.endswith("_DTYPE")] + ["OPS_LIB_PATH", "OPS_EXPORTS", "ops_lib", "_check_op", "movers_shape"]
