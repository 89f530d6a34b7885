"""Helpers of the per-model residual quantum tests (test_lo_shift.py, test_gpu_lo_shift.py): the oracle
(oracle/vit_ref.py) reads its module globals LO_SHIFT / LO_Q at call time, so a test runs it at another shift inside
`oracle_lo_shift(s)`; `split_pair` restates the specification in NumPy float32."""
import contextlib

import numpy as np

from gstreamer_vit_tracker_amd import weights as W

# the yardstick test's outlier recipe (tests/test_gpu_fp32_yardstick.py part d) at the tiny model's width: channel ->
# offset carried by patch_b, and token rows 5::16 whose position embedding carries +20 on every channel
TINY_OUTLIER_CH = {5: 10.0, 37: -13.0, 60: 24.0, 90: -40.0, 120: 100.0}
OUTLIER_ROWS = slice(5, None, 16)
OUTLIER_ROW_OFFSET = 20.0


@contextlib.contextmanager
def oracle_lo_shift(s):
    """oracle.vit_ref at lo_shift s; s None: an UN-QUANTISED float32 residual (the low half is x - bf16(x) itself)"""
    from oracle import vit_ref
    saved = vit_ref.LO_SHIFT, vit_ref.LO_Q, vit_ref.split_residual
    try:
        if s is None:
            def exact(v):
                v = np.asarray(v, np.float32)
                hi = vit_ref.bf16r(v)
                return hi, (v - hi).astype(np.float32)
            vit_ref.split_residual = exact
        else:
            vit_ref.LO_SHIFT, vit_ref.LO_Q = int(s), np.float32(2.0 ** -int(s))
        yield vit_ref
    finally:
        vit_ref.LO_SHIFT, vit_ref.LO_Q, vit_ref.split_residual = saved


def split_pair(x, s):
    """value of the stored pair: bf16(x) + clamp(rint((x - bf16(x)) * 2^s), -127, 127) * 2^-s, all in float32"""
    x = np.asarray(x, np.float32)
    hi = W.bf16_bits_to_f32(W.f32_to_bf16_bits(x)).reshape(x.shape)
    lo8 = np.clip(np.rint((x - hi).astype(np.float32) * np.float32(2.0 ** s)), -127.0, 127.0).astype(np.float32)
    return (hi + lo8 * np.float32(2.0 ** -s)).astype(np.float32)


def pair_parts(x, s):
    """(bf16 bits, lo8 int8) of x's pair at shift s"""
    x = np.asarray(x, np.float32)
    bits = W.f32_to_bf16_bits(x).reshape(x.shape)
    hi = W.bf16_bits_to_f32(bits).reshape(x.shape)
    lo8 = np.clip(np.rint((x - hi).astype(np.float32) * np.float32(2.0 ** s)), -127.0, 127.0).astype(np.int8)
    return bits, lo8


def lo8_of(x, s):
    """the byte a representable stored value x carries: (x - bf16(x)) * 2^s, which must be an integer in [-127, 127]"""
    x = np.asarray(x, np.float32)
    hi = W.bf16_bits_to_f32(W.f32_to_bf16_bits(x)).reshape(x.shape)
    return ((x - hi).astype(np.float32) * np.float32(2.0 ** s)).astype(np.float32)


# the same recipe at D = 768: the yardstick test's own channels
VITB_OUTLIER_CH = {37: 10.0, 200: -13.0, 411: 24.0, 600: -40.0, 750: 100.0}


def tiny_outlier_blob(path, lo_shift=0):
    return outlier_blob(path, "tiny", TINY_OUTLIER_CH, lo_shift)


def outlier_blob(path, cfg_name, channels, lo_shift=0):
    cfg = W.get_config(cfg_name)
    t = W.generate_tensors(cfg)
    code, pb = t["patch_b"]
    pb = pb.copy()
    for c, off in channels.items():
        pb[0, c] += np.float32(off)
    t["patch_b"] = (code, pb)
    code, pos = t["pos"]
    pos = pos.copy()
    pos[OUTLIER_ROWS] += np.float32(OUTLIER_ROW_OFFSET)
    t["pos"] = (code, pos)
    with open(path, "wb") as f:
        f.write(W.pack_blob(cfg, t, lo_shift=lo_shift))
    return str(path)


def xrange_row(x, s):
    """the "xrange" columns of a stored tensor x at shift s, in NumPy"""
    ax = np.abs(np.asarray(x, np.float32))
    n_sat = int((np.abs(lo8_of(x, s)) == 127).sum())
    return [float(s), float(ax.max()), float(n_sat)] + [float((ax >= 2.0 ** k).sum()) for k in range(1, 10)]
