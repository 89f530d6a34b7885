"""Inputs, references and the GELU interval for the tile-edge and value-by-value tests of the GEMM epilogues
(csrc/k_gemm.hip, csrc/k_gemm256.hip), shared by test_epilogue_cases.py (CPU: the premises) and test_gpu_epilogue_edges.py.

TILE EDGES. Small-integer operands at N = K = 256: every product and sum is an exact integer below 2^24, so whatever order
a kernel accumulates in the result is that integer - a row that is never stored, stored twice from the wrong tile, or taken
from a clamped neighbour is a wrong number, not a rounding difference. One pool of rows serves every M: row m of the result
depends on row m of A alone, so the reference of the largest M is computed once and sliced.

VALUES. With zero A and zero W the accumulator is 0 and y = bias[n]: any float32 can be put through the bf16 epilogues, one
value per column. ReLU, k and v round y itself, q rounds float32(y * QK_SCALE); what they must return is the integer rounding
of the oracle (weights.f32_to_bf16_bits), bit for bit. GELU is compared through an interval:

    ref = y * 0.5 * erfc(-y / sqrt 2) in float64 (the erf form cancels in the tail),
    d   = d_poly + |y| Phi(-|y|) 2^-22 + |ref| 2^-23,
    got in [bf16(ref - d), bf16(ref + d)]       (rounding is monotone: exactly the answers a GELU within d can give)

d_poly is the largest |model - ref| of the float32 model of gelu_erf (ln_chain_util._gelu_poly: exact fma, exact exp2)
over the very inputs of the test, 2^-22 the allowance attention_util.py makes for the hardware's exp2 (relative, on the
term a * 2^P(a) it enters through), and the last term the float32 rounding of the final fma."""
import functools
import math

import numpy as np
from scipy.special import erfc

from attention_util import bf16_rne
from gstreamer_vit_tracker_amd.weights import bf16_bits_to_f32, f32_to_bf16_bits
from ln_chain_util import QK_SCALE, _gelu_poly

F = np.float32
SC = F(2.0 ** -12)                  # the X-epilogues' operands: integers * 2^-12, inside the 3-byte pair's exact range
EXP2_REL = 2.0 ** -22               # the hardware exp2, as attention_util.py allows it
GELU_POLY_CLAIM = 6.4e-7            # the figure in csrc/k_gemm_util.hpp

# ---- tile edges --------------------------------------------------------------------------------------------------

TILE_ROWS = {0: 64, 1: 128, 2: 64, 3: 128, 4: 64, 5: 64, 6: 128, 7: 64, 8: 128, 18: 256, 19: 256}      # BM of each configuration
TILE_COLS = {0: 64, 1: 128, 2: 64, 3: 128, 4: 64, 5: 64, 6: 128, 7: 64, 8: 64, 18: 256, 19: 256}       # BN
EDGE_CONFIGS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 18)
EDGE_M = (1, 2, 3, 5, 31, 33, 63, 64, 65, 127, 128, 129, 191, 193, 255, 256, 257, 383, 385)
EDGE_N = EDGE_K = EDGE_D = 256
QKV_B = (1, 3)
QKV_TOKENS = (4, 8, 60, 64, 68, 124, 128, 132, 252, 256, 260)


def qkv_config_fits(cfg, D):
    """launch_cfg (k_gemm.hip): `EPI == EPI_QKV && a.D % BN != 0` is refused - a column tile is q, k or v; gemm256_fits
    (k_gemm256.hip): `a.D % 256 != 0` is refused"""
    return D % TILE_COLS[cfg] == 0


@functools.lru_cache(maxsize=None)
def edge_operands(rows=max(max(EDGE_M), max(QKV_B) * max(QKV_TOKENS)), N=EDGE_N, K=EDGE_K, seed=4100):
    """a [rows, K], w [N, K] in -4 .. 4, bias [N] in -8 .. 8, c0 [rows, N] in -100 .. 99, row terms rs [rows, 2] in
    1 .. 3 / -2 .. 2, column sums cs [N] in -5 .. 5 (float32 integers, read-only), z = a w^T + bias and
    zf = rs0 * (a w^T) + (rs1 * cs + bias) in float64"""
    rng = np.random.default_rng(seed + rows + N + K)
    a = rng.integers(-4, 5, size=(rows, K)).astype(F)
    w = rng.integers(-4, 5, size=(N, K)).astype(F)
    bias = rng.integers(-8, 9, size=N).astype(F)
    c0 = rng.integers(-100, 100, size=(rows, N)).astype(F)
    rs = np.stack([rng.integers(1, 4, size=rows), rng.integers(-2, 3, size=rows)], axis=1).astype(F)
    cs = rng.integers(-5, 6, size=N).astype(F)
    acc = a.astype(np.float64) @ w.astype(np.float64).T
    z = acc + bias
    zf = rs[:, :1].astype(np.float64) * acc + (rs[:, 1:].astype(np.float64) * cs[None, :] + bias[None, :])
    out = dict(a=a, w=w, bias=bias, c0=c0, rs=rs, cs=cs, z=z, zf=zf)
    for v in out.values():
        v.setflags(write=False)
    return out


def bf16_round(x):
    """float32 -> the oracle's integer rounding to bf16, widened again"""
    return bf16_bits_to_f32(f32_to_bf16_bits(np.asarray(x, F)))


def split_pair_value(x, lo_shift=12):
    """the value hi + lo8 * 2^-s of the 3-byte pair of x (numerical specification v3)"""
    x = np.asarray(x, F)
    hi = bf16_round(x)
    lo = np.clip(np.rint((x - hi).astype(F) * F(2.0 ** lo_shift)), -127, 127).astype(F)
    return (hi + lo * F(2.0 ** -lo_shift)).astype(F)


def row_terms64(x, eps=1e-6):
    """NumPy float64 (rstd, -mean * rstd) of float32 rows"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1)
    rstd = 1.0 / np.sqrt(x.var(axis=1) + eps)
    return np.stack([rstd, -mean * rstd], axis=1)


def vt_positions(tokens, perm):
    """position of token t inside its stream's V^T row: t, or t with bits 2 and 3 exchanged (the order mode 3 reads)"""
    t = np.arange(tokens)
    return ((t & ~12) | ((t & 4) << 1) | ((t & 8) >> 1)) if perm else t


def qkv_expected(z, B, tokens, D, perm):
    """z [B * tokens, 3D] (float64 integers or float32) -> qk [M, 2D] and V^T [B * D / 64, 64, npad] with zeros at every
    position that belongs to no token"""
    z32 = np.asarray(z, F)
    qk = np.concatenate([bf16_round((z32[:, :D] * QK_SCALE).astype(F)), bf16_round(z32[:, D:2 * D])], axis=1)
    npad = (tokens + 63) // 64 * 64
    v = bf16_round(z32[:, 2 * D:]).reshape(B, tokens, D // 64, 64).transpose(0, 2, 3, 1).reshape(-1, 64, tokens)
    vt = np.zeros((B * (D // 64), 64, npad), F)
    vt[:, :, vt_positions(tokens, perm)] = v
    return qk, vt


# ---- values ------------------------------------------------------------------------------------------------------

TINY = F(2.0 ** -126)


def _from_bits32(u):
    return np.ascontiguousarray(u, np.uint32).view(F)


@functools.lru_cache(maxsize=None)
def bf16_patterns():
    """every finite bf16 bit pattern widened to float32, normal or zero: 2 * 254 * 128 + 2 values"""
    f = bf16_bits_to_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16))
    f = f[np.isfinite(f) & ((np.abs(f) >= TINY) | (f == 0))]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def tie_set():
    """float32 values just below, on and just above the middle between two bf16 values (low half 0x7FFF, 0x8000, 0x8001),
    over even and odd upper halves (mantissa bits 0, 1, 0x7E, 0x7F), both signs, every normal exponent; exponent 254 with
    mantissa 0x7F is the band that rounds to infinity"""
    e, m, s, lo = np.meshgrid(np.arange(1, 255, dtype=np.uint32), np.array([0, 1, 0x7E, 0x7F], np.uint32),
                              np.array([0, 1], np.uint32), np.array([0x7FFF, 0x8000, 0x8001], np.uint32), indexing="ij")
    f = _from_bits32(((s << 31) | (e << 23) | (m << 16) | lo).ravel())
    assert np.isfinite(f).all()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def random_sets():
    """2 * 10^5 values uniform in [-12, 12] and 2 * 10^5 from N(0, 1.5), float32"""
    rng = np.random.default_rng(6400)
    u = rng.uniform(-12.0, 12.0, 200000).astype(F)
    n = rng.normal(0.0, 1.5, 200000).astype(F)
    for a in (u, n):
        assert (np.abs(a[a != 0]) >= TINY).all()
        a.setflags(write=False)
    return u, n


@functools.lru_cache(maxsize=None)
def subnormal_inputs():
    """float32 subnormals: every bf16 subnormal pattern of both signs, their ties (low half 0x7FFF / 0x8000 / 0x8001 on
    upper halves 0, 1, 0x3F, 0x40, 0x7E, 0x7F), the smallest and the largest subnormal and 500 random ones"""
    rng = np.random.default_rng(6401)
    up = np.arange(1, 128, dtype=np.uint32) << 16
    t_up = np.array([0, 1, 0x3F, 0x40, 0x7E, 0x7F], np.uint32)[:, None] << 16
    ties = (t_up | np.array([0x7FFF, 0x8000, 0x8001], np.uint32)[None, :]).ravel()
    pos = np.concatenate([up, ties, np.array([1, 0x007FFFFF], np.uint32), rng.integers(1, 0x00800000, 500).astype(np.uint32)])
    f = _from_bits32(np.concatenate([pos, pos | np.uint32(0x80000000)]))
    assert ((f != 0) & (np.abs(f) < TINY)).all()
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def rounding_inputs():
    """the normal inputs of the exact-rounding tests: bf16 patterns, ties, uniform, normal - in that order"""
    u, n = random_sets()
    f = np.concatenate([bf16_patterns(), tie_set(), u, n])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def gelu_inputs():
    """the inputs d_poly is taken over: bf16 patterns, uniform, normal - in that order"""
    u, n = random_sets()
    f = np.concatenate([bf16_patterns(), u, n])
    f.setflags(write=False)
    return f


def chunks(values, n):
    """values in pieces of exactly n (the last one padded with zeros) -> (offset, count, piece)"""
    for o in range(0, len(values), n):
        piece = np.zeros(n, F)
        cnt = min(n, len(values) - o)
        piece[:cnt] = values[o:o + cnt]
        yield o, cnt, piece


def q_product(y):
    """float32(y * QK_SCALE): what the q columns round"""
    with np.errstate(under="ignore"):
        return (np.asarray(y, F) * QK_SCALE).astype(F)


# ---- GELU --------------------------------------------------------------------------------------------------------

def gelu_ref(y):
    y = np.asarray(y, np.float64)
    return y * 0.5 * erfc(-y / math.sqrt(2.0))


def gelu_model(y):
    """the float32 model of gelu_erf before its rounding to bf16"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return _gelu_poly(np.asarray(y, F))


@functools.lru_cache(maxsize=None)
def gelu_d_poly():
    """largest |model - ref| over gelu_inputs() and the input it is taken at"""
    y = gelu_inputs()
    err = np.abs(gelu_model(y).astype(np.float64) - gelu_ref(y))
    i = int(err.argmax())
    return float(err[i]), float(y[i])


def _bf16_rne_all(x):
    """attention_util.bf16_rne with the subnormal range (a fixed spacing of 2^-133) and overflow (float32 infinity)"""
    x = np.asarray(x, np.float64)
    r = np.where(np.abs(x) < float(TINY), np.rint(x * 2.0 ** 133) * 2.0 ** -133, bf16_rne(x))
    with np.errstate(over="ignore"):
        return r.astype(F)


def gelu_interval(y, d_poly=None):
    """(lo, hi, ref, d): the bf16 values (float32) a GELU within d of the float64 reference can round to"""
    if d_poly is None:
        d_poly = gelu_d_poly()[0]
    y64 = np.asarray(y, np.float64)
    ref = gelu_ref(y64)
    a = np.abs(y64)
    d = d_poly + a * 0.5 * erfc(a / math.sqrt(2.0)) * EXP2_REL + np.abs(ref) * 2.0 ** -23
    return _bf16_rne_all(ref - d), _bf16_rne_all(ref + d), ref, d


def inside(got, lo, hi):
    got = np.asarray(got, F)
    return (got >= lo) & (got <= hi)        # NaN is outside


@functools.lru_cache(maxsize=None)
def _bf16_grid():
    """every finite bf16 value in ascending order (one zero) and the middles between neighbours, float64"""
    f = bf16_bits_to_f32(np.arange(65536, dtype=np.uint32).astype(np.uint16))
    v = np.unique(f[np.isfinite(f)].astype(np.float64))
    return v, (v[1:] + v[:-1]) / 2


def least_error(got, ref):
    """smallest |v - ref| over the float values v that round to the bf16 value got: the least error the kernel's float32
    GELU must have had to return it (infinite for a non-finite got). Divided by d it is <= 1 inside the interval."""
    v, mid = _bf16_grid()
    g = np.asarray(got, np.float64)
    ok = np.isfinite(g)
    i = np.clip(np.searchsorted(v, np.where(ok, g, 0.0)), 0, len(v) - 1)
    lo = np.where(i > 0, mid[np.maximum(i - 1, 0)], -np.inf)
    hi = np.where(i < len(v) - 1, mid[np.minimum(i, len(mid) - 1)], np.inf)
    e = np.maximum(0.0, np.maximum(lo - ref, ref - hi))
    return np.where(ok, e, np.inf)


# the mutants a value-by-value test must throw out (CPU only)

def gelu_tanh(y):
    y = np.asarray(y, np.float64)
    return (0.5 * y * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (y + 0.044715 * y ** 3)))).astype(F)


def gelu_sigmoid(y):
    y = np.asarray(y, np.float64)
    with np.errstate(over="ignore"):
        return (y / (1.0 + np.exp(-1.702 * y))).astype(F)


def bf16_truncate(x):
    return bf16_bits_to_f32((np.ascontiguousarray(x, F).view(np.uint32) >> np.uint32(16)).astype(np.uint16))


def bf16_half_up(x):
    u = np.ascontiguousarray(x, F).view(np.uint32)
    return bf16_bits_to_f32(((u + np.uint32(0x8000)) >> np.uint32(16)).astype(np.uint16))
