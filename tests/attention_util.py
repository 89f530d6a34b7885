"""Inputs, float64 reference and a derived per-element error bound for the attention kernels (csrc/k_attn.hip: modes 0-3
and the query-subset kernel), shared by test_attention_cases.py (CPU, premises only) and test_gpu_attention_edges.py.

Layout as the operator hooks take it: q, k, v are [B * N, H * 64], row b * N + t is token t of stream b, columns
h * 64 .. h * 64 + 63 belong to head h; q is already in log2 units (the QKV epilogue folds log2(e) / 8 into it), so the
weights are w = 2^(q k^T) / row sum."""
import functools
import math
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

from gstreamer_vit_tracker_amd.weights import bf16_bits_to_f32, f32_to_bf16_bits

U = 2.0 ** -8           # largest relative error of rounding to bf16 (8 significand bits, round to nearest even)
F32 = 2.0 ** -24        # the same for float32


def bf16_rne(x):
    """float64 -> the nearest bf16 value (ties to even), as float64, in one rounding (no float32 step in between)"""
    m, e = np.frexp(np.asarray(x, np.float64))          # |m| in [0.5, 1): m * 2^8 has the 8 significand bits in front
    return np.ldexp(np.rint(m * 256.0), e - 8)


def _heads(B, N, H):
    for b in range(B):
        for h in range(H):
            yield b, h, slice(b * N, (b + 1) * N), slice(h * 64, (h + 1) * 64)


# ---- A. the exact selector ---------------------------------------------------------------------------------------

SEL_MATCH = 56.0        # score of a query with its own key (4 * 7 in each of two dimensions), log2 units


def _coprime(N, idx):
    c = [m for m in range(3, 200) if math.gcd(m, N) == 1]
    return c[(7 * idx + 5) % len(c)]


# (B, N, H) of the exact-selector launches. tokens & 63 = 0 (320), 4 (68), 16 (16, 80, 720), 20 (980), 32 (96), 36 (36, 100),
# 48 (1008); 33 and 97 for modes 0-2 only (mode 3 takes multiples of 4). Workgroups of mode 3 (ceil(ceil(N / 32) / 4) * H * B):
# 1, 3, 2, 3, 6, 9, 9, 18, 16, 8. B = 3 with N = 36, 100, 97: streams 1 and 2 start off every tile boundary.
SELECTOR_SHAPES = [(1, 16, 1), (3, 36, 1), (1, 68, 2), (1, 80, 3), (3, 96, 2), (3, 100, 3), (3, 320, 1), (1, 720, 3),
                   (1, 980, 2), (1, 1008, 1)]
SELECTOR_SHAPES_ANY_N = [(1, 33, 1), (3, 97, 2)]


@functools.lru_cache(maxsize=None)
def selector_case(B, N, H):
    """Key i of every (stream, head) is 7 in dimensions i % 32 and 32 + i // 32 (N <= 1024), query i is 4 in the two
    dimensions of key sel[i]: 56 for the match, 28 for the <= 62 keys that share one dimension, 0 otherwise - inside the
    +-60 window of mode 3's unchecked first pass. sel = (i * m + c) % N with gcd(m, N) = 1 is a permutation, another one
    per (stream, head): every key - the last real one, the first of each tile, each position of a 16-key group - is some
    query's answer. V is odd integers in [-15, 15] (exact in bf16, never 0), drawn per (stream, head) so that no two keys
    share a row. Returns q, k, v (float32, read-only), their bf16 bits and want = V[sel] (float32, [B * N, H * 64])."""
    assert 1 < N <= 1024
    i = np.arange(N)
    q = np.zeros((B * N, H * 64), np.float32)
    k = np.zeros_like(q)
    v = np.zeros_like(q)
    want = np.zeros_like(q)
    sel = np.zeros((B, H, N), np.int64)
    for b, h, rows, cols in _heads(B, N, H):
        idx = b * H + h
        s = (i * _coprime(N, idx) + 5 + 11 * idx) % N
        assert np.array_equal(np.sort(s), i)
        r0, c0 = b * N, h * 64
        k[r0 + i, c0 + i % 32] = 7.0
        k[r0 + i, c0 + 32 + i // 32] = 7.0
        q[r0 + i, c0 + s % 32] = 4.0
        q[r0 + i, c0 + 32 + s // 32] = 4.0
        vv = np.random.default_rng(1000 * N + idx).integers(0, 16, (N, 64)) * 2 - 15
        v[rows, cols] = vv
        want[rows, cols] = vv[s]
        sel[b, h] = s
    c = SimpleNamespace(B=B, N=N, H=H, q=q, k=k, v=v, want=want, sel=sel,
                        qb=f32_to_bf16_bits(q), kb=f32_to_bf16_bits(k), vb=f32_to_bf16_bits(v))
    for a in (q, k, v, want, sel, c.qb, c.kb, c.vb):
        a.setflags(write=False)
    return c


def query_rows(a, B, N, q0, nq):
    """rows q0 .. q0 + nq - 1 of every stream of a [B * N, D] array, compact [B * nq, D]: the subset kernel's output layout"""
    return a.reshape(B, N, -1)[:, q0:q0 + nq].reshape(B * nq, -1)


MODEL_TEMPLATE_TOKENS = {80: 16, 320: 64, 720: 144, 980: 196}      # tiny, cfg2, cfg3, cfg4: template tokens of N


def subset_ranges(N):
    """(q0, nq) of the query-subset kernel for N tokens: everything, the search rows of a model shape, single rows at
    both ends, a range that starts and ends off every block boundary, the last 40"""
    r = [(0, N), (1, 1), (17, 33), (N - 1, 1), (N - 40, 40)]
    if N in MODEL_TEMPLATE_TOKENS:
        r.insert(1, (MODEL_TEMPLATE_TOKENS[N], N - MODEL_TEMPLATE_TOKENS[N]))
    return [(q0, nq) for q0, nq in r if q0 >= 0 and nq >= 1 and q0 + nq <= N]


# ---- B. float64 reference and the derived bound ------------------------------------------------------------------

def _head_ref(qh, kh, vh):
    """one (stream, head) in float64: reference [N, 64] and the three sums the bound is made of"""
    q, k, v = (np.asarray(x, np.float64) for x in (qh, kh, vh))
    N = q.shape[0]
    s = q @ k.T
    m = s.max(axis=1, keepdims=True)
    p = np.exp2(s - m)
    l = p.sum(axis=1, keepdims=True)
    w = p / l
    ref = w @ v
    spread = np.empty_like(ref)                         # sum_j w[i, j] |v[j, d] - ref[i, d]|
    blk = 32        # large enough that the worker threads spend their time inside NumPy, small enough for the cache
    t = np.empty((blk, N, 64))
    for i0 in range(0, N, blk):
        n = min(blk, N - i0)
        np.subtract(v[None, :, :], ref[i0:i0 + n, None, :], out=t[:n])
        np.abs(t[:n], out=t[:n])
        spread[i0:i0 + n] = np.matmul(w[i0:i0 + n, None, :], t[:n])[:, 0, :]
    absv = w @ np.abs(v)                                # sum_j w[i, j] |v[j, d]|
    smag = float((np.abs(q) @ np.abs(k).T).max())       # max over (i, j) of sum_d |q[i, d] k[j, d]|
    return ref, spread, absv, smag, (m + np.log2(l))[:, 0]


def attention_ref64(q, k, v, B, N, H):
    """float64 softmax(q k^T) v in log2 units -> SimpleNamespace(ref, bound, log2_sum), ref and bound [B * N, H * 64],
    log2_sum [B, H, N] the log2 of every row's sum of 2^score.

    bound[i, d] = U (1 + 2 U) A + U |ref| + slack,   A = sum_j w[i, j] |v[j, d] - ref[i, d]|,   U = 2^-8

    The rounding points of k_attn.hip it is derived from - the same in all five paths (softmax_pv for modes 0-2, the
    step and the half step of at3_pass for mode 3 and the subset kernel):
      1. Scores: 4 chained 32x32x16 MFMAs, bf16 operands (products exact in float32), float32 accumulation of 64 terms.
         Modes 0-2 and mode 3's careful pass then subtract a per-query reference in float32 (m_run: lazily raised
         maximum / windowed reference); mode 3's first pass does not. p = 2^(score - reference) by v_exp_f32.
         Each of the <= 64 roundings moves the score by <= 2^-24 max sum_d |q k|, i.e. p by a relative
         eps_p <= ln2 * 64 * 2^-24 * max sum_d |q k| + 2^-22 (the last: one ulp of the hardware exp2).
      2. P is rounded to bf16 (pack_bf16x2 / v_cvt_pk_bf16_f32, nearest even): p~ = p (1 + delta), |delta| <= U. The
         reference subtracted in 1. is common to numerator and denominator and cancels, whatever its value - hence one
         bound for every mode and pass.
      3. The row sum is the float32 sum of the ROUNDED p~ (softmax_pv: psum from the packed bits; mode 3: sum_p8, dot2
         against ones), so out = sum p~ v / sum p~ = ref + sum_j w delta_j (v_j - ref) / (1 + sum_j w delta_j):
         |out - ref| <= U / (1 - U) * A <= U (1 + 2 U) A. This is the main term.
      4. P.V: 32x32x16 MFMAs, V in bf16 (exact input), float32 accumulation over N keys; rescales of O and the sum by
         alpha = 2^(old - new reference) when the reference moves; mode 0 adds the cross-wave combine (four partial
         (m, l, O) through LDS: 2^(m_w - m), 4 multiply-adds per element and per sum), then one multiply by 1 / sum.
         Each is a float32 rounding relative to a partial sum <= sum_j w |v|: N * 2^-24 * sum_j w |v| in all.
      5. The output is rounded to bf16: U |out| <= U |ref| + U |out - ref| (the latter is the 2 U in the main term).
    slack = 2 eps_p A + N 2^-24 sum_j w |v| collects 1. (numerator and denominator both move: the factor 2) and 4.
    It is two to three orders of magnitude below the main term on the test data; nothing here is fitted."""
    q, k, v = (np.asarray(x) for x in (q, k, v))
    ref = np.empty((B * N, H * 64), np.float64)
    bound = np.empty_like(ref)
    lsum = np.empty((B, H, N), np.float64)
    heads = list(_heads(B, N, H))
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        res = list(ex.map(lambda t: _head_ref(q[t[2], t[3]], k[t[2], t[3]], v[t[2], t[3]]), heads))
    for (b, h, rows, cols), (r, spread, absv, smag, ls) in zip(heads, res):
        eps_p = math.log(2.0) * 64 * F32 * smag + 2.0 ** -22
        ref[rows, cols] = r
        bound[rows, cols] = U * (1 + 2 * U) * spread + U * np.abs(r) + 2 * eps_p * spread + N * F32 * absv
        lsum[b, h] = ls
    for a in (ref, bound, lsum):
        a.setflags(write=False)
    return SimpleNamespace(ref=ref, bound=bound, log2_sum=lsum)


def _bf16_normal(rng, shape, scale):
    b = f32_to_bf16_bits((rng.standard_normal(shape) * scale).astype(np.float32))
    return b, bf16_bits_to_f32(b)


@functools.lru_cache(maxsize=None)
def random_case(B, N, H, scale):
    """the data of test_gpu_ops.test_attention / test_attention_mode3 for this shape (same generator, same seed) with its
    float64 reference and bound; computed once, shared by every mode, read-only"""
    rng = np.random.default_rng(N + H)
    D = H * 64
    qb, q = _bf16_normal(rng, (B * N, D), scale * 0.35)
    kb, k = _bf16_normal(rng, (B * N, D), scale)
    vb, v = _bf16_normal(rng, (B * N, D), 1.0)
    r = attention_ref64(q, k, v, B, N, H)
    for a in (qb, kb, vb, q, k, v):
        a.setflags(write=False)
    return SimpleNamespace(B=B, N=N, H=H, qb=qb, kb=kb, vb=vb, q=q, k=k, v=v, ref=r.ref, bound=r.bound, log2_sum=r.log2_sum)


# ---- C. every score near one level -------------------------------------------------------------------------------

OFFSET_LEVELS = (-20.0, -50.0, -64.0, -150.0, 55.0, 90.0)      # the levels of test_attention_uniformly_offset_scores


@functools.lru_cache(maxsize=None)
def offset_case(B, N, level):
    """the construction of test_gpu_ops.test_attention_uniformly_offset_scores, one head, B streams of N tokens: q[:, 0] = 1
    and k[:, 0] = level put every score near `level` log2 units, the other 63 dimensions add a small random part"""
    rng = np.random.default_rng(int(abs(level)) + N)
    M = B * N
    q = np.zeros((M, 64), np.float32)
    k = np.zeros((M, 64), np.float32)
    q[:, 0] = 1.0
    k[:, 0] = level
    q[:, 1:] = rng.standard_normal((M, 63)) * 0.25
    k[:, 1:] = rng.standard_normal((M, 63)) * 0.5
    qb, kb = f32_to_bf16_bits(q), f32_to_bf16_bits(k)
    q, k = bf16_bits_to_f32(qb), bf16_bits_to_f32(kb)
    vb, v = _bf16_normal(rng, (M, 64), 1.0)
    r = attention_ref64(q, k, v, B, N, 1)
    for a in (qb, kb, vb, q, k, v):
        a.setflags(write=False)
    return SimpleNamespace(B=B, N=N, H=1, qb=qb, kb=kb, vb=vb, q=q, k=k, v=v, ref=r.ref, bound=r.bound, log2_sum=r.log2_sum)


# ---- the rounding-point model (CPU only: proves that the bound holds where it should and bites where it should) ---

def model_attention(q, k, v, shift="max", drop_last=False, dup_pad=False, swap=None):
    """One head, [N, 64] each, in float64 except at the kernel's rounding points: p = bf16(2^(score - shift)), the row
    sum over the rounded p, bf16 output. shift: "max" (row maximum), "none" (mode 3's first pass) or an array / number.
    Mutations, each a slip of one key boundary or position:
      drop_last  the last real key is masked (`key >= tokens` taken one too early)
      dup_pad    the first pad key is not masked: its K row is the clamped last real key, its Vt column is zero, so the
                 last key's probability enters the row sum once more and the numerator not at all
      swap       (a, b): V rows a and b change places (a slip in the permuted key order of the P.V operand)"""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    s = q @ k.T
    if isinstance(shift, str):
        m = s.max(axis=1, keepdims=True) if shift == "max" else 0.0
    else:
        m = np.asarray(shift, np.float64).reshape(-1, 1) if np.ndim(shift) else float(shift)
    p = bf16_rne(np.exp2(s - m))
    if drop_last:
        p[:, -1] = 0.0
    if swap is not None:
        v = v.copy()
        v[[swap[0], swap[1]]] = v[[swap[1], swap[0]]]
    l = p.sum(axis=1, keepdims=True)
    if dup_pad:
        l = l + p[:, -1:]
    return bf16_rne((p @ v) / l)
