"""Inputs, float64 reference, a derived per-element error bound and a float32 NumPy model of the folded LayerNorm chain
(X-epilogue statistics -> row terms -> fold -> consuming GEMM epilogue), shared by
test_ln_chain_cases.py (CPU: the bound holds for the honest model and rejects the mutations) and test_gpu_ln_chain.py.

Notation: u = 2^-24 (float32 unit roundoff), ub = 2^-8 (bf16: 8 significand bits, round to nearest even - a value just
above a tie, 1 + 2^-8 + tiny, moves by 2^-8 of itself; 2^-9 is NOT a bound), D columns in nchunk = D / 32 chunks,
A = max_k |x[m][k]|, mu / var the float64 mean / population variance of the float32 row, sigma = sqrt(var + eps),
r = 1 / sigma. First-order counts are multiplied by HO = 1 + 2^-6 for the products of error terms (every relative error
below is < 1e-2 on the test data, so the second-order part is < 1e-2 of the first-order one).

ROW TERMS - the float32 operations of the chunked parallel-variance form (x_chunk_stats in k_gemm_util.hpp, then
rowstat_finalize_kernel / the panel's last workgroup in k_gemm256.hip / ln_finish; the three differ in summation order
only, and every sum below is bounded for ANY order: n - 1 roundings of at most u times the sum of magnitudes):
  1. s_c, the sum of a chunk's 32 values: |s_c - S_c| <= 31 u sum|x| <= 31 u 32 A, so the chunk mean s_c / 32 (exact
     scaling) is within 31 u A of mu_c.
  2. q_c = sum (x - s_c / 32)^2: one rounding in each difference (relative 2 u on its square), 32 fused accumulations:
     q_c = (Q_c + 32 (s_c / 32 - mu_c)^2) (1 + 34 u), the middle term <= 32 (31 u A)^2.
  3. mean: nchunk - 1 roundings in the sum of the s_c, one in the division: |mean - mu| <= (31 + nchunk) u A.
  4. d_c = s_c / 32 - mean, one rounding with |d_c| <= 2 A: |d_c - (mu_c - mu)| <= delta = (64 + nchunk) u A.
  5. M2 = sum_c (q_c + 32 d_c^2): square, add, nchunk - 1 roundings of non-negative terms: relative (2 + nchunk) u on top of
     2.; the delta of 4. moves 32 sum_c d_c^2 by at most 2 delta D sqrt(var) + D delta^2 (Cauchy-Schwarz, 32 sum (mu_c - mu)^2 <= D var).
  6. v = M2 / D + eps: two roundings of non-negative terms. So |v / sigma^2 - 1| <= (38 + nchunk) u + 2 delta / sigma + 5/4 (delta / sigma)^2
     (the last factor takes in the middle term of 2.: (31 / 64)^2 < 1/4).
  7. rstd = 1 / sqrt(v), both correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt): half of 6. plus 2 u:

         |rstd / r - 1| <= E_r = HO (u (21 + nchunk / 2) + (64 + nchunk) u A / sigma + 5/8 ((64 + nchunk) u A / sigma)^2)

     c0 = 21, c1 = 1/2, c2 = 64, c3 = 1 in the form u (c0 + c1 nchunk + (c2 + c3 nchunk) A / sigma). The A / sigma term is
     what a DC-dominated row costs: 1e-7 for N(0, 1), 5e-3 for 1000 + N(0, 1).
  8. -mean * rstd, one more rounding: |. - (-mu r)| <= E_b = HO r (|mu| (E_r + u) + (31 + nchunk) u A).
  Chunk partials: |s_c - S_c| <= 31 u sum_c |x|, |q_c - Q_c| <= 35 u Q_c + 33 (31 u A_c)^2 with A_c the chunk's max |x|, q_c >= 0.

FOLD (fold_layernorm_kernel): Wf = bf16(gamma * W) is one float32 product and one rounding to nearest even - NumPy gives
the same bits. colsum = sum_k Wf, any order: |.| <= D u sum|Wf|. cvec = sum_k beta W + bias: one rounding per product,
D - 1 in the sum, one for the bias: <= (D + 2) u (sum|beta W| + |bias|).

Y = fma(rstd, acc, fma(-mean rstd, colsum, cvec)) against y1 = r acc - mu r colsum + cvec (acc = xh Wf^T in float64):
    dy = HO (E_r |r acc| + E_b |colsum| + r D u sum_k |xh Wf| + |mu r| D u sum|Wf| + (D + 2) u (sum|beta W| + |bias|)
             + u (2 |mu r colsum| + 2 |cvec| + |r acc| + |y1|))
the third term is the float32 accumulation of D exact products in any order (as attention_util.py takes its N * F32 term),
the last line covers the epilogue's roundings whether or not the compiler fuses them (two fma: half of it).
Consumers: ReLU and k, v of QKV round y to bf16: dy + ub (|f(y1)| + dy); q = y * scale adds u |q|; GELU has Lipschitz
constant < 1.13 and the tolerance test_gpu_ops.py grants its polynomial and rounding: 1.13 dy + |ref| ub + 2e-3."""
import functools
from types import SimpleNamespace

import numpy as np
from scipy.special import erf

from gstreamer_vit_tracker_amd.weights import bf16_bits_to_f32, f32_to_bf16_bits

U = 2.0 ** -24
UB = 2.0 ** -8
HO = 1.0 + 2.0 ** -6
EPS = 1e-6
CHUNK = 32
QK_SCALE = np.float32(0.125 * 1.4426950408889634)
GELU, RELU, QKV = 2, 3, 4
CONSUMERS = (GELU, RELU, QKV)
CLASSES = "abcdefg"

# D -> routes (0 finalize launch, 1 inside the 256x256 producer, 2 combined in the consumer)
ROUTES = {128: (0, 2), 256: (0, 1, 2), 384: (0, 2), 768: (0, 1, 2), 1024: (0, 1, 2), 2048: (0,)}
QKV_D = (128, 256, 768)
N_ACT = 256


def shape(D, consumer, route):
    """(B, tokens, N): M = B * tokens is 71 (two 64-row tiles, the second ragged; odd, so the last even row's 16-byte pair
    load of the row terms ends behind the array) or, for the 256x256 producer, 299 (two 256-row panels, the second short).
    QKV needs tokens % 4 == 0, so M cannot be odd there: 72 and 300. No M is a multiple of 7: the classes drift across
    row parities and tile positions."""
    big = route == 1
    if consumer == QKV:
        return (3, 100 if big else 24, 3 * D)
    return (1, 299 if big else 71, N_ACT)


def consumer_cfgs(D, N, route, consumer):
    cfgs = list(range(9)) if D == 768 else [2, 3]
    if route != 2 and N % 256 == 0 and (consumer != QKV or D % 256 == 0):
        cfgs.append(18)
    return cfgs


def all_cases():
    """(D, consumer, route) of every chain the GPU test runs"""
    return [(D, c, rt) for D, routes in ROUTES.items() for c in CONSUMERS if c != QKV or D in QKV_D for rt in routes]


# ---- inputs ------------------------------------------------------------------------------------------------------

def row_classes(M):
    return np.arange(M) % 7


@functools.lru_cache(maxsize=None)
def make_x(M, D):
    """[M, D] float32, class of row m = CLASSES[m % 7]:
    a N(0, 1); b 30 + N(0, 1); c 1000 + N(0, 1); d the constant 0.1f; e N(0, 1) with one 200 in the last chunk;
    f chunk means alternating +4 / -4, spread 0.05 inside a chunk; g 1e-3 N(0, 1)"""
    rng = np.random.default_rng(7000 + 13 * M + D)
    z = rng.standard_normal((M, D))
    x = np.empty((M, D), np.float64)
    cls = row_classes(M)
    x[cls == 0] = z[cls == 0]
    x[cls == 1] = 30.0 + z[cls == 1]
    x[cls == 2] = 1000.0 + z[cls == 2]
    x[cls == 3] = 0.0
    x[cls == 4] = z[cls == 4]
    x[cls == 5] = np.where((np.arange(D) // CHUNK) % 2 == 0, 4.0, -4.0)[None, :] + 0.05 * z[cls == 5]
    x[cls == 6] = 1e-3 * z[cls == 6]
    x = x.astype(np.float32)
    x[cls == 3] = np.float32(0.1)
    x[cls == 4, D - 5] = 200.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def make_params(N, D):
    rng = np.random.default_rng(9000 + 17 * N + D)
    gamma = (1.0 + 0.2 * rng.standard_normal(D)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(D)).astype(np.float32)
    wb = f32_to_bf16_bits((0.05 * rng.standard_normal((N, D))).astype(np.float32))
    bias = (0.3 * rng.standard_normal(N)).astype(np.float32)
    p = SimpleNamespace(N=N, D=D, gamma=gamma, beta=beta, wb=wb, w=bf16_bits_to_f32(wb), bias=bias)
    for a in (gamma, beta, wb, p.w, bias):
        a.setflags(write=False)
    return p


def split_pair(x, lo_shift=12):
    """the 3-byte pair of numerical specification v3: hi = bf16(x) (bits), lo8 = clamp(rint((x - hi) * 2^s), +-127) (int8)"""
    x = np.asarray(x, np.float32)
    hb = f32_to_bf16_bits(x)
    lo = np.clip(np.rint((x - bf16_bits_to_f32(hb)).astype(np.float32) * np.float32(2.0 ** lo_shift)), -127, 127)
    return hb, lo.astype(np.int8)


def vt_layout(v, B, tokens, D):
    """v [B * tokens, D] -> Vt [B * D / 64, 64, tokens] (natural key order), the layout of the QKV epilogue"""
    return v.reshape(B, tokens, D // 64, 64).transpose(0, 2, 3, 1).reshape(-1, 64, tokens)


def qkv_natural(qk, vt, B, tokens, D):
    """qk [M, 2D] and Vt [B * D / 64, 64, npad] as the hook returns them -> [M, 3D]"""
    v = vt[:, :, :tokens].reshape(B, D // 64, 64, tokens).transpose(0, 3, 1, 2).reshape(B * tokens, D)
    return np.concatenate([qk, v], axis=1)


# ---- float64 reference and the derived bound ---------------------------------------------------------------------

def gelu64(y):
    return 0.5 * y * (1.0 + erf(y * 0.7071067811865476))


def row_terms_ref(x, eps=EPS):
    """float64 row terms of the float32 rows and their bounds E_r (relative, rstd) and E_b (absolute, -mean * rstd)"""
    x64 = np.asarray(x, np.float64)
    D = x64.shape[1]
    nchunk = D // CHUNK
    mu = x64.mean(axis=1)
    var = x64.var(axis=1)
    sigma = np.sqrt(var + eps)
    r = 1.0 / sigma
    A = np.abs(x64).max(axis=1)
    t = (64 + nchunk) * U * A / sigma
    E_r = HO * (U * (21 + nchunk / 2) + t + 0.625 * t * t)
    E_b = HO * r * (np.abs(mu) * (E_r + U) + (31 + nchunk) * U * A)
    return SimpleNamespace(mu=mu, var=var, r=r, nmr=-mu * r, E_r=E_r, E_b=E_b, A=A, sigma=sigma)


def cstat_ref(x):
    """float64 chunk partials [M, nchunk, 2] of the float32 rows and their bounds"""
    c = np.asarray(x, np.float64).reshape(x.shape[0], -1, CHUNK)
    S = c.sum(axis=2)
    Q = ((c - S[..., None] / CHUNK) ** 2).sum(axis=2)
    Ac = np.abs(c).max(axis=2)
    return SimpleNamespace(S=S, Q=Q, dS=31 * U * np.abs(c).sum(axis=2), dQ=35 * U * Q + 33 * (31 * U * Ac) ** 2)


def fold_ref(p):
    """float64 fold of float32 gamma / beta / bias and bf16 W: exact Wf bits, colsum, cvec and the two summation bounds"""
    wfb = f32_to_bf16_bits(p.gamma[None, :] * p.w)              # one float32 product, one rounding to nearest even
    wf = bf16_bits_to_f32(wfb).astype(np.float64)
    w64, beta = p.w.astype(np.float64), p.beta.astype(np.float64)
    return SimpleNamespace(wfb=wfb, wf=wf, colsum=wf.sum(axis=1), cvec=w64 @ beta + p.bias,
                           d_colsum=p.D * U * np.abs(wf).sum(axis=1),
                           d_cvec=(p.D + 2) * U * (np.abs(w64) @ np.abs(beta) + np.abs(p.bias.astype(np.float64))))


def apply_consumer(y1, dy, consumer, D):
    """the consumer's function of y1 [M, N] in float64 and the bound of its bf16 output given |y - y1| <= dy"""
    if consumer == GELU:
        ref = gelu64(y1)
        return ref, 1.13 * dy + np.abs(ref) * UB + 2e-3
    if consumer == RELU:
        ref = np.maximum(y1, 0.0)
        return ref, dy + UB * (ref + dy)
    ref, d = y1.copy(), dy.copy()
    ref[:, :D] *= float(QK_SCALE)
    d[:, :D] = d[:, :D] * float(QK_SCALE) + U * np.abs(ref[:, :D])
    return ref, d + UB * (np.abs(ref) + d)


@functools.lru_cache(maxsize=None)
def reference(M, D, N, consumer, eps=EPS):
    """R1: everything in float64 from the float32 x -> ref, bound [M, N] (QKV: [M, 3D] as q | k | v) and the parts"""
    x, p = make_x(M, D), make_params(N, D)
    rt, f = row_terms_ref(x, eps), fold_ref(p)
    xh = bf16_bits_to_f32(f32_to_bf16_bits(x)).astype(np.float64)
    acc = xh @ f.wf.T
    r, mur = rt.r[:, None], (rt.mu * rt.r)[:, None]
    y1 = r * acc - mur * f.colsum[None, :] + f.cvec[None, :]
    dy = HO * (rt.E_r[:, None] * np.abs(r * acc) + rt.E_b[:, None] * np.abs(f.colsum)[None, :]
               + r * (D * U) * (np.abs(xh) @ np.abs(f.wf).T) + np.abs(mur) * f.d_colsum[None, :] + f.d_cvec[None, :]
               + U * (2 * np.abs(mur * f.colsum[None, :]) + 2 * np.abs(f.cvec)[None, :] + np.abs(r * acc) + np.abs(y1)))
    ref, bound = apply_consumer(y1, dy, consumer, D)
    for a in (ref, bound, y1, dy):
        a.setflags(write=False)
    return SimpleNamespace(x=x, p=p, rt=rt, fold=f, y1=y1, dy=dy, ref=ref, bound=bound, cls=row_classes(M))


def worst_by_class(err, bound, cls):
    """largest err / bound per row class (NaN counts as infinite) -> {class letter: ratio}"""
    ratio = np.where(np.isfinite(err), err, np.inf) / bound
    ratio = ratio.reshape(ratio.shape[0], -1).max(axis=1)
    return {CLASSES[c]: float(ratio[cls == c].max()) for c in range(7) if (cls == c).any()}


def describe_worst(got, ref, bound, cls):
    """class, row, parity and column of the element furthest over the bound (None if every element is inside)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    ratio = np.where(np.isfinite(err), err, np.inf) / bound
    if not (ratio > 1.0).any():
        return None
    m, n = np.unravel_index(ratio.argmax(), ratio.shape)
    return (f"{int((ratio > 1.0).sum())} elements over the bound; worst: class {CLASSES[cls[m]]} row {m} "
            f"({'odd' if m & 1 else 'even'}) column {n}: got {got[m, n]!r}, reference {ref[m, n]!r}, bound {bound[m, n]:.3g}, "
            f"err / bound {ratio[m, n]:.3g}")


# ---- the float32 NumPy model (CPU only) --------------------------------------------------------------------------

F = np.float32
MUTATIONS = ("neighbour_row", "half_chunks", "no_eps", "naive_variance", "colsum_unrounded")


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64, one rounding of the sum"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _seq_sum(a, axis):
    """sequential float32 sum along an axis"""
    a = np.moveaxis(np.asarray(a, F), axis, 0)
    s = np.zeros(a.shape[1:], F)
    for t in a:
        s = (s + t).astype(F)
    return s


def _gelu_poly(y):
    """gelu_erf of k_gemm_util.hpp in float32"""
    a = np.abs(y)
    p = _fma(F(-0.0004733149544335902), a, F(0.007084596436470747))
    for c in (-0.05182747542858124, -0.45999234914779663, -1.1507878303527832, -1.000037670135498):
        p = _fma(p, a, F(c))
    return _fma(-a, np.exp2(p.astype(np.float64)).astype(F), np.maximum(y, F(0)))


def model_chain(M, D, N, consumer, eps=EPS, mutation=None):
    """The chain in float32 with sequential sums, the combination in the kernels' formula, the fold, and fma as a float64
    product rounded once -> SimpleNamespace(out [M, N] or [M, 3D], rowstat [M, 2], cstat [M, nchunk, 2]).
    Mutations: neighbour_row (terms of row m ^ 1), half_chunks (only the first half of a row's chunks combined), no_eps,
    naive_variance (float32 E[x^2] - mean^2), colsum_unrounded (column sums of gamma * W before its rounding to bf16)."""
    assert mutation is None or mutation in MUTATIONS
    x, p = make_x(M, D), make_params(N, D)
    nchunk = D // CHUNK
    c = x.reshape(M, nchunk, CHUNK)
    s_c = _seq_sum(c, 2)
    mc = (s_c * F(1.0 / CHUNK)).astype(F)
    q_c = np.zeros((M, nchunk), F)
    for i in range(CHUNK):
        d = (c[:, :, i] - mc).astype(F)
        q_c = _fma(d, d, q_c)
    use = nchunk // 2 if mutation == "half_chunks" else nchunk
    Df = F(D)
    mean = (_seq_sum(s_c[:, :use], 1) / Df).astype(F)
    d_c = (s_c[:, :use] * F(1.0 / CHUNK) - mean[:, None]).astype(F)
    m2 = _seq_sum((q_c[:, :use] + (F(CHUNK) * (d_c * d_c).astype(F)).astype(F)).astype(F), 1)
    var = (m2 / Df).astype(F)
    if mutation == "naive_variance":
        var = ((_seq_sum((x * x).astype(F), 1) / Df).astype(F) - (mean * mean).astype(F)).astype(F)
    e = F(0.0) if mutation == "no_eps" else F(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (F(1.0) / np.sqrt((var + e).astype(F)).astype(F)).astype(F)
        nmr = (-mean * rstd).astype(F)
    rowstat = np.stack([rstd, nmr], axis=1)
    if mutation == "neighbour_row":
        nb = np.arange(M) ^ 1
        nb[nb >= M] = M - 1
        rstd, nmr = rstd[nb], nmr[nb]
    gw = (p.gamma[None, :] * p.w).astype(F)
    wf = bf16_bits_to_f32(f32_to_bf16_bits(gw))
    colsum = _seq_sum(gw if mutation == "colsum_unrounded" else wf, 1)
    cvec = (_seq_sum((p.beta[None, :] * p.w).astype(F), 1) + p.bias).astype(F)
    xh = bf16_bits_to_f32(f32_to_bf16_bits(x))
    acc = (xh @ wf.T).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        y = _fma(rstd[:, None], acc, _fma(nmr[:, None], colsum[None, :], cvec[None, :]))
        if consumer == GELU:
            v = _gelu_poly(y)
        elif consumer == RELU:
            v = np.maximum(y, F(0))
        else:
            v = y.copy()
            v[:, :D] = (v[:, :D] * QK_SCALE).astype(F)
        bad = ~np.isfinite(v)
        out = bf16_bits_to_f32(f32_to_bf16_bits(np.where(bad, F(0), v)))
        out[bad] = np.nan
    return SimpleNamespace(out=out, rowstat=rowstat, cstat=np.stack([s_c, q_c], axis=2))


# ---- the LayerNorm kernels (layernorm_kernel / layernorm_wide_kernel of k_misc.hip: two-pass variance) ------------

def layernorm_ref(x, gamma, beta, eps=EPS):
    """float64 LayerNorm of float32 rows and the bound of the kernels' bf16 output, counted the same way:
    mean = sum / D in any order: |mean - mu| <= delta = D u A. v = x - mean (one rounding), sum of v^2 in any order:
    relative (D + 2) u on D var + D delta^2, / D and + eps two more, so rstd = 1 / sqrt(.) has
    |rstd / r - 1| <= E = HO (u (D / 2 + 4) + (delta / sigma)^2 / 2); y = ((v rstd) gamma + beta), three more roundings:
        |y - ref| <= dy = HO |gamma| r (delta + |x - mu| (E + 3 u)) + u |ref|,   bound = dy + ub (|ref| + dy)"""
    x64 = np.asarray(x, np.float64)
    g, b = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    D = x64.shape[1]
    mu = x64.mean(axis=1, keepdims=True)
    sigma = np.sqrt(x64.var(axis=1, keepdims=True) + eps)
    r = 1.0 / sigma
    delta = D * U * np.abs(x64).max(axis=1, keepdims=True)
    E = HO * (U * (D / 2 + 4) + 0.5 * (delta / sigma) ** 2)
    ref = (x64 - mu) * r * g + b
    dy = HO * np.abs(g) * r * (delta + np.abs(x64 - mu) * (E + 3 * U)) + U * np.abs(ref)
    return ref, dy + UB * (np.abs(ref) + dy)


LN_CLASSES = (0, 1, 3, 6)          # a, b, d, g of make_x


def layernorm_rows(M, D, shift):
    """M rows of width D, row m of class LN_CLASSES[(m + shift) % 4], cut from make_x (row index = class there)"""
    src = make_x(71, D)
    return np.stack([src[LN_CLASSES[(m + shift) % 4] + 7 * (m % 9)] for m in range(M)])
