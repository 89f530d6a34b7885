"""The GEMM epilogues at the edges of their tiles and value by value (inputs, references and the GELU interval:
epilogue_util.py; their premises: test_epilogue_cases.py).

1. Every forced tile configuration at M below, at and just past one, two and three tiles, on exact small integers: the
   operator hooks hand every output back from a buffer that started as 0xff bytes between guard bands, so a row no tile
   stored is a NaN (asserted first), a store past row M an error of the hook, and anything else a wrong integer.
2. Every finite bf16 pattern, the ties of the rounding and 4 * 10^5 ordinary values through ReLU, GELU and the QKV epilogue,
   one value per column (zero operands: y = bias[n]): the rounding must be the oracle's bit for bit, GELU inside the interval
   of a float64 reference."""
import functools

import numpy as np
import pytest

import epilogue_util as eu

pytestmark = pytest.mark.gpu

F = np.float32
SC = eu.SC


def _bits(vt, x):
    return vt.weights.f32_to_bf16_bits(np.asarray(x, F))


# ---- 1. tile edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", eu.EDGE_CONFIGS)
@pytest.mark.parametrize("epi", [0, 1, 4])
def test_x_epilogues_at_every_tile_edge(gpu, cfg, epi):
    """epilogues 0 (plain), 1 (+= the old pair) and 4 (+= positional rows): the exact integers, and the finalized row
    terms within the bounds of test_x_epilogues_pair_and_row_statistics of NumPy's float64 terms of the result"""
    o = eu.edge_operands()
    ab, wb, bias = _bits(gpu, o["a"]), _bits(gpu, o["w"] * SC), o["bias"] * SC
    for M in eu.EDGE_M:
        c0 = None if epi == 0 else o["c0"][:M] * SC
        want = ((o["z"][:M] + (0 if epi == 0 else o["c0"][:M])) * float(SC)).astype(F)
        got, rs = gpu.op_gemm_bf16(ab[:M], wb, bias, c_init=c0, epilogue=epi, cfg=cfg, want_rowstat=True)
        assert np.isfinite(got).all() and np.isfinite(rs).all(), (M, np.argwhere(~np.isfinite(got))[:4])
        assert np.array_equal(got, want), (M, np.argwhere(got != want)[:4])
        ref = eu.row_terms64(got)
        assert np.abs(rs[:, 0] / ref[:, 0] - 1).max() < 2e-5, (M, np.abs(rs[:, 0] / ref[:, 0] - 1).max())
        assert np.abs(rs[:, 1] - ref[:, 1]).max() < 2e-4 * np.abs(ref[:, 1]).max(), M


@functools.lru_cache(maxsize=None)
def _edge_gelu(folded):
    lo, hi, _, _ = eu.gelu_interval(eu.edge_operands()["zf" if folded else "z"][:max(eu.EDGE_M)])
    return lo, hi


@pytest.mark.parametrize("cfg", eu.EDGE_CONFIGS)
@pytest.mark.parametrize("epi", [3, 2])
def test_bf16_epilogues_at_every_tile_edge(gpu, cfg, epi):
    """ReLU (3): bf16_round(max(y, 0)) exactly; GELU (2): inside the interval - both on y = acc + bias and on the folded
    form y = rs0 * acc + (rs1 * colsum + bias) with integer row and column terms"""
    o = eu.edge_operands()
    ab, wb = _bits(gpu, o["a"]), _bits(gpu, o["w"])
    for M in eu.EDGE_M:
        for folded in (False, True):
            y = o["zf" if folded else "z"][:M]
            got = gpu.op_gemm_bf16(ab[:M], wb, o["bias"], epilogue=epi, cfg=cfg, rowstat=o["rs"][:M] if folded else None,
                                   colsum=o["cs"] if folded else None)
            assert np.isfinite(got).all(), (M, folded, np.argwhere(~np.isfinite(got))[:4])
            if epi == 3:
                want = eu.bf16_round(np.maximum(y, 0))
                assert np.array_equal(got, want), (M, folded, np.argwhere(got != want)[:4])
            else:
                lo, hi = _edge_gelu(folded)
                ok = eu.inside(got, lo[:M], hi[:M])
                assert ok.all(), (M, folded, np.argwhere(~ok)[:4])


@pytest.mark.parametrize("cfg", [c for c in eu.EDGE_CONFIGS if eu.qkv_config_fits(c, eu.EDGE_D)])
@pytest.mark.parametrize("perm", [0, 1])
def test_qkv_at_every_tile_edge(gpu, cfg, perm):
    """streams of 4 .. 260 tokens, one and three of them, with and without integer row terms: q scaled and rounded, k and
    V^T exact, and every V^T position that belongs to no token still the zero it started as"""
    D = eu.EDGE_D
    o = eu.edge_operands(N=3 * D)
    ab, wb = _bits(gpu, o["a"]), _bits(gpu, o["w"])
    for B in eu.QKV_B:
        for tokens in eu.QKV_TOKENS:
            M = B * tokens
            for folded in (False, True):
                qk, vt = gpu.op_qkv_bf16(ab[:M], wb, o["bias"], B, tokens, D, cfg=cfg, vt_perm=perm,
                                         rowstat=o["rs"][:M] if folded else None, colsum=o["cs"] if folded else None)
                assert np.isfinite(qk).all() and np.isfinite(vt).all(), (B, tokens, folded)
                want_qk, want_vt = eu.qkv_expected(o["zf" if folded else "z"][:M], B, tokens, D, perm)
                assert np.array_equal(qk, want_qk), (B, tokens, folded, np.argwhere(qk != want_qk)[:4])
                assert np.array_equal(vt, want_vt), (B, tokens, folded, np.argwhere(vt != want_vt)[:4])


@functools.lru_cache(maxsize=None)
def _persistent_operands(rows, N, K):
    """as eu.edge_operands, in float32 (exact: every partial sum is an integer below 2^24) and without the addend"""
    rng = np.random.default_rng(rows + N + K)
    a = rng.integers(-4, 5, size=(rows, K)).astype(F)
    w = rng.integers(-4, 5, size=(N, K)).astype(F)
    bias = rng.integers(-8, 9, size=N).astype(F)
    rs = np.stack([rng.integers(1, 4, size=rows), rng.integers(-2, 3, size=rows)], axis=1).astype(F)
    cs = rng.integers(-5, 6, size=N).astype(F)
    acc = a @ w.T
    out = dict(a=a, w=w, bias=bias, rs=rs, cs=cs, z=acc + bias, zf=rs[:, :1] * acc + (rs[:, 1:] * cs[None, :] + bias[None, :]))
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("r,folded", [(2, True), (130, True), (254, True), (1, False), (129, False), (255, False)])
def test_persistent_relu_with_a_ragged_last_panel(gpu, r, folded):
    """config 19 on 65 row panels x 4 column tiles = 260 tiles (more than 256: the persistent schedule), the last panel
    2 .. 255 rows high; an odd M keeps the persistent kernel only without row terms (launch_gemm256)"""
    N, K, M = 1024, 128, 16384 + r
    o = _persistent_operands(16384 + 255, N, K)
    got = gpu.op_gemm_bf16(_bits(gpu, o["a"][:M]), _bits(gpu, o["w"]), o["bias"], epilogue=3, cfg=19,
                           rowstat=o["rs"][:M] if folded else None, colsum=o["cs"] if folded else None)
    assert np.isfinite(got).all(), np.argwhere(~np.isfinite(got))[:4]
    want = eu.bf16_round(np.maximum(o["zf" if folded else "z"][:M], 0))
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]


@pytest.mark.parametrize("perm,folded", [(0, False), (0, True), (1, False), (1, True)])
def test_persistent_qkv_with_a_ragged_last_panel(gpu, perm, folded):
    """config 19, D = 512, 43 streams of 260 tokens: M = 11,180, 44 x 6 = 264 tiles, the last panel 172 rows, every stream
    starting off the 64-token and the 256-row grid"""
    B, tokens, D = 43, 260, 512
    M = B * tokens
    o = _persistent_operands(M, 3 * D, D)
    qk, vt = gpu.op_qkv_bf16(_bits(gpu, o["a"]), _bits(gpu, o["w"]), o["bias"], B, tokens, D, cfg=19, vt_perm=perm,
                             rowstat=o["rs"] if folded else None, colsum=o["cs"] if folded else None)
    assert np.isfinite(qk).all() and np.isfinite(vt).all()
    want_qk, want_vt = eu.qkv_expected(o["zf" if folded else "z"], B, tokens, D, perm)
    assert np.array_equal(qk, want_qk), np.argwhere(qk != want_qk)[:4]
    assert np.array_equal(vt, want_vt), np.argwhere(vt != want_vt)[:4]


# ---- 2. value by value -------------------------------------------------------------------------------------------

# configuration -> (M, N, K) of a launch whose bias carries N values: the 4-wave kernel's scalar path (2, 3), the 256x256
# kernel (18), and 1 x 260 tiles for the persistent kernel's packed path (19; one launch carries every bf16 pattern)
VALUE_SHAPE = {2: (5, 8192, 128), 3: (5, 8192, 128), 18: (5, 8192, 128), 19: (2, 66560, 128)}


def _push(gpu, cfg, epi, values):
    """every value through the epilogue as the bias of a zero product -> [len(values)]; all M rows must agree"""
    M, N, K = VALUE_SHAPE[cfg]
    za, zw = np.zeros((M, K), np.uint16), np.zeros((N, K), np.uint16)
    out = np.empty(len(values), F)
    for o, cnt, piece in eu.chunks(values, N):
        got = gpu.op_gemm_bf16(za, zw, piece, epilogue=epi, cfg=cfg)
        assert got.shape == (M, N)
        same = (got == got[0]) | (np.isnan(got) & np.isnan(got[0]))
        assert same.all(), (o, np.argwhere(~same)[:4])
        out[o:o + cnt] = got[0, :cnt]
    return out


def _subnormal_report(what, y, got, want):
    """a subnormal value to round comes back as the oracle's bits or as a zero: which, counted where the two differ"""
    y, got, want = (np.asarray(v, F) for v in (y, got, want))
    as_oracle, as_zero = got == want, got == 0
    assert (as_oracle | as_zero).all(), (what, y[~(as_oracle | as_zero)][:4], got[~(as_oracle | as_zero)][:4])
    differ = want != 0
    kept, flushed = int((as_oracle & differ).sum()), int((as_zero & differ).sum())
    print(f"epilogue subnormals {what}: {kept} of {int(differ.sum())} come back as the oracle's bits, {flushed} as zero")


def _mismatch(x, got, want):
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    return None if bad.size == 0 else (bad.size, [(x[i].item(), hex(x[i:i + 1].view(np.uint32)[0]), got[i].item(), want[i].item())
                                                  for i in bad[:4]])


@pytest.mark.parametrize("cfg", [2, 3, 18, 19])
def test_relu_rounds_every_value_like_the_oracle(gpu, cfg):
    x = eu.rounding_inputs()
    got = _push(gpu, cfg, 3, x)
    assert _mismatch(x, got, eu.bf16_round(np.maximum(x, 0))) is None, _mismatch(x, got, eu.bf16_round(np.maximum(x, 0)))
    s = eu.subnormal_inputs()
    _subnormal_report(f"ReLU cfg {cfg}", s, _push(gpu, cfg, 3, s), eu.bf16_round(np.maximum(s, 0)))


@pytest.mark.parametrize("cfg", [2, 3, 18, 19])
def test_gelu_lies_inside_the_interval_at_every_value(gpu, cfg):
    """no tolerance on the bf16 result: it must be one of the (one or two) values a GELU within d of the float64
    reference rounds to, at every input"""
    y = np.concatenate([eu.gelu_inputs(), eu.subnormal_inputs()])
    lo, hi, ref, d = eu.gelu_interval(y)
    got = _push(gpu, cfg, 2, y)
    ratio = eu.least_error(got, ref) / d
    i = int(ratio.argmax())
    print(f"epilogue GELU cfg {cfg}: d_poly = {eu.gelu_d_poly()[0]:.4g}; worst err / d = {ratio[i]:.4f} at y = {y[i]!r} "
          f"(got {got[i]!r}, reference {ref[i]!r}) over {len(y)} inputs")
    ok = eu.inside(got, lo, hi)
    assert ok.all(), (int((~ok).sum()), [(y[j].item(), got[j].item(), lo[j].item(), hi[j].item()) for j in np.flatnonzero(~ok)[:4]])


@pytest.mark.parametrize("cfg", [2, 3, 18])
def test_qkv_rounds_every_value_like_the_oracle(gpu, cfg):
    """D = 1024, one stream of 12 tokens: a bias of 3 x 1024 values, three launches with the thirds rotated, so that every
    value is a q (float32(y * QK_SCALE) rounded), a k and a v (y rounded; V^T through the transposed store). A q whose
    product is subnormal goes by the rule of the subnormal inputs."""
    D, tokens = 1024, 12
    x = np.concatenate([eu.rounding_inputs(), eu.subnormal_inputs()])
    x = np.concatenate([x, np.zeros(-len(x) % (3 * D), F)])
    za, zw = np.zeros((tokens, D), np.uint16), np.zeros((3 * D, D), np.uint16)
    got = {k: np.empty(len(x), F) for k in "qkv"}
    for o in range(0, len(x), 3 * D):
        thirds = x[o:o + 3 * D].reshape(3, D)
        for rot in range(3):
            order = [(j + rot) % 3 for j in range(3)]            # order[section] = the third that section carries
            qk, vt = gpu.op_qkv_bf16(za, zw, thirds[order].ravel(), 1, tokens, D, cfg=cfg, vt_perm=rot & 1)
            v = vt[:, :, :tokens].reshape(D, tokens).T           # every position below 12 belongs to a token in either order
            for name, sec in (("q", qk[:, :D]), ("k", qk[:, D:]), ("v", v)):
                same = (sec == sec[0]) | (np.isnan(sec) & np.isnan(sec[0]))
                assert same.all(), (name, o, rot)
            assert np.all(vt[:, :, tokens:] == 0)
            for name, sec, j in (("q", qk[0, :D], order[0]), ("k", qk[0, D:], order[1]), ("v", v[0], order[2])):
                got[name][o + j * D:o + (j + 1) * D] = sec
    normal = np.abs(x) >= eu.TINY
    for name in "kv":
        bad = _mismatch(x[normal | (x == 0)], got[name][normal | (x == 0)], eu.bf16_round(x[normal | (x == 0)]))
        assert bad is None, (name, bad)
        _subnormal_report(f"{name} cfg {cfg}", x[~normal & (x != 0)], got[name][~normal & (x != 0)], eu.bf16_round(x[~normal & (x != 0)]))
    p = eu.q_product(x)
    pn = (np.abs(p) >= eu.TINY) | (p == 0)
    bad = _mismatch(x[pn], got["q"][pn], eu.bf16_round(p[pn]))
    assert bad is None, ("q", bad)
    _subnormal_report(f"q cfg {cfg} (subnormal product)", p[~pn], got["q"][~pn], eu.bf16_round(p[~pn]))
