"""The premises of test_gpu_attention_edges.py, proved on the float64 reference and a NumPy model of the kernels' rounding
points alone (no GPU): the selector data make the exact answer V[sel] inside the window of mode 3's unchecked first pass,
the derived bound holds for every softmax reference a kernel may subtract, and key-boundary slips of weight ~1/N - which
the older tolerance 0.02 * max|ref| lets through - break one of the two new checks."""
import numpy as np
import pytest

import attention_util as au


@pytest.mark.parametrize("B,N,H", au.SELECTOR_SHAPES + au.SELECTOR_SHAPES_ANY_N)
def test_selector_premises(B, N, H):
    """in float64: every row sum is 2^56.0000003 at most (to the seven decimals given; the first pass of mode 3 keeps a row
    whose sum lies in [2^-60, 2^60]), the other keys together add at most 1.8e-6 to any output element, and the reference
    rounds to V[sel] bit for bit - so the GPU tests may ask for equality"""
    c = au.selector_case(B, N, H)
    r = au.attention_ref64(c.q, c.k, c.v, B, N, H)
    assert r.log2_sum.min() >= au.SEL_MATCH
    assert np.round(r.log2_sum.max(), 7) <= 56.0000003
    assert -60.0 < r.log2_sum.min() and r.log2_sum.max() < 60.0
    w_sel = np.exp2(au.SEL_MATCH - r.log2_sum)                              # [B, H, N]: the weight of the matching key
    w_sel = w_sel.transpose(0, 2, 1).reshape(B * N, H)
    others = r.ref - np.repeat(w_sel, 64, axis=1) * c.want                  # sum over j != sel of w[i, j] v[j, d]
    print(f"selector B={B} N={N} H={H}: log2 row sum <= {r.log2_sum.max():.9f}, other keys <= {np.abs(others).max():.3g}")
    assert np.abs(others).max() <= 1.8e-6
    assert np.array_equal(au.bf16_rne(r.ref), c.want)
    assert np.all(c.want % 2 != 0) and np.abs(c.want).max() <= 15
    # every key is some query's answer, in every (stream, head), and no two heads share the permutation
    assert all(np.array_equal(np.sort(c.sel[b, h]), np.arange(N)) for b in range(B) for h in range(H))
    if B * H > 1:
        assert not np.array_equal(c.sel[0, 0], c.sel[-1, -1])


def _head(N, scale, seed):
    rng = np.random.default_rng(seed)
    return (au.bf16_rne(rng.standard_normal((N, 64)) * scale * 0.35), au.bf16_rne(rng.standard_normal((N, 64)) * scale),
            au.bf16_rne(rng.standard_normal((N, 64))))


@pytest.mark.parametrize("N,scale", [(16, 3.0), (33, 3.0), (36, 2.0), (100, 1.0), (320, 1.0), (720, 1.0), (980, 0.5)])
def test_bound_holds_for_every_reference(N, scale):
    """the rounding-point model with the three references a path may subtract - none (mode 3's first pass), an arbitrary one
    (a lazily raised maximum, the windowed reference) and the row maximum - stays inside the bound at every element, and
    not by much: the worst ratio over these shapes and seeds is 0.98 (N = 16, scale 3: a handful of keys carry a row)"""
    worst = 0.0
    for seed in range(6):
        q, k, v = _head(N, scale, seed)
        r = au.attention_ref64(q, k, v, 1, N, 1)
        arbitrary = np.random.default_rng(100 + seed).uniform(-6.0, 6.0, N)
        for shift in ("none", arbitrary, "max"):
            ratio = np.abs(au.model_attention(q, k, v, shift) - r.ref) / r.bound
            worst = max(worst, float(ratio.max()))
    print(f"model N={N} scale={scale}: max(err / bound) = {worst:.4f}")
    assert worst <= 1.0
    if N == 16:
        assert worst > 0.9          # tight, not generous


MUTATIONS = {"drop_last": dict(drop_last=True), "dup_pad": dict(dup_pad=True), "swap": dict(swap=(4, 8))}


def test_diffuse_slips_pass_the_old_tolerance_and_break_the_bound():
    """N = 980, score scale 0.5 (ViT-L's token count with flat attention): each slip moves the output by about one key's
    weight, 1e-3 - far inside 0.02 * max(1, max|ref|) and mean 2e-3, the tolerance of test_gpu_ops - yet dropping the last
    key or swapping two V rows of a 16-key group (4 and 8: the rows the permuted order exchanges) puts at least 1 % of the
    elements over the derived bound, which a correct kernel never crosses. The duplicated pad key rescales a row by
    1 / (1 + w_last): no element crosses the bound here; the exact selector catches that one (next test)."""
    q, k, v = _head(980, 0.5, 0)
    r = au.attention_ref64(q, k, v, 1, 980, 1)
    over = {}
    for name, kw in [("none", {})] + list(MUTATIONS.items()):
        err = np.abs(au.model_attention(q, k, v, "none", **kw) - r.ref)
        assert err.max() < 0.02 * max(1.0, np.abs(r.ref).max()) and err.mean() < 2e-3, name     # invisible before
        over[name] = float((err > r.bound).mean())
    print("share of elements over the bound at N = 980, scale 0.5:", over)
    assert over["none"] == 0.0
    assert over["drop_last"] >= 0.01
    assert over["swap"] >= 0.01


@pytest.mark.parametrize("N", [36, 980])
def test_selector_catches_every_slip(N):
    """on the selector data each of the three slips changes the bf16 output of the queries that select the keys involved
    (the duplicated pad key halves the row of the query whose answer is the last key), so equality with V[sel] fails"""
    c = au.selector_case(1, N, 1)
    assert np.array_equal(au.model_attention(c.q, c.k, c.v, "none"), c.want)
    assert np.array_equal(au.model_attention(c.q, c.k, c.v, "max"), c.want)
    for name, kw in MUTATIONS.items():
        got = au.model_attention(c.q, c.k, c.v, "none", **kw)
        bad = np.flatnonzero((got != c.want).any(axis=1))
        assert bad.size >= 1, name
        hit = {"drop_last": [N - 1], "dup_pad": [N - 1], "swap": [4, 8]}[name]
        assert sorted(c.sel[0, 0][bad]) == hit, name


def test_subset_ranges_cover_the_edges():
    assert au.subset_ranges(16) == [(0, 16), (1, 1), (15, 1)]
    assert au.subset_ranges(980) == [(0, 980), (196, 784), (1, 1), (17, 33), (979, 1), (940, 40)]
    for N in (36, 68, 80, 96, 100, 320, 720, 1008):
        assert all(0 <= q0 and nq >= 1 and q0 + nq <= N for q0, nq in au.subset_ranges(N))
