"""The score launch of the appearance check (csrc/k_appearance.hip) through the operator hook vt_op_appearance_score, on
the MI355X, against the NumPy float64 restatement of tests/appearance_util.py.

Integer-valued bf16 data with |v| <= 16 make all five sums exact in ANY order of the additions (every partial sum is an
integer below 2^53): there the kernel's sums are compared bit for bit. On random data the similarity is held to the bound
derived in appearance_util's docstring, whose premise each test asserts on its own data."""
import numpy as np
import pytest

import appearance_util as au

pytestmark = pytest.mark.gpu

CHUNK = 8               # VT_APPEAR_CHUNK_ROWS: rows per workgroup of the score launch
VITL14 = (196, 588, 640)
SHAPES = [(1, 12, 16), (16, 768, 768), VITL14, (13, 48, 64)]       # (nt, cols, kpad); 196 and 13 are no multiples of 8
NAN = np.uint16(0x7FC0)


def _bits(x):
    return au.f32_to_bf16_bits(np.asarray(x, np.float32))


def _ints(rng, n, nt, cols, kpad, lo=-16, hi=17):
    v = np.full((n, nt, kpad), NAN, np.uint16)
    v[:, :, :cols] = _bits(rng.integers(lo, hi, size=(n, nt, cols)).astype(np.float32))
    return v


def _want(a, p, cols):
    return np.array([au.sums(x, y, cols) for x, y in zip(a, p)])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", [1, 2, 33])
def test_integer_sums_are_bit_equal(gpu, shape, n):
    nt, cols, kpad = shape
    rng = np.random.default_rng(nt * 1000 + n)
    a, p = _ints(rng, n, nt, cols, kpad), _ints(rng, n, nt, cols, kpad)
    got = gpu.op_appearance_score(a, p, cols)
    want = _want(a, p, cols)
    assert np.array_equal(got["sums"].view(np.uint64), want.view(np.uint64)), (got["sums"], want)
    for i in range(n):
        sim, status = au.finish(want[i], nt * cols)
        assert got["status"][i] == status
        f = au.premise(a[i], p[i], cols)
        if status == 1:
            assert f >= 0.25, f"premise: {f}"
            assert abs(float(got["similarity"][i]) - float(sim)) <= au.sim_tolerance(nt * cols, 0.25, sim), (i, got["similarity"][i], sim)


@pytest.mark.parametrize("shape", [(16, 768, 768), VITL14])
def test_every_single_element_counts(gpu, shape):
    """slot 0 is the base; every other slot differs from it in ONE element of the probe: the first and the last element
    and the first element of every chunk. Each must move Sp, Spp and Sap by exactly what NumPy says."""
    nt, cols, kpad = shape
    rng = np.random.default_rng(7)
    base_a, base_p = _ints(rng, 1, nt, cols, kpad, 1, 17), _ints(rng, 1, nt, cols, kpad, 1, 17)      # no zeros: a sign flip is a change
    where = [(0, 0), (nt - 1, cols - 1)] + [(r, 0) for r in range(0, nt, CHUNK)]
    n = 1 + len(where)
    a, p = np.repeat(base_a, n, axis=0), np.repeat(base_p, n, axis=0)
    for i, (r, c) in enumerate(where):
        p[i + 1, r, c] ^= np.uint16(0x8000)
    got = gpu.op_appearance_score(a, p, cols)["sums"]
    want = _want(a, p, cols)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for i in range(1, n):
        assert got[i][1] != got[0][1] and got[i][4] != got[0][4], f"element {where[i - 1]} does not reach the sums"
        assert got[i][0] == got[0][0] and got[i][2] == got[0][2] and got[i][3] == got[0][3]
    # and one of the anchor, in the last pad-adjacent column
    a2 = a[:2].copy()
    a2[1, nt - 1, cols - 1] ^= np.uint16(0x8000)
    g2 = gpu.op_appearance_score(a2, p[:2], cols)["sums"]
    assert g2[1][0] != g2[0][0] and np.array_equal(g2.view(np.uint64), _want(a2, p[:2], cols).view(np.uint64))


def test_pad_columns_are_never_read(gpu):
    nt, cols, kpad = VITL14
    rng = np.random.default_rng(8)
    a, p = _ints(rng, 2, nt, cols, kpad), _ints(rng, 2, nt, cols, kpad)
    got = gpu.op_appearance_score(a, p, cols)
    a[:, :, cols:] = _bits([3.0])[0]
    p[:, :, cols:] = np.uint16(0x7F80)      # +inf
    again = gpu.op_appearance_score(a, p, cols)
    assert np.array_equal(got["sums"].view(np.uint64), again["sums"].view(np.uint64))
    assert np.array_equal(got["similarity"].view(np.uint32), again["similarity"].view(np.uint32))
    assert np.isfinite(got["sums"]).all()


@pytest.mark.parametrize("shape", [(16, 768, 768), VITL14])
def test_random_data_within_the_derived_bound(gpu, shape, capsys):
    nt, cols, kpad = shape
    rng = np.random.default_rng(9)
    n = 4
    fa = rng.standard_normal((n, nt, kpad)).astype(np.float32)
    mix = np.array([0.95, 0.5, 0.0, -0.7], np.float32).reshape(n, 1, 1)
    fp = mix * fa + np.sqrt(1 - mix * mix) * rng.standard_normal((n, nt, kpad)).astype(np.float32) + np.float32(0.25)
    a, p = _bits(fa), _bits(fp)
    a[:, :, cols:] = NAN
    p[:, :, cols:] = NAN
    got = gpu.op_appearance_score(a, p, cols)
    worst = 0.0
    for i in range(n):
        f = au.premise(a[i], p[i], cols)
        assert f >= 0.5, f"premise: va, vp are only {f} of Saa, Spp"
        want = au.score(a[i], p[i], cols)
        assert got["status"][i] == want["status"] == 1
        d = abs(float(got["similarity"][i]) - float(want["similarity"]))
        worst = max(worst, d)
        assert d <= au.sim_tolerance(nt * cols, 0.5, want["similarity"]), (i, got["similarity"][i], want["similarity"])
        g = au.gamma(nt * cols)
        ref = au.sums(a[i], p[i], cols)
        fa64, fp64 = au.bits_to_f64(a[i][:, :cols]), au.bits_to_f64(p[i][:, :cols])
        scale = [np.abs(fa64).sum(), np.abs(fp64).sum(), ref[2], ref[3], np.abs(fa64 * fp64).sum()]
        for k in range(5):      # both computations are within g * sum |x| of the exact sum
            assert abs(got["sums"][i][k] - ref[k]) <= 2 * g * scale[k], (i, k, got["sums"][i][k], ref[k])
    assert abs(float(got["similarity"][0])) > 0.9 and abs(float(got["similarity"][2])) < 0.05
    with capsys.disabled():
        print(f"\n[appearance op {shape}] max |sim - numpy| {worst:.3e}, bound {au.sim_bound(nt * cols, 0.5):.3e}")


def test_exact_value_cases(gpu):
    rng = np.random.default_rng(10)
    nt, cols, kpad = 16, 768, 768
    a = _ints(rng, 1, nt, cols, kpad)[0]
    small = _ints(rng, 1, nt, cols, kpad, -3, 4)[0]
    lin = _bits(2.0 * au.bits_to_f64(small).astype(np.float32) + 3.0)
    flat = np.full((nt, kpad), _bits([5.0])[0], np.uint16)
    A = np.stack([a, a, small, a, flat, flat])
    P = np.stack([a, a ^ np.uint16(0x8000), lin, flat, a, flat])
    got = gpu.op_appearance_score(A, P, cols)
    assert list(got["status"]) == [1, 1, 1, 3, 3, 3]
    assert list(got["similarity"]) == [1.0, -1.0, 1.0, 0.0, 0.0, 0.0]
    assert np.array_equal(got["sums"].view(np.uint64), _want(A, P, cols).view(np.uint64))


def test_two_runs_give_identical_bits(gpu):
    nt, cols, kpad = VITL14
    rng = np.random.default_rng(11)
    a, p = _bits(rng.standard_normal((33, nt, kpad))), _bits(rng.standard_normal((33, nt, kpad)))
    one, two = gpu.op_appearance_score(a, p, cols), gpu.op_appearance_score(a, p, cols)
    assert np.array_equal(one["sums"].view(np.uint64), two["sums"].view(np.uint64))
    assert np.array_equal(one["similarity"].view(np.uint32), two["similarity"].view(np.uint32))
    assert np.array_equal(one["status"], two["status"])


def test_bad_arguments(gpu):
    a = np.zeros((1, 4, 16), np.uint16)
    for kw in (dict(cols=0), dict(cols=17)):
        with pytest.raises(gpu.VtError) as ei:
            gpu.op_appearance_score(a, a, **kw)
        assert ei.value.code == -1
