"""The appearance score restated (tests/appearance_util.py): exact-value cases, the premise of its error bound, mutation
checks, and the signal on the committed fixture (tests/golden/appearance_tiny.npz, tests/golden/make_appearance.py). No GPU:
tests/test_gpu_appearance_op.py holds the kernel to this restatement."""
import importlib.util
import os

import numpy as np
import pytest

import appearance_util as au

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(HERE, "golden", "appearance_tiny.npz")))


@pytest.fixture(scope="module")
def mk():
    spec = importlib.util.spec_from_file_location("_make_appearance", os.path.join(HERE, "golden", "make_appearance.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _bits(x):
    return au.f32_to_bf16_bits(np.asarray(x, np.float32))


def _ints(rng, nt, cols, kpad, lo=-16, hi=17):
    """integer-valued bf16 rows (exact) with NaN bit patterns in every pad column"""
    v = np.full((nt, kpad), 0x7FC0, np.uint16)
    v[:, :cols] = _bits(rng.integers(lo, hi, size=(nt, cols)).astype(np.float32))
    return v


def test_exact_values():
    rng = np.random.default_rng(1)
    a = _ints(rng, 16, 768, 768)
    one = au.score(a, a, 768)
    assert one["status"] == 1 and one["similarity"] == np.float32(1.0) and one["similarity"].dtype == np.float32
    neg = a.copy()
    neg ^= np.uint16(0x8000)                            # p = -a (the sign bit of every element; -0 stays a zero)
    r = au.score(a, neg, 768)
    assert r["status"] == 1 and r["similarity"] == np.float32(-1.0)
    small = _ints(rng, 16, 768, 768, -3, 4)
    lin = _bits(2.0 * au.bits_to_f64(small).astype(np.float32) + 3.0)       # p = 2a + 3, exact in bf16 on |a| <= 3
    assert np.array_equal(au.bits_to_f64(lin), 2.0 * au.bits_to_f64(small) + 3.0)
    r = au.score(small, lin, 768)
    assert r["status"] == 1 and r["similarity"] == np.float32(1.0)


def test_flat_rows_give_status_3():
    rng = np.random.default_rng(2)
    a = _ints(rng, 4, 48, 64)
    flat = np.full((4, 64), _bits([5.0])[0], np.uint16)
    for x, y in ((a, flat), (flat, a), (flat, flat)):
        r = au.score(x, y, 48)
        assert r["status"] == 3 and r["similarity"] == np.float32(0.0)


def test_pad_columns_are_not_read():
    rng = np.random.default_rng(3)
    a, p = _ints(rng, 16, 588, 592), _ints(rng, 16, 588, 592)
    want = au.score(a, p, 588)
    a2, p2 = a.copy(), p.copy()
    a2[:, 588:] = _bits([7.0])[0]
    p2[:, 588:] = 0
    got = au.score(a2, p2, 588)
    assert np.array_equal(want["sums"], got["sums"]) and want["similarity"] == got["similarity"]
    assert np.isfinite(want["sums"]).all()


def test_integer_sums_are_exact_in_any_order():
    rng = np.random.default_rng(4)
    a, p = _ints(rng, 196, 588, 592), _ints(rng, 196, 588, 592)
    want = au.sums(a, p, 588)
    fa, fp = au.bits_to_f64(a[:, :588]).reshape(-1), au.bits_to_f64(p[:, :588]).reshape(-1)
    perm = rng.permutation(fa.size)
    loop = [float(np.cumsum(v[perm])[-1]) for v in (fa, fp, fa * fa, fp * fp, fa * fp)]     # a serial order, shuffled
    assert np.array_equal(want, np.array(loop))
    assert np.all(want == np.round(want)) and np.abs(want).max() < 2.0 ** 53


def test_dropping_an_element_moves_the_result_beyond_the_bound():
    rng = np.random.default_rng(5)
    nt, cols = 16, 768
    a = _bits(rng.standard_normal((nt, cols)))
    p = _bits(au.bits_to_f64(a) * 0.8 + 0.6 * rng.standard_normal((nt, cols)))
    f = au.premise(a, p, cols)
    assert f >= 0.5, f"premise: va, vp are only {f} of Saa, Spp"
    tol = au.sim_tolerance(nt * cols, 0.5, 1.0)
    full = au.score(a, p, cols)
    assert full["status"] == 1 and 0.5 < full["similarity"] < 0.95
    s_row = au.sums(a[:-1], p[:-1], cols)
    sim_row, _ = au.finish(s_row, (nt - 1) * cols)
    assert abs(float(sim_row) - float(full["similarity"])) > tol, "dropping the last row is not visible"
    fa, fp = au.bits_to_f64(a[:, :cols]).reshape(-1)[:-1], au.bits_to_f64(p[:, :cols]).reshape(-1)[:-1]
    s_el = np.array([fa.sum(), fp.sum(), (fa * fa).sum(), (fp * fp).sum(), (fa * fp).sum()])
    assert np.all(np.abs(s_el - full["sums"])[2:4] > 0), "dropping the last element is not visible in the sums"
    d = np.abs(s_el - full["sums"])
    for k, ref in enumerate((np.abs(fa).sum(), np.abs(fp).sum(), full["sums"][2], full["sums"][3], np.abs(fa * fp).sum())):
        assert d[k] > au.gamma(nt * cols) * ref, f"sum {k}: dropping the last element stays inside the summation bound"


def test_bound_is_small_against_binary32():
    # at the largest shape in use (ViT-L/14: 196 rows of 588) and a premise of 1 % the bound is below a binary32 ulp at 1
    assert au.sim_bound(196 * 588, 0.01) < 2.0 ** -24


def test_rule8_gates_on_top_of_the_refresh_rule():
    class R:
        def __init__(self, ok=True, score=0.9, bbox=(100, 100, 40, 40)):
            self.success, self.score, self.bbox = ok, score, bbox

    pre = np.array([100, 100, 40, 40], np.float32)
    rule = au.Rule(64, 128, 2, 0.0, 900)
    assert rule.tau == np.float32(900) / np.float32(1000)
    assert rule.step(R(), pre_box=pre, record=(1, 0.99)) is None                      # update 1: period not reached
    assert rule.step(R(), pre_box=pre, record=(1, 0.5)) == "gate"                     # due, too dissimilar
    assert rule.step(R(), pre_box=pre, record=(3, 1.0)) == "gate"                     # due again, a flat probe
    assert rule.step(R(), pre_box=pre, record=(1, float(rule.tau))) == "fire"         # similarity == tau passes
    assert (rule.generation, rule.last_frame, rule.gated) == (1, 4, [2, 3])
    assert rule.step(R(), pre_box=pre, record=(1, 0.0)) is None
    assert rule.step(R(ok=False), pre_box=pre, record=(0, 0.0)) is None               # a failed update is not gated: rule 3
    off = au.Rule(64, 128, 2, 0.0, 0)                                                  # tau 0: the refresh rule alone
    assert [off.step(R(), pre_box=pre, record=(1, -1.0)) for _ in range(4)] == [None, "fire", None, "fire"]


def test_signal_on_the_committed_fixture(fx, mk):
    """the table of the signal as inequalities: the same target stays near 1, a shifted box and a blended target fall
    monotonically, an absent target is uncorrelated"""
    cols = int(fx["cols"])
    anchor = fx["anchor"]

    def sim(rows):
        r = au.score(anchor, rows, cols)
        assert r["status"] == 1
        return float(r["similarity"])

    assert au.score(anchor, anchor, cols)["similarity"] == np.float32(1.0)
    assert fx["same_sim"].min() > 0.97 and fx["same_sim"].max() <= 1.0
    assert abs(sim(fx["same_last_rows"]) - fx["same_sim"][-1]) < 1e-7
    offs = [sim(r) for r in fx["offset_rows"]]
    assert np.allclose(offs, fx["offset_sim"], atol=1e-7)
    assert 1.0 > offs[0] > offs[1] > offs[2] > offs[3]
    assert offs[0] > 0.95 and 0.92 < offs[1] < 0.96 and 0.85 < offs[2] < 0.91 and 0.74 < offs[3] < 0.81
    blends = [sim(r) for r in fx["blend_rows"]]
    assert np.allclose(blends, fx["blend_sim"], atol=1e-7)
    assert 1.0 > blends[0] > blends[1] > blends[2] > blends[3]
    assert blends[0] > 0.97 and blends[3] < 0.88
    assert abs(sim(fx["absent_rows"])) < 0.1 and abs(float(fx["absent_sim"])) < 0.1
    assert fx["same_sim"].min() > max(offs[1], blends[2]), "the same target scores below a 2-px shift or a 75 % blend"


def test_gate_clip_conditions_hold_on_the_committed_fixture(fx, mk):
    mk.check(fx)
    assert int(fx["gate_pm"]) == mk.GATE_PM and int(fx["period"]) == mk.PERIOD and int(fx["n_updates"]) == mk.N_UPDATES
    imp = fx["gate_impostor"] != 0
    assert imp.sum() == 18 and [bool(mk.impostor_at(i)) for i in range(1, mk.N_UPDATES + 1)] == list(imp)
    assert fx["gate_sim"][imp].max() < 0.89 and fx["gate_sim"][~imp].min() > 0.91
