"""The premises of test_gpu_ln_chain.py, proved on the float64 reference and a float32 NumPy model of the folded LayerNorm
chain alone (no GPU): at every shape and consumer of the GPU test the honest model lies inside the derived bound of
ln_chain_util.py at every element, and the slips the older operator tests let through - row terms of the neighbouring row,
half of a row's chunks, a dropped eps, a float32 E[x^2] - mean^2 - are thrown out by it."""
import numpy as np
import pytest

import ln_chain_util as lu


def _cpu_shapes():
    seen = []
    for D, consumer, route in lu.all_cases():
        B, tokens, N = lu.shape(D, consumer, route)
        s = (B * tokens, D, N, consumer)
        if s not in seen:
            seen.append(s)
    return seen


def _checks(m, R):
    """err / bound of the three things the GPU test compares: out per element, rstd and -mean * rstd per row"""
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.abs(m.out.astype(np.float64) - R.ref) / R.bound
        rstd = np.abs(m.rowstat[:, 0].astype(np.float64) / R.rt.r - 1.0) / R.rt.E_r
        nmr = np.abs(m.rowstat[:, 1].astype(np.float64) - R.rt.nmr) / R.rt.E_b
    inf = lambda a: np.where(np.isfinite(a), a, np.inf)
    return inf(out), inf(rstd), inf(nmr)


def _fmt(d):
    return " ".join(f"{k}={v:.3g}" for k, v in d.items())


@pytest.mark.parametrize("M,D,N,consumer", _cpu_shapes())
def test_honest_model_is_inside_the_bound(M, D, N, consumer):
    """sequential float32 sums are one of the orders the bound allows: every output element, every row term and every
    chunk partial of the model lies inside. Largest err / bound per class printed; the outputs come close to 1 (the bf16
    rounding of the result is most of the bound on well-conditioned rows), the row terms stay far below (a worst case
    over all orders against one benign order)."""
    R = lu.reference(M, D, N, consumer)
    m = lu.model_chain(M, D, N, consumer)
    out, rstd, nmr = _checks(m, R)
    per_class = lu.worst_by_class(np.abs(m.out.astype(np.float64) - R.ref), R.bound, R.cls)
    print(f"ln_chain model M={M} D={D} N={N} consumer={consumer}: out err/bound {_fmt(per_class)}; "
          f"rstd {rstd.max():.3g} -mean*rstd {nmr.max():.3g}")
    assert out.max() <= 1.0, lu.describe_worst(m.out, R.ref, R.bound, R.cls)
    assert rstd.max() <= 1.0 and nmr.max() <= 1.0
    assert max(per_class.values()) > 0.5                # tight where the rounding of the result dominates, not generous
    cs = lu.cstat_ref(R.x)
    assert np.all(np.abs(m.cstat[:, :, 0] - cs.S) <= cs.dS) and np.all(np.abs(m.cstat[:, :, 1] - cs.Q) <= cs.dQ)
    assert np.all(m.cstat[:, :, 1] >= 0)
    d = R.cls == 3                                       # the constant rows: rstd is eps^-1/2 within its bound
    assert np.all(np.abs(m.rowstat[d, 0] * np.sqrt(lu.EPS) - 1.0) <= R.rt.E_r[d] + 1e-9)


@pytest.mark.parametrize("M,D,N,consumer", _cpu_shapes())
def test_mutations_are_rejected(M, D, N, consumer):
    """1 (neighbouring row's terms): every pair of rows (m, m ^ 1) - always of two classes - is rejected on the outputs, on
    both of its rows unless one is constant (class d: rstd = 1000 makes its own bound wide; its partner is thrown out by
    that same 1000). 2 (half of the chunks): rejected on the outputs. 3 (no eps): every row of classes d and g is
    rejected on the outputs. 4 (float32 E[x^2] - mean^2): most rows of class c are rejected on their row terms - what routes 0
    and 1 hand back - and at some shapes on the outputs too: there the any-order accumulation terms of a row at 1000 are of
    the size of the damage (ratios printed). 5 (column sums before the rounding of the weights) is reported only."""
    R = lu.reference(M, D, N, consumer)
    cls = R.cls
    res = {mut: _checks(lu.model_chain(M, D, N, consumer, mutation=mut), R) for mut in lu.MUTATIONS}
    row_out = {mut: r[0].max(axis=1) for mut, r in res.items()}
    print(f"ln_chain mutations M={M} D={D} N={N} consumer={consumer}: " + "; ".join(
        f"{mut}: out {_fmt({lu.CLASSES[c]: row_out[mut][cls == c].max() for c in range(7)})} rstd {res[mut][1].max():.3g}"
        for mut in lu.MUTATIONS))
    paired = (np.arange(M) ^ 1) < M
    assert np.all(cls[paired] != cls[np.arange(M)[paired] ^ 1])
    nb = row_out["neighbour_row"]
    idx = np.arange(M)[paired]
    assert np.all(np.maximum(nb[idx], nb[idx ^ 1]) > 1.0)                    # every pair ...
    assert np.all(nb[idx][cls[idx] != 3] > 1.0)                              # ... and every row of it but the constant ones
    assert row_out["half_chunks"].max() > 1.0
    assert np.all(row_out["half_chunks"][np.isin(cls, (0, 1, 4, 5, 6))] > 1.0)
    assert np.all(row_out["no_eps"][np.isin(cls, (3, 6))] > 1.0)
    assert (res["naive_variance"][1][cls == 2] > 1.0).mean() >= 0.5         # a float32 accident may leave a row inside
    assert row_out["no_eps"][np.isin(cls, (0, 1, 4, 5))].max() <= 1.0       # where eps does not matter nothing is rejected


def test_bf16_rounding_needs_its_full_unit_roundoff():
    """rounding to 8 significand bits moves a value just above a tie by 2^-8 of itself: a bound built on 2^-9 would throw
    out the honest model"""
    R = lu.reference(71, 768, 256, lu.RELU)
    m = lu.model_chain(71, 768, 256, lu.RELU)
    err = np.abs(m.out.astype(np.float64) - R.ref)
    assert (err > R.dy + 2.0 ** -9 * (R.ref + R.dy)).any()
    assert (err <= R.bound).all()


def test_shapes_cover_the_table():
    cases = lu.all_cases()
    assert {D for D, _, _ in cases} == {128, 256, 384, 768, 1024, 2048}
    assert {rt for D, _, rt in cases if D == 2048} == {0} and {rt for D, _, rt in cases if D == 128} == {0, 2}
    for D, consumer, route in cases:
        B, tokens, N = lu.shape(D, consumer, route)
        M = B * tokens
        assert M % 7 != 0 and M % 64 != 0 and (consumer == lu.QKV or M % 2 == 1) and (consumer != lu.QKV or tokens % 4 == 0)
        assert (M > 256) == (route == 1)
        cfgs = lu.consumer_cfgs(D, N, route, consumer)
        assert (18 in cfgs) == (route != 2 and N % 256 == 0 and (consumer != lu.QKV or D % 256 == 0))
