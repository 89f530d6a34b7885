"""The premises of test_gpu_epilogue_edges.py, proved without a GPU on the float64 reference, the oracle's integer rounding
and the float32 model of gelu_erf: the honest model lies inside the GELU interval at every input with a d_poly no larger
than the kernel's own claim, the slips the older tolerance (|ref| * 2^-8 + 2e-3) lets through are thrown out, the tie set
and the M list hold what the tests rely on, and the integer operands keep every sum exact."""
import numpy as np

import epilogue_util as eu
from gstreamer_vit_tracker_amd.weights import f32_to_bf16_bits


def test_gelu_model_is_inside_the_interval_and_d_poly_is_the_kernels_claim():
    y = eu.gelu_inputs()
    d_poly, at = eu.gelu_d_poly()
    lo, hi, ref, d = eu.gelu_interval(y)
    got = eu.bf16_round(eu.gelu_model(y))
    two = int((lo != hi).sum())
    print(f"epilogue GELU: d_poly = {d_poly:.4g} at y = {at:.6g} over {len(y)} inputs; {two} intervals admit two bf16 values, "
          f"{len(y) - two} one; model worst least-error / d = {(eu.least_error(got, ref) / d).max():.4f}")
    assert d_poly <= eu.GELU_POLY_CLAIM
    assert np.isfinite(got).all() and eu.inside(got, lo, hi).all()
    assert (lo <= hi).all() and np.array_equal(eu.bf16_round(lo), lo) and np.array_equal(eu.bf16_round(hi), hi)
    # the subnormal inputs: GELU(y) is y / 2 there, far inside d of zero
    s = eu.subnormal_inputs()
    lo, hi, _, _ = eu.gelu_interval(s)
    assert eu.inside(eu.bf16_round(eu.gelu_model(s)), lo, hi).all() and eu.inside(np.zeros(len(s), np.float32), lo, hi).all()


def test_gelu_mutants_are_rejected():
    """the tanh and the sigmoid form of GELU, truncation of the result and half-up rounding of it: each is outside the
    interval at thousands of inputs, while an erf of 3.3e-7 error (the Abramowitz-Stegun form the kernel had before: the
    reference displaced by that much) stays inside"""
    y = eu.gelu_inputs()
    lo, hi, ref, _ = eu.gelu_interval(y)
    out = lambda got: int((~eu.inside(got, lo, hi)).sum())
    n = dict(tanh=out(eu.bf16_round(eu.gelu_tanh(y))), sigmoid=out(eu.bf16_round(eu.gelu_sigmoid(y))),
             truncation=out(eu.bf16_truncate(eu.gelu_model(y))), half_up=out(eu.bf16_half_up(eu.gelu_model(y))),
             old_tolerance_tanh=int((np.abs(eu.bf16_round(eu.gelu_tanh(y)) - ref) > np.abs(ref) * 2.0 ** -8 + 2e-3).sum()))
    sign = np.where(np.arange(len(y)) & 1, 1.0, -1.0)
    n["erf_3.3e-7"] = out(eu.bf16_round((ref + 3.3e-7 * sign).astype(np.float32)))
    print("epilogue GELU mutants rejected at: " + ", ".join(f"{k} {v}" for k, v in n.items()) + f" of {len(y)} inputs")
    assert n["tanh"] > 10000 and n["sigmoid"] > 10000 and n["truncation"] > 10000
    assert n["old_tolerance_tanh"] == 0           # what the older tests would have said to the tanh form
    assert n["erf_3.3e-7"] == 0


def test_rounding_mutants_are_rejected_on_the_exact_sets():
    """ReLU, k and v must return the oracle's rounding bit for bit: truncation differs on every value above a middle and on
    the odd ties, half-up on the even ties only - the tie set is what catches it"""
    x = eu.rounding_inputs()
    want = eu.bf16_round(x)
    assert int((eu.bf16_truncate(x) != want).sum()) > 100000
    t = eu.tie_set()
    half_up = eu.bf16_half_up(t) != eu.bf16_round(t)
    u = eu.random_sets()[0]             # a random float32 is a tie once in 65,536: without the tie set half-up would pass
    assert half_up.sum() >= 2 * 2 * 200 and (eu.bf16_half_up(u) != eu.bf16_round(u)).sum() < 20
    q = eu.q_product(x)
    assert (np.abs(q[x != 0]) > 0).all()


def test_tie_set_holds_both_directions_at_every_exponent():
    t = eu.tie_set()
    u = t.view(np.uint32)
    tie = (u & 0xFFFF) == 0x8000
    expo = (u >> 23) & 0xFF
    odd = ((u >> 16) & 1) == 1
    down = tie & ~odd          # the even neighbour is below: rounds down
    up = tie & odd
    assert len(np.unique(expo[down])) >= 200 and len(np.unique(expo[up])) >= 200
    assert np.array_equal(f32_to_bf16_bits(t[down]), (u[down] >> 16).astype(np.uint16))
    assert np.array_equal(f32_to_bf16_bits(t[up]), ((u[up] >> 16) + 1).astype(np.uint16))
    for low in (0x7FFF, 0x8001):
        assert len(np.unique(expo[(u & 0xFFFF) == low])) >= 200
    assert np.isinf(eu.bf16_round(t)).sum() == 4          # +-: the tie and the value above it, at the top of the range
    assert len(eu.bf16_patterns()) == 2 * 254 * 128 + 2
    assert len(eu.rounding_inputs()) == len(eu.bf16_patterns()) + len(t) + 400000


def test_m_list_covers_every_tile_height():
    for bm in sorted(set(eu.TILE_ROWS.values())):
        assert {bm - 1, bm, bm + 1} <= set(eu.EDGE_M), bm
    assert {1, 2, 3} <= set(eu.EDGE_M) and max(eu.EDGE_M) > 256 + 128
    assert all(eu.qkv_config_fits(c, eu.EDGE_D) for c in eu.EDGE_CONFIGS)       # nothing to skip at D = 256
    assert all(t % 4 == 0 for t in eu.QKV_TOKENS)
    assert {60, 64, 68} <= set(eu.QKV_TOKENS) and {252, 256, 260} <= set(eu.QKV_TOKENS)


def test_integer_operands_are_exact_and_inside_the_pair():
    o = eu.edge_operands()
    K = o["a"].shape[1]
    assert np.abs(o["a"]).max() * np.abs(o["w"]).max() * K + 8 + 100 < 2 ** 24        # any partial sum, any order
    assert 3 * 16 * K + 2 * 5 + 8 < 2 ** 24                                           # with the folded row terms
    for x in (o["z"], o["z"] + o["c0"]):
        x32 = (x * float(eu.SC)).astype(np.float32)
        assert np.array_equal(x32.astype(np.float64), x * float(eu.SC))                # the scaled integers are float32 values
        assert np.array_equal(eu.split_pair_value(x32), x32)                          # ... and 3-byte pairs
    assert np.array_equal(o["zf"], np.rint(o["zf"])) and np.abs(o["zf"]).max() < 2 ** 24
    assert (np.asarray(o["z"] * float(eu.SC)).var(axis=1) > 100 * 1e-6).all()          # eps does not decide the row terms
