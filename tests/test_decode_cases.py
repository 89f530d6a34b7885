"""The decode tests' own tools, checked without a GPU: the exact-logit encoding, the float64 restatement of vto_decode
against vto_decode itself on the edge cases, and the case generators' tolerance and exclusion share (tests/decode_util.py,
from the reference alone). The GPU side is tests/test_gpu_decode.py."""
import itertools

import numpy as np
import pytest

import decode_util as du


def _sum_in_order(pieces, order, signs):
    acc = np.zeros_like(pieces[0])
    for j in order:
        acc = (acc + signs * pieces[j]).astype(np.float32)
    return acc


def test_three_piece_split_is_exact_under_every_summation_order():
    rng = np.random.default_rng(7)
    x = np.concatenate([
        (rng.standard_normal(4000) * 1.5).astype(np.float32),
        (rng.standard_normal(2000) * 10.0 ** rng.uniform(-24, 30, 2000)).astype(np.float32),
        # denormals and the normals just above them. A sum of bf16 values is a multiple of bf16's smallest denormal,
        # 2^-133: those are the float32 the encoding can carry down there (split3 refuses the others)
        (rng.integers(1, 1 << 7, 200).astype(np.uint32) << np.uint32(16)).view(np.float32),
        -(rng.integers(1, 1 << 7, 200).astype(np.uint32) << np.uint32(16)).view(np.float32),
        (rng.integers(1 << 7, 1 << 23, 500).astype(np.float64) * 2.0 ** -133).astype(np.float32),
        np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, np.finfo(np.float32).tiny, 2.0 ** -133, 0.0, -0.0,
                  1.0, 6.0, 30.0, -4.0, 0.5, 16777215.0, 1.0000001, 0.99999994], np.float32)]).astype(np.float32)
    with pytest.raises(AssertionError):
        du.split3(np.array([1.401298464e-45], np.float32))
    mag = np.abs(x)
    pieces = du.split3(mag)
    for p in pieces:        # bf16 values of the operand's sign: the low 16 bits are clear
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF)) and np.all(p >= 0)
    signs = np.where(np.signbit(x), np.float32(-1.0), np.float32(1.0))
    want = np.where(x == 0, np.float32(0.0), x)         # -0.0 comes back as +0.0 or -0.0: the same logit
    for order in itertools.permutations(range(3)):
        got = _sum_in_order(pieces, order, signs)
        assert np.array_equal(got, want), order
    # any subset sum is representable: pairs first (a tree reduction), in float32, equal to the float64 sum
    for a, b in itertools.combinations(range(3), 2):
        s32 = (pieces[a] + pieces[b]).astype(np.float32)
        assert np.array_equal(s32.astype(np.float64), pieces[a].astype(np.float64) + pieces[b].astype(np.float64))
        c = 3 - a - b
        assert np.array_equal((s32 + pieces[c]).astype(np.float32), mag)


def _emulate_logit_layer(t_bits, w4, order):
    """the 5-logit layer in NumPy float32 over the channels in `order`, pairwise (t0 * w0 + t1 * w1) like both kernels"""
    t = (t_bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    out = np.zeros((t.shape[0], 5), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in order:
            for k in range(5):
                pair = (t[:, c] * w4[k, c] + t[:, c + 1] * w4[k, c + 1]).astype(np.float32)
                out[:, k] = (out[:, k] + pair).astype(np.float32)
    return out


def test_encoding_reproduces_the_logits_finite_and_not():
    rng = np.random.default_rng(11)
    lg = (rng.standard_normal((300, 5)) * 1.5).astype(np.float32)
    lg[0] = [np.inf, -np.inf, np.nan, 0.0, 2.0 ** -133]
    lg[1] = [np.nan, np.nan, np.inf, 30.0, -4.0]
    lg[2] = np.finfo(np.float32).max
    for C in (64, 128):
        t, w4, b4 = du.encode(lg, C)
        assert t.shape == (300, C) and not np.any(t & 0x8000) and not b4.any()       # every piece >= 0: relu(t) = t
        assert np.all((t & 0x7F80) != 0x7F80)                                         # and finite
        assert not t[:, 30:].any() and not w4[:, 30:].any() and not w4[5:].any()
        pairs = list(range(0, C, 2))
        for order in (pairs, pairs[::-1], list(rng.permutation(pairs))):
            assert du.same_logits(_emulate_logit_layer(t, w4, order), lg)
    w3, b3 = du.identity_conv(64)
    w = (w3.astype(np.uint32) << np.uint32(16)).view(np.float32).reshape(64, 9, 64)
    assert np.array_equal(w[:, 4], np.eye(64, dtype=np.float32)) and w.sum() == 64 and not b3.any()


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_restatement_agrees_with_vto_decode_on_the_edge_cases(oracle, grid, C):
    """ties, threshold, clamps, non-finite logits: the same cell, the same integer box, the same success flag from the
    float32 specification and the float64 restatement (the generators assert the cells they aim at themselves)"""
    flat, real = du.ties(grid, C)
    sets = [flat, real, du.threshold_cases(grid, C, 0.5), du.threshold_cases(grid, C, du.THR_ABOVE_HALF),
            du.clamp_cases(grid, C), du.nonfinite_cases(grid, C)]
    for c in sets:
        assert c.tol == du.sweep(grid, C).tol and c.dist <= du.sweep(grid, C).dist      # one bar per shape, the largest distance
        assert np.array_equal(c.ora["idx"], c.f64["idx"])
        k = c.keep
        assert np.array_equal(c.ora["ibox"][k], c.f64["ibox"][k])
        assert np.array_equal(du.success_of(c.ora["score"], c.thr)[k], du.success_of(c.f64["score"], c.thr)[k])
        fin = np.isfinite(c.f64["score"])
        assert np.array_equal(np.isnan(c.ora["score"]), np.isnan(c.f64["score"]))
        assert np.abs(c.ora["score"][fin] - c.f64["score"][fin]).max() < 1e-6
    # at the threshold: >= succeeds, the next float32 above 0.5 fails
    assert np.all(du.success_of(sets[2].ora["score"], sets[2].thr) == 1)
    assert np.all(du.success_of(sets[3].ora["score"], sets[3].thr) == 0)
    # a failed update keeps box and success_count and writes the rest
    c = sets[3]
    st = du.expected_states(c.states, c.ora, c.thr)
    assert np.array_equal(st["box"], c.states["box"]) and np.array_equal(st["success_count"], c.states["success_count"])
    assert np.array_equal(st["frames_done"], c.states["frames_done"] + 1) and np.array_equal(st["last_idx"], c.ora["idx"])
    assert du.clamp_cases(grid, C).dropped == 0.0, "a hand-made clamp case sits on a rounding boundary: move it"


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_sweep_tolerance_and_exclusion_share(oracle, grid, C):
    """the sweep's bar comes from the reference alone (4 x the float32 specification's distance from float64), and the
    cases it excludes from the exact comparisons are at most 2 %; the clamp shares are asserted by the generator"""
    c = du.sweep(grid, C)
    print(du.report_line("every cell as the argmax", c), "clamp shares L/T/R/B", " ".join(f"{s:.2f}" for s in c.shares))
    assert c.n == grid * grid and 0.0 < c.tol < 0.01, c.tol          # px: far below what a wrong cell or weight moves
    assert c.dropped <= du.MAX_DROP_SHARE, c.dropped
    k = c.keep
    assert np.array_equal(c.ora["ibox"][k], c.f64["ibox"][k])
    assert np.array_equal(du.success_of(c.ora["score"], c.thr), du.success_of(c.f64["score"], c.thr))
    assert min(c.shares) >= du.MIN_CLAMP_SHARE
    # every word outside the decode's remit is recognisable: non-zero, so a kernel that zeroes it is seen
    for name in du.KEPT:
        assert np.all(c.states[name] != 0), name
