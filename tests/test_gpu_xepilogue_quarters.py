"""The X-epilogues of the 256x256 kernel (csrc/k_gemm256.hip) write a tile out in four double-buffered quarters of 64 rows:
quarter (i, h) holds the accumulator blocks mf = 2h, 2h+1 of rows i of both wave rows, i.e. tile rows

    wr * 128 + i * 64 + (2h + ml) * 16 + 0..15        (wr, ml = 0, 1)

and a wave writes four row pairs of it. The M values below put the end of the rows inside each quarter and inside each kind
of row pair: 2, 3 (first pair; the odd last row), 62, 64, 66 (the last pair of rows i = 0 / the first of rows i = 1 of wave
row 0), 127, 129 (the edge between the wave rows), 190, 194 (rows i = 0 / 1 of wave row 1), 255, 257 (the tile edge) and
258 + 64 (a second row panel that ends between rows i = 0 and rows i = 1).

Exact small integers (epilogue_util.edge_operands): whatever the order of accumulation, x is that integer * 2^-12, which the
3-byte pair holds exactly; the hooks' outputs start as 0xff bytes between guard bands, so a row no quarter stored is a NaN
and a store past row M an error. N = 256 / 768: one and three workgroups per row panel take a ticket on its counter;
K = 128 is the shortest main loop (two K-tiles) in front of the epilogue. Every launch runs twice and must return the same
bytes: the panel counters come back to zero and nothing depends on which workgroup arrives last."""
import numpy as np
import pytest

import epilogue_util as eu

pytestmark = pytest.mark.gpu

F = np.float32
SC = eu.SC
QUARTER_M = (2, 3, 62, 64, 66, 127, 129, 190, 194, 255, 257, 258 + 64)


def _bits(vt, x):
    return vt.weights.f32_to_bf16_bits(np.asarray(x, F))


def test_the_cases_put_the_edge_inside_every_quarter():
    """(not a GPU premise, but it belongs to the cases above) the last valid row of the last panel falls into each of the
    four quarters, into both wave rows, and M is odd at least once per wave row"""
    last = [(M - 1) % 256 for M in QUARTER_M]
    quarters = {(((r >> 6) & 1), ((r >> 5) & 1)) for r in last}          # (i, h) of tile row r
    assert quarters == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {r >> 7 for r in last} == {0, 1}
    assert {(M % 2, ((M - 1) % 256) >> 7) for M in QUARTER_M} >= {(1, 0), (1, 1), (0, 0), (0, 1)}


@pytest.mark.parametrize("N,K", [(256, 128), (256, 768), (768, 128), (768, 768)])
@pytest.mark.parametrize("epi", [0, 1, 4])
def test_quarter_edges_exact_and_repeatable(gpu, epi, N, K):
    """epilogues 0 (plain), 1 (+= the old pair) and 4 (+= positional rows) on configuration 18: finite, the exact integers,
    the row terms within the bounds of test_gpu_epilogue_edges.test_x_epilogues_at_every_tile_edge, and a second launch
    with the same bytes"""
    o = eu.edge_operands(rows=max(QUARTER_M), N=N, K=K)
    assert np.abs(o["z"]).max() + 100 < 2 ** 15          # inside the pair's exact range: |lo8| <= 64 at quantum 2^-12
    ab, wb, bias = _bits(gpu, o["a"]), _bits(gpu, o["w"] * SC), o["bias"] * SC
    for M in QUARTER_M:
        c0 = None if epi == 0 else o["c0"][:M] * SC
        want = ((o["z"][:M] + (0 if epi == 0 else o["c0"][:M])) * float(SC)).astype(F)
        got, rs = gpu.op_gemm_bf16(ab[:M], wb, bias, c_init=c0, epilogue=epi, cfg=18, want_rowstat=True)
        assert np.isfinite(got).all() and np.isfinite(rs).all(), (M, np.argwhere(~np.isfinite(got))[:4])
        assert np.array_equal(got, want), (M, np.argwhere(got != want)[:4])
        ref = eu.row_terms64(got)
        assert np.abs(rs[:, 0] / ref[:, 0] - 1).max() < 2e-5, (M, np.abs(rs[:, 0] / ref[:, 0] - 1).max())
        assert np.abs(rs[:, 1] - ref[:, 1]).max() < 2e-4 * np.abs(ref[:, 1]).max(), M
        got2, rs2 = gpu.op_gemm_bf16(ab[:M], wb, bias, c_init=c0, epilogue=epi, cfg=18, want_rowstat=True)
        assert got2.tobytes() == got.tobytes(), M
        assert rs2.tobytes() == rs.tobytes(), M


def test_remapped_addend_on_quarters(gpu):
    """the smallest shape of test_gpu_last_rows: seg_rows = 64, seg_skip = 16, 5 segments, M = 320, N = 256, K = 128 - a
    segment is one quarter of wave row 0 and crosses into wave row 1 and into the second panel. Exact integers: the pair is
    that of z + the addend's remapped row, the launch on the gathered rows gives the same bytes, and so does a second
    launch of each."""
    M, N, K, seg, skip = 320, 256, 128, 64, 16
    rows_in = (M // seg) * (seg + skip)
    o = eu.edge_operands(rows=rows_in, N=N, K=K)
    ab, wb, bias = _bits(gpu, o["a"][:M]), _bits(gpu, o["w"] * SC), o["bias"] * SC
    x_in = o["c0"] * SC                                   # integers * 2^-12 below 2^7 * 2^-12: hi + lo8 exactly
    hi = _bits(gpu, x_in)
    lo = np.rint((x_in - gpu.weights.bf16_bits_to_f32(hi)) * F(4096)).astype(np.int8)
    assert np.array_equal(gpu.weights.bf16_bits_to_f32(hi) + lo.astype(F) * SC, x_in)
    m = np.arange(M)
    src = m + (m // seg + 1) * skip
    want = ((o["z"][:M] + o["c0"][src]) * float(SC)).astype(F)
    remap = gpu.op_gemm_resid_seg(ab, wb, bias, hi, lo, M, seg_rows=seg, seg_skip=skip)
    plain = gpu.op_gemm_resid_seg(ab, wb, bias, hi[src], lo[src], M)
    x_out = gpu.weights.bf16_bits_to_f32(remap[0]) + remap[1].astype(F) * SC
    assert np.isfinite(x_out).all() and np.isfinite(remap[2]).all() and np.isfinite(remap[3]).all()
    assert np.array_equal(x_out, want), np.argwhere(x_out != want)[:4]
    ref = eu.row_terms64(x_out)
    assert np.abs(remap[3][:, 0] / ref[:, 0] - 1).max() < 2e-5
    assert np.abs(remap[3][:, 1] - ref[:, 1]).max() < 2e-4 * np.abs(ref[:, 1]).max()
    again = gpu.op_gemm_resid_seg(ab, wb, bias, hi, lo, M, seg_rows=seg, seg_skip=skip)
    plain_again = gpu.op_gemm_resid_seg(ab, wb, bias, hi[src], lo[src], M)
    for a, b, c, d, name in zip(remap, plain, again, plain_again, ("xh", "xl", "cstat", "rowstat")):
        assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes(), name
