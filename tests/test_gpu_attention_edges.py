"""The attention kernels (modes 0-3 and the query-subset kernel) at their key boundaries: exact answers on selector data
that stay inside the window of mode 3's unchecked first pass, and a derived per-element bound against a float64 reference
on random, diffuse and off-window data (attention_util.py; premises in test_attention_cases.py). The operator hooks hand
back NaN for a row the kernel never stored and an error for a store just outside the output."""
import numpy as np
import pytest

import attention_util as au

pytestmark = pytest.mark.gpu


# ---- A. exact selector -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,H,mode", [s + (m,) for s in au.SELECTOR_SHAPES + au.SELECTOR_SHAPES_ANY_N for m in (0, 1, 2, 3)
                                        if m < 3 or s[1] % 4 == 0])      # mode 3 takes multiples of 4: 33, 97 are for modes 0-2
def test_selector_is_exact_for_every_key(gpu, B, N, H, mode):
    """every key is the answer of one query per (stream, head): out == V[sel] bit for bit. Matching score 56 log2 units:
    mode 3 answers from its first pass, the half step included where tokens & 63 is in 1..32 (16, 68, 80, 96, 720, 980)."""
    c = au.selector_case(B, N, H)
    got = gpu.op_attention_bf16(c.qb, c.kb, c.vb, B, N, H, mode=mode)
    assert np.isfinite(got).all()
    bad = np.argwhere(got != c.want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (row, column) {bad[0]}: {got[tuple(bad[0])]} != {c.want[tuple(bad[0])]}"
    again = gpu.op_attention_bf16(c.qb, c.kb, c.vb, B, N, H, mode=mode)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))          # run-to-run identical


@pytest.mark.parametrize("B,N,H", au.SELECTOR_SHAPES)
def test_selector_query_subsets_are_exact(gpu, B, N, H):
    """the subset kernel on the same data, for query ranges at both ends, off every block boundary and the search rows of
    the model shapes: exact, and the rows of the full kernel"""
    c = au.selector_case(B, N, H)
    full = gpu.op_attention_bf16(c.qb, c.kb, c.vb, B, N, H, mode=3)
    for q0, nq in au.subset_ranges(N):
        got = gpu.op_attention_queries(c.qb, c.kb, c.vb, B, N, H, q0, nq)
        assert got.shape == (B * nq, H * 64)
        assert np.isfinite(got).all(), (q0, nq)
        assert np.array_equal(got, au.query_rows(c.want, B, N, q0, nq)), (q0, nq)
        assert np.array_equal(got.view(np.uint32), au.query_rows(full, B, N, q0, nq).view(np.uint32)), (q0, nq)
        again = gpu.op_attention_queries(c.qb, c.kb, c.vb, B, N, H, q0, nq)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), (q0, nq)


# ---- B. derived bound on random data -----------------------------------------------------------------------------

# the shapes of test_gpu_ops.test_attention and test_attention_mode3 (same data), then the diffuse cases
RANDOM_SHAPES = [(1, 80, 2, 1.0), (2, 320, 12, 1.0), (1, 720, 12, 1.0), (1, 980, 16, 0.5), (1, 33, 1, 3.0), (3, 100, 2, 1.0),
                 (3, 96, 2, 1.0), (1, 16, 1, 3.0), (2, 1008, 4, 0.5), (5, 720, 12, 2.0), (2, 980, 16, 0.5), (1, 36, 1, 2.0),
                 (2, 980, 4, 0.5), (2, 720, 3, 0.5)]
DIFFUSE_EXTRA = (3, 100, 2, 0.5)


def _within_bound(got, ref, bound, what):
    assert np.isfinite(got).all(), what
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    print(f"attention_bound {what} max(err/bound) = {ratio.max():.4f}")
    over = np.argwhere(ratio > 1.0)
    assert over.size == 0, f"{what}: {len(over)} elements over the bound, worst ratio {ratio.max():.4f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"


@pytest.mark.parametrize("B,N,H,scale,mode", [s + (m,) for s in RANDOM_SHAPES + [DIFFUSE_EXTRA] for m in (0, 1, 2, 3)
                                              if m < 3 or s[1] % 4 == 0])
def test_random_data_within_the_derived_bound(gpu, B, N, H, scale, mode):
    """|got - ref| <= bound at every element (bound: attention_util.attention_ref64), no share left out"""
    c = au.random_case(B, N, H, scale)
    got = gpu.op_attention_bf16(c.qb, c.kb, c.vb, B, N, H, mode=mode)
    _within_bound(got, c.ref, c.bound, f"mode={mode} B={B} N={N} H={H} scale={scale}")


@pytest.mark.parametrize("B,N,H,scale", [s for s in RANDOM_SHAPES + [DIFFUSE_EXTRA] if s[1] % 4 == 0])
def test_random_data_query_subset_within_the_derived_bound(gpu, B, N, H, scale):
    """the subset kernel on the search rows (model shapes) or on a range that starts off every block boundary"""
    c = au.random_case(B, N, H, scale)
    q0 = au.MODEL_TEMPLATE_TOKENS.get(N, N // 5 + 1)
    got = gpu.op_attention_queries(c.qb, c.kb, c.vb, B, N, H, q0, N - q0)
    _within_bound(got, au.query_rows(c.ref, B, N, q0, N - q0), au.query_rows(c.bound, B, N, q0, N - q0),
                  f"mode=subset B={B} N={N} H={H} scale={scale}")


# ---- C. off-window levels on ragged token counts -----------------------------------------------------------------

@pytest.mark.parametrize("mode", [2, 3])
@pytest.mark.parametrize("level", au.OFFSET_LEVELS)
@pytest.mark.parametrize("N", [16, 36, 80, 100])
def test_offset_scores_on_a_partly_masked_tile(gpu, N, level, mode):
    """every score near `level` with a last (or only) tile that is partly padding, stream 1 starting off a tile boundary:
    mode 3's careful pass shifts its reference in a step that holds -inf entries (-64, -150, +90) and the first pass keeps
    rows far outside the careful pass's window (-50, +55). Finite, and inside the derived bound."""
    c = au.offset_case(2, N, level)
    got = gpu.op_attention_bf16(c.qb, c.kb, c.vb, 2, N, 1, mode=mode)
    _within_bound(got, c.ref, c.bound, f"mode={mode} offset level={level} N={N}")
