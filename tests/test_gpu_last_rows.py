"""The last encoder block on the search rows only: behind the last attention nobody reads the
template rows, so an eligible pass computes the last block's attention output compactly (search queries only), reads
the residual addend of its proj through a row remap and runs fc1, fc2, the final LayerNorm and the head on n * ns rows.
The results are the bits of a pass over all rows ("last_rows" = 0): checked here on engines at the stream counts where
the compact proj just takes / just misses the 256x256 kernel, against a tapped engine, and on the two changed kernels
at operator level."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 640, 360
UPDATES = 3


def _frames(gpu, n, t):
    """stream i: scene i % 5 at time t + 7 * (i // 5) - every stream sees its own picture"""
    cache = _frames.cache
    out = []
    for i in range(n):
        key = (i % 5, t + 7 * (i // 5))
        if key not in cache:
            if key[0] not in _frames.scenes:
                _frames.scenes[key[0]] = gpu.synth.MovingSquare(W, H, 48, seed=900 + key[0])
            cache[key] = gpu.NV12Frame(_frames.scenes[key[0]].frame_nv12(key[1]), W, H)
        out.append(cache[key])
    return out


_frames.cache, _frames.scenes = {}, {}


def _track(gpu, weights, n, last_rows=None, taps=False, tensors=("feat", "head_out", "state")):
    """init + UPDATES updates of an n-stream engine; the results of every update and the named tensors of every stream
    after the last one (uint32 views: equality is equality of bits)"""
    g = gpu.Group(weights, n_streams=n)
    if last_rows is not None:
        g.set_tuning("last_rows", last_rows)
    if taps:
        g.enable_taps(True)
    f0 = _frames(gpu, n, 0)
    for i in range(n):
        sc = _frames.scenes[i % 5]
        g.init_host(i, f0[i], gpu.BBox.new(*sc.gt_box(7 * (i // 5))))
    res = []
    for t in range(1, UPDATES + 1):
        res.append([(r.success, r.score, tuple(r.bbox)) for r in g.update_host(_frames(gpu, n, t))])
    out = {"results": res, "rows": int(g.read_tensor("last_block_rows")[0])}
    for name in tensors:
        out[name] = [g.read_tensor(name, i).view(np.uint32).copy() for i in range(n)]
    return g, out


def _same(a, b, n, names=("feat", "head_out", "state")):
    assert a["results"] == b["results"]
    for name in names:
        for i in range(n):
            assert np.array_equal(a[name][i], b[name][i]), (name, i)


@pytest.fixture(scope="module")
def cfg3_19(gpu, weights_cfg3):
    """cfg3 x 19: 10,944 compact rows = 43 panels x 3 column tiles = 129 tiles, the smallest count at which the compact
    proj still takes the 256x256 kernel. nt = 144 is no multiple of 32, the 576-row segments straddle the 256-row
    panels and the last panel is part full."""
    g, d = _track(gpu, weights_cfg3, 19, tensors=("feat", "head_out", "state", "x", "attn"))
    d["x_again"] = g.read_tensor("x", 5).view(np.uint32).copy()        # the read puts the rows back: idempotent
    d["feat_again"] = g.read_tensor("feat", 5).view(np.uint32).copy()  # ... and leaves the compact pair readable
    return d


def test_cfg3_19_streams_equal_all_rows(gpu, weights_cfg3, cfg3_19):
    _, full = _track(gpu, weights_cfg3, 19, last_rows=0)
    assert cfg3_19["rows"] == 576 and full["rows"] == 720
    assert all(r[0] for r in cfg3_19["results"][-1])           # every stream tracks
    _same(cfg3_19, full, 19)
    assert np.array_equal(cfg3_19["x_again"], cfg3_19["x"][5]) and np.array_equal(cfg3_19["feat_again"], cfg3_19["feat"][5])


@pytest.mark.parametrize("n,rows", [(43, 256), (42, 320)])
def test_cfg2_threshold_between_the_two_kernels(gpu, weights_cfg2, n, rows):
    """cfg2 (ns = 256, ntok = 320): 43 streams = 43 panels x 3 = 129 tiles, compact; 42 = 126 tiles: the compact proj would
    run on the 4-wave kernel, which has no remap - the pass runs all rows as before"""
    _, a = _track(gpu, weights_cfg2, n)
    _, b = _track(gpu, weights_cfg2, n, last_rows=0)
    assert a["rows"] == rows and b["rows"] == 320
    _same(a, b, n)


def test_tapped_engine_runs_all_rows_and_agrees(gpu, weights_cfg3, cfg3_19):
    """taps copy whole-layout rows of every block: a tapped engine runs all rows. Its layer{L-1} search rows are the
    compact engine's "x" search rows, its layer{L-2} template rows the compact engine's "x" template rows (what block L-2
    left there); "attn" of the compact engine has zero template rows."""
    g, t = _track(gpu, weights_cfg3, 19, taps=True, tensors=("feat",))
    assert t["rows"] == 720 and t["results"] == cfg3_19["results"]
    mi = g.model_info()
    nt, ns, D, L = mi.tokens_template, mi.tokens_search, mi.dim, mi.layers
    for i in range(19):
        assert np.array_equal(t["feat"][i], cfg3_19["feat"][i]), i
        x = cfg3_19["x"][i].reshape(nt + ns, D)
        last = g.read_tensor(f"layer{L - 1}", i).view(np.uint32).reshape(nt + ns, D)
        prev = g.read_tensor(f"layer{L - 2}", i).view(np.uint32).reshape(nt + ns, D)
        assert np.array_equal(x[nt:], last[nt:]), i
        assert np.array_equal(x[:nt], prev[:nt]), i
        assert not np.array_equal(last[:nt], prev[:nt])         # the rows the compact pass did not compute do differ
        at = cfg3_19["attn"][i].reshape(nt + ns, D)
        assert not at[:nt].any() and at[nt:].any()


# ---- the attention kernel on search queries only -----------------------------------------------------------------

def _bits(gpu, x):
    return gpu.weights.f32_to_bf16_bits(np.asarray(x, np.float32))


def _rand_bf16(gpu, rng, shape, scale=1.0):
    b = _bits(gpu, rng.standard_normal(shape) * scale)
    return b, gpu.weights.bf16_bits_to_f32(b)


def _attn_ref(q, k, v, B, N, H):
    out = np.zeros((B * N, H * 64), np.float32)
    smax = 0.0
    for b in range(B):
        for h in range(H):
            sl, rows = slice(h * 64, (h + 1) * 64), slice(b * N, (b + 1) * N)
            s = q[rows, sl] @ k[rows, sl].T
            smax = max(smax, float(np.abs(s).max()))
            p = np.exp2(s - s.max(axis=1, keepdims=True))       # q arrives pre-scaled by log2(e)/8
            out[rows, sl] = (p @ v[rows, sl]) / p.sum(axis=1, keepdims=True)
    return out, smax


def _search_rows(a, B, N, q0):
    return a.reshape(B, N, -1)[:, q0:].reshape(B * (N - q0), -1)


@pytest.mark.parametrize("N,q0", [(80, 16), (320, 64), (720, 144), (980, 196)])
def test_attention_search_queries_equal_the_full_kernel(gpu, N, q0):
    """the model shapes (template / search tokens of tiny, cfg2, cfg3, cfg4), 2 streams, 2 heads, scores inside the
    +-32 window: the compact output is rows q0.. of the full kernel bit for bit - whichever 128-query group a query
    falls into, whether q0 is a multiple of 32 (64) or not (16, 144, 196), with a ragged last query block (980 - 196 =
    784 = 24.5 blocks) and with the half last key tile (80, 720: 16 keys; 980: 20)"""
    rng = np.random.default_rng(N)
    B, H = 2, 2
    qb, q = _rand_bf16(gpu, rng, (B * N, H * 64), 0.35)
    kb, k = _rand_bf16(gpu, rng, (B * N, H * 64))
    vb, v = _rand_bf16(gpu, rng, (B * N, H * 64))
    ref, smax = _attn_ref(q, k, v, B, N, H)
    assert smax < 30.0                                          # the premise: every score inside the window
    full = gpu.op_attention_bf16(qb, kb, vb, B, N, H, mode=3)
    got = gpu.op_attention_queries(qb, kb, vb, B, N, H, q0, N - q0)
    assert got.shape == (B * (N - q0), H * 64)
    assert np.array_equal(got.view(np.uint32), _search_rows(full, B, N, q0).view(np.uint32))
    assert np.abs(got - _search_rows(ref, B, N, q0)).max() < 0.02 * max(1.0, np.abs(ref).max())


def test_attention_search_queries_outside_the_window(gpu):
    """one search query whose scores reach far beyond +-60 log2 units: its workgroup's unchecked pass fails the row-sum
    test and the careful pass runs - for other queries than in the full kernel, whose groups are cut from token 0. Checked
    against float32 NumPy under the tolerance of test_gpu_ops.test_attention_late_maximum_rescale, not for equality."""
    rng = np.random.default_rng(5)
    B, N, H, q0 = 2, 320, 2, 64
    q = (rng.standard_normal((B * N, H * 64)) * 0.35).astype(np.float32)
    q[N + 200] *= 60.0                                          # stream 1, search query 136
    qb = _bits(gpu, q)
    q = gpu.weights.bf16_bits_to_f32(qb)
    kb, k = _rand_bf16(gpu, rng, (B * N, H * 64))
    vb, v = _rand_bf16(gpu, rng, (B * N, H * 64))
    ref, smax = _attn_ref(q, k, v, B, N, H)
    assert smax > 100.0
    got = gpu.op_attention_queries(qb, kb, vb, B, N, H, q0, N - q0)
    assert np.isfinite(got).all()
    err = np.abs(got - _search_rows(ref, B, N, q0))
    assert err.max() < 0.03 * max(1.0, np.abs(ref).max()), err.max()


# ---- the residual GEMM of the 256x256 kernel with the remapped addend read ---------------------------------------

def _pair(gpu, x, shift=12):
    """the stored pair of x (specification v3): hi = bf16(x), lo8 = clamp(rint((x - hi) * 2^s), +-127)"""
    hi = _bits(gpu, x)
    lo = np.clip(np.rint((x - gpu.weights.bf16_bits_to_f32(hi)) * np.float32(1 << shift)), -127, 127).astype(np.int8)
    return hi, lo


def test_x_epilogue_remapped_addend_equals_in_place_on_gathered_rows(gpu):
    """seg_rows = 64, seg_skip = 16, 5 segments: M = 320 (the second 256-row panel is part full, a segment crosses the
    panel edge), N = 256, K = 128. Output pair, chunk partials and row terms are the bits of the in-place launch on the
    gathered rows; with seg_rows = 0 the new entry is the launch vt_op_gemm_bf16_lo(epilogue 1, cfg 18) always ran."""
    rng = np.random.default_rng(11)
    M, N, K, seg, skip = 320, 256, 128, 64, 16
    rows_in = (M // seg) * (seg + skip)
    ab, _ = _rand_bf16(gpu, rng, (M, K))
    wb, _ = _rand_bf16(gpu, rng, (N, K), 0.08)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    x_in = (rng.standard_normal((rows_in, N)) * 1.5).astype(np.float32)
    hi, lo = _pair(gpu, x_in)
    m = np.arange(M)
    src = m + (m // seg + 1) * skip
    assert src.max() == rows_in - 1 and np.setdiff1d(np.arange(rows_in), src).size == 5 * skip
    remap = gpu.op_gemm_resid_seg(ab, wb, bias, hi, lo, M, seg_rows=seg, seg_skip=skip)
    plain = gpu.op_gemm_resid_seg(ab, wb, bias, hi[src], lo[src], M)
    for got, want, name in zip(remap, plain, ("xh", "xl", "cstat", "rowstat")):
        g_, w_ = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
        assert np.array_equal(g_, w_), name
    assert np.isfinite(plain[2]).all() and np.isfinite(plain[3]).all()
    # seg_rows = 0 is today's launch: the existing entry point on the same operands (the canonical pair of a float32
    # x decodes and re-encodes to itself)
    x_g = gpu.weights.bf16_bits_to_f32(hi[src]) + lo[src].astype(np.float32) * np.float32(2.0 ** -12)
    c, ro = gpu.op_gemm_bf16(ab, wb, bias, c_init=x_g, epilogue=1, cfg=18, want_rowstat=True)
    x_out = gpu.weights.bf16_bits_to_f32(plain[0]) + plain[1].astype(np.float32) * np.float32(2.0 ** -12)
    assert np.array_equal(c.view(np.uint32), x_out.view(np.uint32))
    assert np.array_equal(ro.view(np.uint32), plain[3].view(np.uint32))
    # and it is the right quantity: x = A W^T + bias + addend, to the pair's precision
    a = gpu.weights.bf16_bits_to_f32(ab)
    w = gpu.weights.bf16_bits_to_f32(wb)
    ref = a @ w.T + bias + x_g
    assert np.abs(x_out - ref).max() < 2.0 ** -12 + 1e-4 * np.abs(ref).max()


def test_remap_is_refused_where_no_kernel_has_it(gpu):
    """odd segments (a row pair would straddle two) and shapes the 256x256 kernel does not take are errors, never a
    quiet run on another kernel"""
    rng = np.random.default_rng(3)
    ab, _ = _rand_bf16(gpu, rng, (64, 128))
    hi, lo = _pair(gpu, rng.standard_normal((128, 256)).astype(np.float32))
    wb, _ = _rand_bf16(gpu, rng, (256, 128), 0.08)
    with pytest.raises(gpu.VtError):
        gpu.op_gemm_resid_seg(ab, wb, None, hi, lo, 64, seg_rows=31, seg_skip=2)
    with pytest.raises(gpu.VtError):      # the addend read would leave the input pair
        gpu.op_gemm_resid_seg(ab, wb, None, hi, lo, 64, seg_rows=16, seg_skip=32)
