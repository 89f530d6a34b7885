"""The per-model residual quantum on the GPU: the blob's lo_shift reaches every kernel that
writes or reads the 3-byte pair, the range report "xrange" says what a stream's residual holds, and a default blob runs
exactly as before. Every reference here is the specification restated in NumPy (lo_shift_util.split_pair) or the oracle
run at the same shift (lo_shift_util.oracle_lo_shift)."""
import struct

import numpy as np
import pytest

from lo_shift_util import (VITB_OUTLIER_CH, lo8_of, oracle_lo_shift, outlier_blob, pair_parts, split_pair, tiny_outlier_blob,
                           xrange_row)
from test_gpu_pipeline import TAP_BARS

pytestmark = pytest.mark.gpu

VT_ERR_INVALID_ARG, VT_ERR_FORMAT = -1, -4


def _bits(gpu, x):
    return gpu.weights.f32_to_bf16_bits(np.asarray(x, np.float32)).reshape(np.shape(x))


# ---- a. the encoder (and the decoder of the read-modify-write), value by value ------------------------------------------

@pytest.mark.parametrize("s", [8, 9, 14])
@pytest.mark.parametrize("cfg", [0, 2, 5, 8, 18])
def test_x_epilogues_encode_every_float_at_the_shift(gpu, cfg, s):
    """test_x_epilogues_encode_every_float_like_the_specification with its values rescaled to the shift's ranges (exact
    below R = 2^(15 - s), the one-quantum band R .. 2R, saturation beyond): zero operands, the bias is the value.
    Epilogue 1 also adds a c_init that is itself a representable pair at s: the decoder inside the read-modify-write."""
    rng = np.random.default_rng(1000 * s + cfg)
    M, N, K = 300, 768, 256
    Q, R = np.float32(2.0 ** -s), np.float32(2.0 ** (15 - s))
    r8 = R / np.float32(8.0)        # a binade well inside the exact range; its bf16 ulp is r8 / 128
    hand = np.array([r8, r8 + 3 * Q, r8 * (1 + 2.0 ** -8), r8 * (1 + 2.0 ** -8) + Q, -2.5 * r8 - 2.5 * Q, 2.5 * r8 + 3.5 * Q,
                     0.375 * Q, -0.5 * Q, 1.5 * Q, 0.0, -0.0, 2 * R - R / 256, -(2 * R - R / 256), R + R / 256,
                     R + R / 256 - Q / 4, 5 * R + R / 128, -(5 * R + R / 128), 125.04 * R, -3750.0 * R, 127.5 * Q, 128.5 * Q],
                    np.float32)
    ties = R + (np.arange(64, dtype=np.float32) * 2 + 1) * (R / np.float32(256.0))      # bf16 ties of the band R .. 2R
    bias = np.concatenate([hand, ties, -ties, (rng.normal(0, 0.08, 200) * R).astype(np.float32),
                           (rng.uniform(1, 2, 200) * R * rng.choice([-1, 1], 200)).astype(np.float32),
                           (rng.uniform(2, 40, 100) * R * rng.choice([-1, 1], 100)).astype(np.float32)])
    bias = np.concatenate([bias, (rng.uniform(-0.5, 0.5, N - len(bias)) * R).astype(np.float32)])
    za, zw = np.zeros((M, K), np.float32), np.zeros((N, K), np.float32)
    want = np.broadcast_to(split_pair(bias, s), (M, N))
    c_pair = split_pair((rng.uniform(-0.4, 0.4, (M, N)) * R).astype(np.float32), s)
    cases = ((0, None, want), (1, np.zeros((M, N), np.float32), want),
             (1, c_pair, split_pair((np.broadcast_to(bias, (M, N)) + c_pair).astype(np.float32), s)))
    for epi, c0, ref in cases:
        got = gpu.op_gemm_bf16(_bits(gpu, za), _bits(gpu, zw), bias, c_init=c0, epilogue=epi, cfg=cfg, lo_shift=s)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (epi, c0 is not None, bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])], bias[bad[0][1]])
    assert np.abs(want[0, :9] - hand[:9]).max() <= float(Q) / 2             # ordinary values: half a quantum


# ---- b. the readers: the final LayerNorm inside the band kernel and as its own launch -------------------------------------

@pytest.mark.parametrize("s", [8, 14])
def test_layernorm_readers_decode_the_pair_at_the_shift(gpu, s):
    rng = np.random.default_rng(s)
    D, N, grid, nt = 768, 128, 8, 80
    ntok = nt + grid * grid
    R = 2.0 ** (15 - s)
    x = (rng.normal(0, 0.2, (ntok, D)) * R).astype(np.float32)
    xh, lo8 = pair_parts(x, s)
    xs = split_pair(x, s).astype(np.float64)[nt:]
    g, b = rng.uniform(0.9, 1.1, D).astype(np.float32), rng.uniform(-0.02, 0.02, D).astype(np.float32)
    w = rng.uniform(-0.05, 0.05, (N, D)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, N).astype(np.float32)
    out = [gpu.op_headconv_ln(xh, lo8, g, b, _bits(gpu, w), bias, 1, grid, ntok, nt, fused=f, lo_shift=s) for f in (True, False)]
    assert np.array_equal(out[0], out[1]), "band kernel and stand-alone LayerNorm differ"
    mu = xs.mean(1, keepdims=True)
    ln = (xs - mu) / np.sqrt(xs.var(1, keepdims=True) + 1e-6) * g + b
    lnb = gpu.weights.bf16_bits_to_f32(_bits(gpu, ln)).reshape(ln.shape).astype(np.float64)
    wb = gpu.weights.bf16_bits_to_f32(_bits(gpu, w)).reshape(w.shape).astype(np.float64)
    ref = np.maximum(lnb @ wb.T + bias, 0)
    # the hook's existing bar (tests/test_gpu_ops.py): bf16 output + a bf16 flip of a normalised input here and there
    assert np.all(np.abs(out[0] - ref) <= np.abs(ref) * 2.0 ** -8 + 2e-2), np.abs(out[0] - ref).max()
    # a reader on the default quantum would be off by up to 127 (2^-s - 2^-12) per element: not the same rows at all
    wrong = gpu.op_headconv_ln(xh, lo8, g, b, _bits(gpu, w), bias, 1, grid, ntok, nt, fused=True, lo_shift=12 if s != 12 else 8)
    assert not np.array_equal(wrong, out[0])


# ---- c / e. model level on the tiny outlier blob, and the range report -----------------------------------------------------

# Layer taps against the oracle at the same shift. TAP_BARS cannot serve below s = 12: two implementations of one
# specification disagree by rounding flips of one quantum at each of the 2L + 1 stores, and the quantum is coarser. The
# bars are 2 x the distance measured on MI355X (profiles/lo_shift.txt), relative to the tensor's maximum:
#   tiny, outlier blob, s = 8, B = 1 and 8: worst layer tap 3.24e-5 of max (1.0 quantum)
LAYER_BAR_TINY_S8 = 6.5e-5
# independent of any measurement: no tap element further than 32 quanta of the shift from the oracle (a reader or writer
# on the wrong constant is off by up to 127 (2^-s - 2^-12), over 100 quanta, on most elements)
TAP_MAX_QUANTA = 32

def _frame(gpu):
    sc = gpu.synth.MovingSquare(640, 480, 64, seed=2)
    return sc.frame_nv12(0), sc.gt_box(0)


def _run(gpu, weights, B, taps=True, streams=None):
    buf, box = _frame(gpu)
    grp = gpu.Group(weights, n_streams=B)
    grp.enable_taps(taps)
    f = gpu.NV12Frame(buf, 640, 480)
    for i in range(B):
        grp.init_host(i, f, gpu.BBox.new(*box))
    if streams is None:
        grp.update_host([f] * B)
    else:
        grp.update_host([f] * len(streams), streams=streams)
    return grp


@pytest.fixture(scope="module")
def oracle_s8(gpu, oracle, tmp_path_factory):
    """the tiny outlier blob stamped s = 8 and the oracle's taps on the test frame at that shift (computed once)"""
    path = tiny_outlier_blob(tmp_path_factory.mktemp("lo") / "tiny_outliers_s8.vtw", lo_shift=8)
    buf, box = _frame(gpu)
    with oracle_lo_shift(8):
        ref = oracle.VitTrackRef(path)
        of = oracle.Frame.nv12(buf, 640, 480)
        ref.init(of, box)
        ref.update(of, taps=True)
    return path, ref.last


@pytest.mark.parametrize("B", [1, 8])
def test_tiny_outlier_model_at_shift_8(gpu, oracle_s8, B):
    path, orc = oracle_s8
    grp = _run(gpu, path, B)
    mi = grp.model_info()
    n, d, L = mi.tokens_template + mi.tokens_search, mi.dim, mi.layers
    bar_x, bar_feat, bar_head = TAP_BARS["tiny"]
    for i in sorted({0, B - 1}):
        taps = {k: grp.read_tensor(k, i).reshape(n, d) for k in ["tokens0"] + [f"layer{l}" for l in range(L)]}
        for k, x in taps.items():
            b = lo8_of(x, 8)
            assert np.all(b == np.rint(b)) and np.abs(b).max() <= 127, f"{k}: not a pair at shift 8"
        # tokens0: the same float32 value rounded to the pair - at most one quantum apart, on few elements
        d0 = np.abs(taps["tokens0"] - orc["tokens0"])
        assert d0.max() <= 2.0 ** -8 and (d0 > 0).mean() < 0.02, (d0.max(), (d0 > 0).mean())
        for l in range(L):
            dl = np.abs(taps[f"layer{l}"] - orc[f"layer{l}"])
            rel = dl.max() / np.abs(orc[f"layer{l}"]).max()
            print(f"[tiny s=8 B={B} stream {i}] layer{l}: max {dl.max() * 256:.1f} quanta, {rel:.2e} of max")
            # no reader or writer on another constant: that is > 100 quanta on most elements
            assert dl.max() <= TAP_MAX_QUANTA * 2.0 ** -8
            assert rel <= LAYER_BAR_TINY_S8, (l, rel)
        feat = grp.read_tensor("feat", i).reshape(mi.tokens_search, d)
        e_feat = np.abs(feat - orc["feat"]).max() / np.abs(orc["feat"]).max()
        ho = grp.read_tensor("head_out", i).reshape(mi.tokens_search, 8)
        e_head = np.abs(ho[:, :5] - orc["head_out"][:, :5]).max() / max(1.0, np.abs(orc["head_out"]).max())
        print(f"[tiny s=8 B={B} stream {i}] feat {e_feat:.2e} (bar {bar_feat:.0e}), head {e_head:.2e} (bar {bar_head:.0e})")
        assert e_feat < bar_feat and e_head < bar_head
        # e. the range report equals the NumPy statistics of the HIP path's own taps, exactly
        rows = grp.read_tensor("xrange", i).reshape(-1, 12)
        assert rows.shape[0] == L + 1
        for r, x in zip(rows, taps.values()):
            assert list(map(float, r)) == xrange_row(x, 8)
        assert all(r["n_sat"] == 0 for r in grp.residual_range(i))


# ---- d. the 256x256 kernel's X-epilogues inside the pass -------------------------------------------------------------------

#   cfg2, outlier blob, s = 9, 34 streams, streams 0 and 33: worst layer tap 8.15e-5 of max (5.0 quanta; the CPU
#   stand-in of two implementations one rounding flip apart gives 4.5e-3) - the bar is 2 x the measured value
LAYER_BAR_CFG2_S9 = 1.63e-4


def test_cfg2_34_streams_at_shift_9_on_the_256x256_kernels(gpu, oracle, tmp_path):
    """cfg2 at s = 9 with 34 streams: the smallest engine whose patch embedding, proj and fc2 take GEMM_CFG_256PP
    (34 * 320 rows -> 43 panels x 3 >= 128 tiles; 33 streams do not). Outlier blob, one update with taps, first and
    last stream against the oracle at s = 9; the range report against the HIP path's own taps."""
    S, B = 9, 34
    path = outlier_blob(tmp_path / "cfg2_outliers_s9.vtw", "cfg2", VITB_OUTLIER_CH, lo_shift=S)
    buf, box = _frame(gpu)
    with oracle_lo_shift(S):
        ref = oracle.VitTrackRef(path)
        of = oracle.Frame.nv12(buf, 640, 480)
        ref.init(of, box)
        ref.update(of, taps=True)
    orc = ref.last
    grp = _run(gpu, path, B)
    mi = grp.model_info()
    n, d, L = mi.tokens_template + mi.tokens_search, mi.dim, mi.layers
    assert n * B >= 43 * 256 - 255 and (n * B + 255) // 256 * 3 >= 128
    bar_x, bar_feat, bar_head = TAP_BARS["cfg2"]
    q = 2.0 ** -S
    for i in (0, B - 1):
        taps = {k: grp.read_tensor(k, i).reshape(n, d) for k in ["tokens0"] + [f"layer{l}" for l in range(L)]}
        for k, x in taps.items():
            b = lo8_of(x, S)
            assert np.all(b == np.rint(b)) and np.abs(b).max() <= 127, f"{k}: not a pair at shift {S}"
        d0 = np.abs(taps["tokens0"] - orc["tokens0"])
        assert d0.max() <= q and (d0 > 0).mean() < 0.02, (d0.max(), (d0 > 0).mean())
        worst_rel, worst_q = 0.0, 0.0
        for l in range(L):
            dl = np.abs(taps[f"layer{l}"] - orc[f"layer{l}"])
            worst_rel = max(worst_rel, float(dl.max() / np.abs(orc[f"layer{l}"]).max()))
            worst_q = max(worst_q, float(dl.max() / q))
        feat = grp.read_tensor("feat", i).reshape(mi.tokens_search, d)
        e_feat = np.abs(feat - orc["feat"]).max() / np.abs(orc["feat"]).max()
        ho = grp.read_tensor("head_out", i).reshape(mi.tokens_search, 8)
        e_head = np.abs(ho[:, :5] - orc["head_out"][:, :5]).max() / max(1.0, np.abs(orc["head_out"]).max())
        print(f"[cfg2 s=9 B={B} stream {i}] worst layer tap {worst_rel:.3e} of max, {worst_q:.1f} quanta "
              f"(bars {LAYER_BAR_CFG2_S9}, {TAP_MAX_QUANTA}); feat {e_feat:.2e} (bar {bar_feat:.0e}), head {e_head:.2e} "
              f"(bar {bar_head:.0e})")
        assert worst_q <= TAP_MAX_QUANTA
        assert worst_rel <= LAYER_BAR_CFG2_S9
        assert e_feat < bar_feat and e_head < bar_head
        rows = grp.read_tensor("xrange", i).reshape(-1, 12)
        assert rows.shape[0] == L + 1
        for r, x in zip(rows, taps.values()):
            assert list(map(float, r)) == xrange_row(x, S)


def test_xrange_tells_a_model_that_leaves_the_range(gpu, tmp_path):
    path = tiny_outlier_blob(tmp_path / "tiny_outliers.vtw")            # default shift
    grp = _run(gpu, path, 2)
    rr = grp.residual_range(1)
    assert [r["stage"] for r in rr] == ["tokens0", "layer0", "layer1"] and all(r["lo_shift"] == 12 for r in rr)
    assert sum(r["n_sat"] for r in rr) > 0 and max(r["max_abs"] for r in rr) > 100.0
    assert gpu.weights.recommend_lo_shift(rr) == 8
    assert gpu.weights.recommend_lo_shift(grp.read_tensor("xrange", 1).reshape(-1, 12)) == 8
    # with taps enabled the report needs a tapped pass: a fresh engine has none
    fresh = gpu.Group(path, n_streams=1)
    fresh.enable_taps(True)
    with pytest.raises(gpu.VtError) as ei:
        fresh.read_tensor("xrange", 0)
    assert ei.value.code == VT_ERR_INVALID_ARG
    # without taps: one row, the statistics of "x"
    grp.enable_taps(False)
    f = gpu.NV12Frame(_frame(gpu)[0], 640, 480)
    grp.update_host([f, f])
    row = grp.read_tensor("xrange", 0).reshape(-1, 12)
    assert row.shape == (1, 12) and list(map(float, row[0])) == xrange_row(grp.read_tensor("x", 0), 12)
    # the slot rules of the per-pass tensors after a subset pass
    grp.update_host([f], streams=[1])
    assert list(map(float, grp.read_tensor("xrange", 1)))  == xrange_row(grp.read_tensor("x", 1), 12)
    assert np.array_equal(grp.read_tensor("slot.xrange", 0), grp.read_tensor("xrange", 1))
    with pytest.raises(gpu.VtError) as ei:
        grp.read_tensor("xrange", 0)
    assert ei.value.code == VT_ERR_INVALID_ARG


# ---- f. nothing changes by default ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 8])
def test_slot_12_and_slot_0_are_the_same_engine(gpu, weights_tiny, tmp_path, B):
    p12 = tmp_path / "tiny_lo12.vtw"
    p12.write_bytes(open(weights_tiny, "rb").read())
    gpu.weights.set_lo_shift(str(p12), 12)
    sc = gpu.synth.MovingSquare(640, 480, 64, seed=4)
    grps = [gpu.Group(w, n_streams=B) for w in (weights_tiny, str(p12))]
    for g in grps:
        g.enable_taps(True)
    for t in range(5):
        f = gpu.NV12Frame(sc.frame_nv12(t), 640, 480)
        res = []
        for g in grps:
            if t == 0:
                for i in range(B):
                    g.init_host(i, f, gpu.BBox.new(*sc.gt_box(0)))
            res.append([(r.bbox, r.score, r.success) for r in g.update_host([f] * B)])
        assert res[0] == res[1]
        for i in sorted({0, B - 1}):
            for k in ("tokens0", "layer0", "layer1", "feat", "head_out", "state"):
                a, b = (g.read_tensor(k, i) for g in grps)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, i, k)


@pytest.mark.parametrize("slot", [5, 15, -1])
def test_bad_lo_shift_is_refused(gpu, weights_tiny, tmp_path, slot):
    import torch
    raw = bytearray(open(weights_tiny, "rb").read())
    struct.pack_into("<i", raw, 8 + 4 * 12, slot)
    p = tmp_path / "bad.vtw"
    p.write_bytes(raw)
    with pytest.raises(gpu.VtError) as ei:
        gpu.VitTrack(str(p))
    assert ei.value.code == VT_ERR_FORMAT and "lo_shift" in str(ei.value)
    blob = torch.from_numpy(np.frombuffer(bytes(raw), np.uint8).copy()).cuda()
    with pytest.raises(gpu.VtError) as ei:
        gpu.Group(n_streams=2, device_blob=(blob.data_ptr(), blob.numel()))
    assert ei.value.code == VT_ERR_FORMAT and "lo_shift" in str(ei.value)


# ---- g. closed loop at another shift --------------------------------------------------------------------------------------

def test_closed_loop_at_shift_9(gpu, oracle, tmp_path, monkeypatch):
    """tiny, s = 9, 20 frames of synth.MovingSquare: boxes within +-1 px of the oracle run at the same shift, same
    success flags"""
    monkeypatch.setenv("VT_WEIGHTS_DIR", str(tmp_path))
    weights = gpu.weights.ensure_weights("tiny", lo_shift=9)
    sc = gpu.synth.MovingSquare(640, 480, 64, seed=3)
    grp = gpu.Group(weights, n_streams=1)
    with oracle_lo_shift(9):
        ref = oracle.VitTrackRef(weights)
        for t in range(20):
            buf = sc.frame_nv12(t)
            f, of = gpu.NV12Frame(buf, 640, 480), oracle.Frame.nv12(buf, 640, 480)
            if t == 0:
                grp.init_host(0, f, gpu.BBox.new(*sc.gt_box(0)))
                ref.init(of, sc.gt_box(0))
            r, rr = grp.update_host([f])[0], ref.update(of)
            assert np.abs(np.array(r.bbox) - np.array(rr.bbox)).max() <= 1, (t, r.bbox, rr.bbox)
            assert bool(r.success) == bool(rr.success), t
    assert grp.residual_range(0)[0]["lo_shift"] == 9
