"""The per-model residual quantum on the CPU: the blob's lo_shift field, its helpers, and what the coarser quantum buys
on a model with outlier channels (oracle against the oracle with an un-quantised residual)."""
import hashlib
import struct

import numpy as np
import pytest

import gstreamer_vit_tracker_amd as vt
from lo_shift_util import oracle_lo_shift, split_pair, tiny_outlier_blob

W = vt.weights


@pytest.fixture(scope="module")
def tiny_tensors():
    cfg = W.get_config("tiny")
    return cfg, W.generate_tensors(cfg)


def _slot12(blob):
    return struct.unpack_from("<i", blob, 8 + 4 * 12)[0]


def test_default_blob_keeps_its_bytes(tiny_tensors, weights_tiny):
    cfg, t = tiny_tensors
    a, b = W.pack_blob(cfg, t), W.pack_blob(cfg, t, lo_shift=0)
    assert hashlib.sha256(a).digest() == hashlib.sha256(b).digest() and _slot12(a) == 0
    assert hashlib.sha256(open(weights_tiny, "rb").read()).digest() == hashlib.sha256(a).digest()
    assert W.parse_blob(a)[0]["lo_shift"] == 12


def test_lo_shift_round_trip_and_range(tiny_tensors):
    cfg, t = tiny_tensors
    base = W.pack_blob(cfg, t)
    for s in range(6, 15):
        blob = W.pack_blob(cfg, t, lo_shift=s)
        assert _slot12(blob) == s and W.parse_blob(blob)[0]["lo_shift"] == s
        diff = np.flatnonzero(np.frombuffer(blob, np.uint8) != np.frombuffer(base, np.uint8))
        assert list(diff) == [8 + 4 * 12], "only header int 12 may differ"
    for s in (5, 15, -1, 1):
        with pytest.raises(ValueError):
            W.pack_blob(cfg, t, lo_shift=s)


def test_set_lo_shift_and_cache_name(tiny_tensors, tmp_path, monkeypatch):
    cfg, t = tiny_tensors
    p = tmp_path / "a.vtw"
    p.write_bytes(W.pack_blob(cfg, t))
    W.set_lo_shift(str(p), 9)
    assert p.read_bytes() == W.pack_blob(cfg, t, lo_shift=9)
    W.set_lo_shift(str(p), 0)
    assert p.read_bytes() == W.pack_blob(cfg, t)
    with pytest.raises(ValueError):
        W.set_lo_shift(str(p), 15)
    (tmp_path / "junk").write_bytes(b"x" * 300)
    with pytest.raises(ValueError):
        W.set_lo_shift(str(tmp_path / "junk"), 9)
    monkeypatch.setenv("VT_WEIGHTS_DIR", str(tmp_path / "cache"))
    d, s9 = W.ensure_weights("tiny"), W.ensure_weights("tiny", lo_shift=9)
    assert d != s9 and W.parse_blob(open(s9, "rb").read())[0]["lo_shift"] == 9
    assert W.parse_blob(open(d, "rb").read())[0]["lo_shift"] == 12


def _row(s, max_abs, n_sat, reach):
    """an xrange row whose values reach 2^reach (n(|x| >= 2^k) > 0 for k <= reach)"""
    return [s, max_abs, n_sat] + [3 if k <= reach else 0 for k in range(1, 10)]


def test_recommend_lo_shift():
    assert W.recommend_lo_shift([_row(12, 3.4, 0, 1)]) == 12            # |x| < 4 < 8
    assert W.recommend_lo_shift([_row(12, 7.9, 0, 2)]) == 12
    assert W.recommend_lo_shift([_row(12, 8.0, 0, 3)]) == 11            # reaches 2^3: exact range must be 16
    assert W.recommend_lo_shift([_row(12, 3.0, 0, 1), _row(12, 120.0, 9, 6)]) == 8    # the worst stage decides
    assert W.recommend_lo_shift([_row(9, 300.0, 0, 8)]) == 6
    assert W.recommend_lo_shift([dict(lo_shift=12, max_abs=20.0, n_sat=1, n_ge_pow2=_row(0, 0, 0, 4)[3:])]) == 10
    with pytest.raises(ValueError):
        W.recommend_lo_shift([_row(12, 600.0, 0, 9)])
    with pytest.raises(ValueError):
        W.recommend_lo_shift([[1, 2, 3]])


def test_split_pair_ranges():
    """exact range, one-quantum band, saturation (never a wrap) at every shift"""
    rng = np.random.default_rng(5)
    for s in range(6, 15):
        q = 2.0 ** -s
        x = (rng.uniform(-1, 1, 20000) * 2.0 ** (15 - s)).astype(np.float32)
        assert np.abs(split_pair(x, s).astype(np.float64) - x).max() <= q / 2
        x = (rng.uniform(1, 2, 20000) * 2.0 ** (15 - s) * rng.choice([-1, 1], 20000)).astype(np.float32)
        assert np.abs(split_pair(x, s).astype(np.float64) - x).max() <= q
        x = (rng.uniform(2, 64, 20000) * 2.0 ** (15 - s) * rng.choice([-1, 1], 20000)).astype(np.float32)
        hi = W.bf16_bits_to_f32(W.f32_to_bf16_bits(x))
        assert np.all(np.abs(split_pair(x, s) - x) <= np.abs(hi - x))     # no worse than plain bf16


def test_coarser_quantum_is_closer_on_outlier_channels(tmp_path):
    """tiny model with outlier channels and offset rows: the oracle at s = 9 is at most half as far from the oracle
    with an un-quantised residual as the oracle at s = 12 (final features, rms)"""
    from oracle import vit_ref
    blob = tiny_outlier_blob(tmp_path / "tiny_outliers.vtw")
    m = vit_ref.Model(blob)
    rng = np.random.default_rng(11)
    patches = W.f32_to_bf16_bits(rng.normal(0, 1, (m.nt + m.ns, m.kpad)).astype(np.float32)).reshape(m.nt + m.ns, m.kpad)
    feats = {}
    for s in (None, 12, 9):
        with oracle_lo_shift(s):
            feats[s] = m.forward(patches)["feat"].astype(np.float64)
    d12 = np.sqrt(np.mean((feats[12] - feats[None]) ** 2))
    d9 = np.sqrt(np.mean((feats[9] - feats[None]) ** 2))
    print(f"\nfinal-feature rms distance to the un-quantised residual: s=12 {d12:.3e}, s=9 {d9:.3e} ({d9 / d12:.2f} x)")
    assert d9 <= 0.5 * d12
