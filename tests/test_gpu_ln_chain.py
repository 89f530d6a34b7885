"""The folded LayerNorm as the engine runs it (vt_op_ln_chain_bf16: X-epilogue statistics -> row terms by one of three
routes -> fold -> consuming epilogue) against a float64 reference of the float32 input, inside the per-element bound
derived in ln_chain_util.py (premises on the CPU: test_ln_chain_cases.py). Rows cycle through seven classes - N(0, 1), DC
of 30 and of 1000, constant, one outlier, chunk means that alternate, variance at the size of eps - so real row terms,
not integers, pass through every route, width and tile configuration."""
import numpy as np
import pytest

import ln_chain_util as lu

pytestmark = pytest.mark.gpu

INVALID_ARG = -1


def _params():
    return [(D, c, rt, cfg) for D, c, rt in lu.all_cases() for cfg in lu.consumer_cfgs(D, lu.shape(D, c, rt)[2], rt, c)]


def _run(gpu, D, consumer, route, cfg, pcfg=None, **kw):
    B, tokens, N = lu.shape(D, consumer, route)
    R = lu.reference(B * tokens, D, N, consumer)
    if pcfg is None:
        pcfg = 18 if route == 1 else -1         # the launcher's choice at 71 rows is a 4-wave configuration
    r = gpu.op_ln_chain_bf16(R.x, B, tokens, R.p.wb, R.p.gamma, R.p.beta, R.p.bias, consumer, route=route,
                             producer_cfg=pcfg, consumer_cfg=cfg, eps=lu.EPS, **kw)
    out = lu.qkv_natural(r["out"], r["vt"], B, tokens, D) if consumer == lu.QKV else r["out"]
    return R, r, out


def _untouched(a):
    return bool(np.all(a.view(np.uint8) == 0xff))


def _check_chain(R, r, out, route, what):
    # 1. the output, every element
    per_class = lu.worst_by_class(np.abs(out.astype(np.float64) - R.ref), R.bound, R.cls)
    print(f"ln_chain gpu {what}: out err/bound max {max(per_class.values()):.4f} "
          + " ".join(f"{k}={v:.3g}" for k, v in per_class.items()))
    assert lu.describe_worst(out, R.ref, R.bound, R.cls) is None, what + ": " + lu.describe_worst(out, R.ref, R.bound, R.cls)
    # 2. the row terms that routes 0 and 1 hand over; route 2 never writes the array
    rs = r["rowstat"]
    if route == 2:
        assert _untouched(rs)
    else:
        assert np.isfinite(rs).all(), what            # never a NaN from a negative M2
        e_r = np.abs(rs[:, 0].astype(np.float64) / R.rt.r - 1.0) / R.rt.E_r
        e_b = np.abs(rs[:, 1].astype(np.float64) - R.rt.nmr) / R.rt.E_b
        print(f"ln_chain gpu {what}: rstd err/bound {e_r.max():.4f} -mean*rstd err/bound {e_b.max():.4f}")
        assert e_r.max() <= 1.0, (what, int(e_r.argmax()), lu.CLASSES[R.cls[e_r.argmax()]], rs[e_r.argmax()])
        assert e_b.max() <= 1.0, (what, int(e_b.argmax()), lu.CLASSES[R.cls[e_b.argmax()]], rs[e_b.argmax()])
        d = R.cls == 3
        assert np.all(np.abs(rs[d, 0] * np.sqrt(lu.EPS) - 1.0) <= R.rt.E_r[d] + 1e-9)      # constant rows: eps^-1/2
    # 3. the chunk partials
    cs = lu.cstat_ref(R.x)
    s, q = r["cstat"][:, :, 0], r["cstat"][:, :, 1]
    assert np.all(np.abs(s - cs.S) <= cs.dS), what
    assert np.all(q >= 0) and np.all(np.abs(q - cs.Q) <= cs.dQ), what
    # 4. the stored pair
    hb, lo = lu.split_pair(R.x)
    assert np.array_equal(r["xh"], hb) and np.array_equal(r["xl"], lo), what
    # 5. the fold
    assert np.array_equal(r["wf"], R.fold.wfb), what
    assert np.all(np.abs(r["colsum"] - R.fold.colsum) <= R.fold.d_colsum), what
    assert np.all(np.abs(r["cvec"] - R.fold.cvec) <= R.fold.d_cvec), what


@pytest.mark.parametrize("D,consumer,route,cfg", _params())
def test_chain_within_the_derived_bound(gpu, D, consumer, route, cfg):
    R, r, out = _run(gpu, D, consumer, route, cfg)
    _check_chain(R, r, out, route, f"D={D} consumer={consumer} route={route} cfg={cfg}")


@pytest.mark.parametrize("D,pcfg", [(768, c) for c in (0, 1, 2, 3, 4, 5, 6, 7, 8, 18)] + [(2048, c) for c in (2, 3, 18)])
def test_every_producer_configuration(gpu, D, pcfg):
    """the statistics of every tile configuration that can write the pair, handed to the finalize launch (the engine's
    route when producer and consumer run on different kernels): the 256x256 producer without its own finalize too, at
    2048 columns the only way it runs"""
    R, r, out = _run(gpu, D, lu.RELU, 0, 2, pcfg=pcfg)
    _check_chain(R, r, out, 0, f"D={D} consumer={lu.RELU} route=0 producer={pcfg}")


@pytest.mark.parametrize("N,D", [(7, 128), (7, 192), (64, 192), (256, 384), (5, 2048)])
def test_fold_alone(gpu, N, D):
    """the fold at widths where every lane has one pair (128), where half the lanes sit out the second step (192), a
    ragged block of four waves (N = 7, 5) and the longest stride (2048)"""
    p = lu.make_params(N, D)
    f = lu.fold_ref(p)
    r = gpu.op_ln_chain_bf16(None, 0, 0, p.wb, p.gamma, p.beta, p.bias, 0, launches=2)
    assert np.array_equal(r["wf"], f.wfb)
    assert np.all(np.abs(r["colsum"] - f.colsum) <= f.d_colsum)
    assert np.all(np.abs(r["cvec"] - f.cvec) <= f.d_cvec)
    print(f"ln_chain gpu fold N={N} D={D}: colsum err/bound {(np.abs(r['colsum'] - f.colsum) / f.d_colsum).max():.4f} "
          f"cvec err/bound {(np.abs(r['cvec'] - f.cvec) / f.d_cvec).max():.4f}")


@pytest.mark.parametrize("D,consumer,route", [(D, c, rt) for D, c, rt in lu.all_cases() if c != lu.GELU])
def test_three_launches_give_the_bits_of_one(gpu, D, consumer, route):
    """the chain run three times on the same buffers: same bits everywhere; on route 1 the hook fails unless the panel
    counters are back at zero after every launch"""
    cfg = 18 if route == 1 and 18 in lu.consumer_cfgs(D, lu.shape(D, consumer, route)[2], route, consumer) else 2
    _, one, _ = _run(gpu, D, consumer, route, cfg, launches=1)
    _, three, _ = _run(gpu, D, consumer, route, cfg, launches=3)
    for k in ("out", "vt", "xh", "xl", "cstat", "rowstat", "wf", "colsum", "cvec"):
        assert np.array_equal(one[k].view(np.uint8), three[k].view(np.uint8)), k


@pytest.mark.parametrize("D,consumer", [(D, c) for D, c, rt in lu.all_cases() if rt == 2])
def test_route_2_against_route_0(gpu, D, consumer):
    """the consumer's own combination and the finalize launch sum in different orders: both inside the bound of the
    reference, not necessarily equal"""
    R, _, o0 = _run(gpu, D, consumer, 0, 2)
    _, _, o2 = _run(gpu, D, consumer, 2, 2)
    for o in (o0, o2):
        assert lu.describe_worst(o, R.ref, R.bound, R.cls) is None
    diff = np.abs(o0.astype(np.float64) - o2)
    print(f"ln_chain gpu route0-route2 D={D} consumer={consumer}: max |diff| {diff.max():.4g}, max diff/bound "
          f"{(diff / R.bound).max():.4f}, elements that differ {int((diff > 0).sum())} of {diff.size}")
    assert np.all(diff <= 2 * R.bound)


REFUSED = [
    # D, consumer, route, producer_cfg, consumer_cfg, B, tokens, N
    (256, lu.RELU, 1, 2, 2, 1, 71, 256),         # route 1 needs the 256x256 producer
    (384, lu.RELU, 1, 18, 2, 1, 71, 256),        # ... and D % 256 == 0
    (2048, lu.RELU, 1, 18, 2, 1, 71, 256),       # ... and D <= 1536
    (256, lu.RELU, 2, 2, 18, 1, 71, 256),        # route 2 is the 4-wave consumer's
    (192, lu.RELU, 2, 2, 2, 1, 71, 256),         # ... with D % 128 == 0
    (2048, lu.RELU, 2, 2, 2, 1, 71, 256),        # ... and D <= 1024
    (128, lu.QKV, 0, 2, 2, 3, 24, 256),          # QKV: N == 3 * D
    (128, lu.QKV, 0, 2, 2, 3, 22, 384),          # QKV: tokens % 4 == 0
]


@pytest.mark.parametrize("D,consumer,route,pcfg,ccfg,B,tokens,N", REFUSED)
def test_refusals_leave_the_outputs_alone(gpu, D, consumer, route, pcfg, ccfg, B, tokens, N):
    p = lu.make_params(N, D)
    x = lu.make_x(B * tokens, D)
    r = gpu.op_ln_chain_bf16(x, B, tokens, p.wb, p.gamma, p.beta, p.bias, consumer, route=route, producer_cfg=pcfg,
                             consumer_cfg=ccfg, check=False)
    assert r["rc"] == INVALID_ARG
    for k in ("out", "vt", "xh", "xl", "cstat", "rowstat", "wf", "colsum", "cvec"):
        assert _untouched(r[k]), k
