"""Helpers of the decode-stage tests (test_decode_cases.py, test_gpu_decode.py): exact float32 logits through the real
5-logit layer, the float64 restatement of vto_decode (oracle/vt_oracle.c), and the case generators.

Exact logits. A float32 x >= 0 is cut into three bf16 pieces by truncation, hi = top 8 significand bits of x, mid = top
8 bits of x - hi, lo = x - hi - mid (at most 8 bits are left): the pieces are disjoint bit fields of one 24-bit
significand, so the sum of ANY subset of them is exact in float32 and the kernels reproduce x whatever their summation
order. Logit k owns channels 6k .. 6k+5 = (hi, mid, lo) of max(x, 0) with w4 = +1 and (hi, mid, lo) of max(-x, 0) with
w4 = -1; every other channel and b4 are zero. For the band kernel the last 3x3 layer is the identity (centre tap, b3 = 0):
t3 = relu(t) = t since every piece is >= 0.
Non-finite logits cannot be carried by a non-finite piece (0 * inf in the other logits' rows), so they are made by
float32 overflow of FINITE pieces: +inf = two pieces of bf16 max on the positive channels 6k, 6k+1, -inf = two on the
negative channels 6k+4, 6k+5, NaN = both. Both kernels add an even-aligned channel pair first (t0 * w0 + t1 * w1), so
the pair overflows before it meets anything else: +inf, -inf, and (+inf) + (-inf) = NaN in every order.

Tolerance (the issue's rule): device expf is not glibc's, so score and float box are compared within TOL = 4 x the largest
distance between vto_decode (float32, glibc) and the float64 restatement over the shape's cases - measured from the
reference alone. Integer box and success are exact, but for cases whose float64 value lies within TOL of a rounding
boundary (x.5) or of the threshold: those are dropped here, deterministically, and at most 2 % of a sweep may be."""
import ctypes
import functools

import numpy as np

from gstreamer_vit_tracker_amd import weights as W
from gstreamer_vit_tracker_amd.snapshot import STATE

SHAPES = [(8, 64), (16, 128), (24, 128), (28, 128), (13, 64)]      # (grid, C): tiny, cfg2, cfg3, cfg5, short last band
FRAMES = [(640, 480), (1920, 1080), (3840, 2160)]
BF16_MAX = 0x7F7F
MAX_DROP_SHARE = 0.02
MIN_CLAMP_SHARE = 0.10
REMIT = ("box", "frames_done", "success_count", "last_idx", "last_fbox", "last_score")     # what the decode may write
KEPT = tuple(n for n in STATE.names if n not in REMIT)


def r_max(grid):
    """largest band height with R * grid <= 112 cells"""
    return min(grid, 112 // grid)


# ---- exact logits -----------------------------------------------------------------------------------------------

def split3(x):
    """float32 x >= 0 (finite) -> (hi, mid, lo) float32 arrays, each a bf16 value, hi + mid + lo == x exactly. Every normal
    >= 2^-110 splits, and below that the multiples of 2^-133 (bf16's smallest denormal): no sum of bf16 values is anything else."""
    x = np.ascontiguousarray(x, np.float32)
    assert np.all(np.isfinite(x)) and np.all(x >= 0)
    trunc = lambda v: (np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    hi = trunc(x)
    r1 = (x - hi).astype(np.float32)
    mid = trunc(r1)
    lo = (r1 - mid).astype(np.float32)
    assert np.array_equal(trunc(lo), lo), "bits below 2^-133, bf16's smallest denormal"
    return hi, mid, lo


def _bits(v):
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def encode(logits, C):
    """logits [n, 5] float32 (any value, non-finite included) -> (t bf16 bits [n, C], w4 [8, C], b4 [8])"""
    lg = np.ascontiguousarray(logits, np.float32)
    n = lg.shape[0]
    assert lg.shape == (n, 5) and C >= 30
    fin = np.isfinite(lg)
    v = np.where(fin, lg, np.float32(0.0)).astype(np.float32)
    t = np.zeros((n, C), np.uint16)
    for k in range(5):
        for j, piece in enumerate(split3(np.maximum(v[:, k], np.float32(0.0)))):
            t[:, 6 * k + j] = _bits(piece)
        for j, piece in enumerate(split3(np.maximum(-v[:, k], np.float32(0.0)))):
            t[:, 6 * k + 3 + j] = _bits(piece)
        pos = np.isnan(lg[:, k]) | (lg[:, k] == np.inf)
        neg = np.isnan(lg[:, k]) | (lg[:, k] == -np.inf)
        t[pos, 6 * k] = t[pos, 6 * k + 1] = BF16_MAX
        t[neg, 6 * k + 4] = t[neg, 6 * k + 5] = BF16_MAX
    w4 = np.zeros((8, C), np.float32)
    for k in range(5):
        w4[k, 6 * k:6 * k + 3] = 1.0
        w4[k, 6 * k + 3:6 * k + 6] = -1.0
    return t, w4, np.zeros(8, np.float32)


def identity_conv(C):
    """(w3 bf16 bits [C, 9C], b3 [C]) of the 3x3 layer that copies its input: 1.0 on the centre tap's own channel"""
    w3 = np.zeros((C, 9 * C), np.uint16)
    w3[np.arange(C), 4 * C + np.arange(C)] = 0x3F80
    return w3, np.zeros(C, np.float32)


def same_logits(got, want):
    """bit for bit, any NaN standing for any NaN (an overflow-made NaN carries the hardware's payload)"""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


# ---- the decode, twice ------------------------------------------------------------------------------------------------

def _sig64(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def decode_f64(logits, hann, grid, geo, fw, fh):
    """vto_decode restated in float64, vectorised over cases: logits [n, ns, 5], hann [ns], geo [n, 4], fw / fh [n] ->
    dict(idx, score, fbox [n, 4], ibox [n, 4], x1_raw, y1_raw, x2_raw, y2_raw). C's fmin / fmax (a NaN operand is ignored),
    first maximum in ascending cell order, a NaN response never compares greater."""
    lg = np.asarray(logits, np.float64)
    n, ns = lg.shape[0], grid * grid
    hann = np.asarray(hann, np.float64).reshape(ns)
    geo = np.asarray(geo, np.float64).reshape(n, 4)
    resp = _sig64(lg[:, :, 0]) * hann
    idx = np.argmax(np.where(np.isnan(resp) | (resp <= -1.0), -np.inf, resp), axis=1)
    rows = np.arange(n)
    score = _sig64(lg[rows, idx, 0])
    bx, by = idx % grid, idx // grid
    acc = np.zeros((5, n))
    with np.errstate(invalid="ignore", divide="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ix, iy = bx + dx, by + dy
                ok = (ix >= 0) & (iy >= 0) & (ix < grid) & (iy < grid)
                c = np.where(ok, iy * grid + ix, 0)
                o = lg[rows, c]
                w = (_sig64(o[:, 0]) * hann[c]) ** 2
                terms = [w, w * ((ix + (3.0 * _sig64(o[:, 1]) - 1.0)) / grid), w * ((iy + (3.0 * _sig64(o[:, 2]) - 1.0)) / grid),
                         w * _sig64(o[:, 3]), w * _sig64(o[:, 4])]
                for k in range(5):
                    acc[k] = np.where(ok, acc[k] + terms[k], acc[k])
        cxn, cyn, wn, hn = (acc[k] / acc[0] for k in (1, 2, 3, 4))
        side = geo[:, 3]
        cx, cy = (geo[:, 0] + 0.5) + cxn * side, (geo[:, 1] + 0.5) + cyn * side
        bw, bh = wn * side, hn * side
        x1r, y1r = cx - 0.5 * bw, cy - 0.5 * bh
        x2r, y2r = x1r + bw, y1r + bh
        Wf, Hf = np.asarray(fw, np.float64), np.asarray(fh, np.float64)
        x1 = np.fmin(np.fmax(0.0, x1r), Wf - 10.0)
        y1 = np.fmin(np.fmax(0.0, y1r), Hf - 10.0)
        x2 = np.fmin(np.fmax(10.0, x2r), Wf)
        y2 = np.fmin(np.fmax(10.0, y2r), Hf)
        bw, bh = np.fmax(10.0, x2 - x1), np.fmax(10.0, y2 - y1)
    fbox = np.stack([x1, y1, bw, bh], axis=1)
    return dict(idx=idx.astype(np.int64), score=score, fbox=fbox, ibox=np.floor(fbox + 0.5).astype(np.int64),
                x1_raw=x1r, y1_raw=y1r, x2_raw=x2r, y2_raw=y2r)


def decode_oracle(logits, hann, grid, geo, fw, fh):
    """vto_decode itself (float32, the specification), case by case -> dict(idx, score float32, fbox float32 [n, 4],
    ibox int32 [n, 4])"""
    from oracle import vit_ref
    L = vit_ref.lib()
    lg = np.ascontiguousarray(logits, np.float32)
    n, ns = lg.shape[0], grid * grid
    hann = np.ascontiguousarray(hann, np.float32).reshape(ns)
    geo = np.ascontiguousarray(geo, np.float32).reshape(n, 4)
    ho = np.zeros((ns, 8), np.float32)
    out, ib = np.zeros(6, np.float32), np.zeros(4, np.int32)
    res = dict(idx=np.zeros(n, np.int64), score=np.zeros(n, np.float32), fbox=np.zeros((n, 4), np.float32),
               ibox=np.zeros((n, 4), np.int32))
    for i in range(n):
        ho[:, :5] = lg[i]
        L.vto_decode(vit_ref._fp(ho), vit_ref._fp(hann), grid, vit_ref._fp(geo[i]), int(fw[i]), int(fh[i]), vit_ref._fp(out),
                     ib.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        res["idx"][i], res["score"][i], res["fbox"][i], res["ibox"][i] = int(out[5]), out[0], out[1:5], ib
    return res


def success_of(score, thr):
    """the success gate: float32 score >= float32 threshold, false for NaN"""
    return (np.asarray(score, np.float32) >= np.float32(thr)).astype(np.int32)


def distance(ora, f64):
    """largest |float32 specification - float64 restatement| over score and float box of the cases both decode to finite
    values (the argmax cell must agree for the comparison to mean anything: asserted)"""
    fin = np.isfinite(f64["score"]) & np.all(np.isfinite(f64["fbox"]), axis=1)
    assert np.array_equal(ora["idx"][fin], f64["idx"][fin])
    if not fin.any():
        return 0.0
    return float(max(np.abs(ora["score"][fin].astype(np.float64) - f64["score"][fin]).max(),
                     np.abs(ora["fbox"][fin].astype(np.float64) - f64["fbox"][fin]).max()))


def near_boundary(f64, thr, tol):
    """cases whose float64 box lies within tol of a rounding boundary x.5, or whose score within tol of the threshold"""
    v = f64["fbox"] + 0.5
    with np.errstate(invalid="ignore"):
        return (np.abs(v - np.rint(v)) <= tol).any(axis=1) | (np.abs(f64["score"] - float(np.float32(thr))) <= tol)


# ---- states -----------------------------------------------------------------------------------------------------

def make_states(geo, fw, fh, seed):
    """StreamState records whose words outside the decode's remit hold recognisable non-zero values"""
    n = len(fw)
    rng = np.random.default_rng(seed)
    st = np.zeros(n, STATE)
    i = np.arange(n)
    st["box"] = np.stack([11.0 + i, 22.0 + i, 33.0 + (i % 7), 44.0 + (i % 5)], axis=1)
    st["geo"] = np.asarray(geo, np.float32).reshape(n, 4)
    st["frame_w"], st["frame_h"] = fw, fh
    st["initialized"] = 1
    st["frames_done"] = rng.integers(1, 1000, n)
    st["success_count"] = (st["frames_done"] * rng.uniform(0.0, 1.0, n)).astype(np.int32)
    st["last_idx"] = 7
    st["last_fbox"] = np.stack([1.25 + i, 2.5 + i, 3.75 + 0 * i, 4.125 + 0 * i], axis=1)
    st["last_score"] = 0.123
    st["window_miss"] = 3 + (i % 11)
    st["tpl_gen"] = 5 + (i % 3)
    st["tpl_frame"] = 2 + (i % 13)
    return st


def expected_states(states, ora, thr, updates=1):
    """what `updates` decodes of the same logits leave in the records, from the specification's results"""
    st = states.copy()
    ok = success_of(ora["score"], thr).astype(bool)
    st["last_fbox"], st["last_score"], st["last_idx"] = ora["fbox"], ora["score"], ora["idx"]
    st["frames_done"] += updates
    st["success_count"] += updates * ok
    st["box"][ok] = ora["ibox"][ok].astype(np.float32)
    return st


def expected_results(ora, thr):
    from gstreamer_vit_tracker_amd import RESULT_DTYPE
    r = np.zeros(len(ora["idx"]), RESULT_DTYPE)
    r["success"], r["score"], r["bbox"] = success_of(ora["score"], thr), ora["score"], ora["ibox"]
    return r


def draw_geometry(n, rng):
    """crop geometry (x0m, y0m, scale, side) and frame sizes such that a good share of boxes leaves the frame on each of its
    four sides: the crop origin is drawn from a range that overhangs every edge by most of a side"""
    f = rng.integers(0, len(FRAMES), n)
    fw = np.array([FRAMES[k][0] for k in f], np.int32)
    fh = np.array([FRAMES[k][1] for k in f], np.int32)
    side = np.round(rng.uniform(64.0, np.minimum(1600.0, 1.2 * fw)) * 8) / 8
    x0 = np.round(rng.uniform(-0.8 * side, fw - 0.2 * side) * 8) / 8
    y0 = np.round(rng.uniform(-0.8 * side, fh - 0.2 * side) * 8) / 8
    x0, y0 = np.where(x0 == 0, 0.125, x0), np.where(y0 == 0, 0.125, y0)      # every word of geo recognisable: non-zero
    geo = np.stack([x0, y0, side / 256.0, side], axis=1).astype(np.float32)
    return geo, fw, fh


def clamp_shares(f64, fw, fh):
    """share of cases whose unclamped box crosses the frame's left, top, right, bottom edge"""
    return (float((f64["x1_raw"] < 0).mean()), float((f64["y1_raw"] < 0).mean()),
            float((f64["x2_raw"] > fw).mean()), float((f64["y2_raw"] > fh).mean()))


# ---- case sets: one stream per case, all streams of a set share Hann and threshold ------------------------------------

class Cases:
    """logits [n, ns, 5] float32, hann [ns] float32, states [n] STATE, thr; ora / f64: the two references; tol: the bar for
    score and float box; keep [n]: cases whose integer box and success are compared (the others lie within tol of a
    rounding boundary or of the threshold)"""

    def __init__(self, grid, C, logits, hann, states, thr, names=None, exact=False, tol=None):
        self.grid, self.C, self.ns, self.n = grid, C, grid * grid, len(states)
        self.logits = np.ascontiguousarray(logits, np.float32)
        assert self.logits.shape == (self.n, self.ns, 5)
        self.hann = np.ascontiguousarray(hann, np.float32).reshape(self.ns)
        self.states, self.thr = states, float(np.float32(thr))
        self.names = names or [str(i) for i in range(self.n)]
        geo, fw, fh = states["geo"], states["frame_w"], states["frame_h"]
        self.ora = decode_oracle(self.logits, self.hann, grid, geo, fw, fh)
        self.f64 = decode_f64(self.logits, self.hann, grid, geo, fw, fh)
        self.dist = distance(self.ora, self.f64)
        # the bar is the SHAPE's: the sweep measures it, every other set of the shape is handed it (their own distances are
        # smaller: test_decode_cases.py asserts that, so it is 4 x the largest distance over all the shape's cases)
        self.tol = 4.0 * self.dist if tol is None else tol
        # exact: a set whose outcome does not depend on expf (ties, threshold at logit 0): nothing is ever dropped
        self.keep = np.ones(self.n, bool) if exact else ~near_boundary(self.f64, self.thr, self.tol)
        self.dropped = float(1.0 - self.keep.mean())
        self.t, self.w4, self.b4 = None, None, None

    def operands(self):
        if self.t is None:
            self.t, self.w4, self.b4 = encode(self.logits.reshape(-1, 5), self.C)
        return self.t, self.w4, self.b4


def lifted_hann(grid):
    """The sweep's window: 0.5 + 0.5 * hann2d. With hann2d itself a border cell (1e-4 at a corner of grid 28) cannot be
    the argmax against cells drawn around sigmoid(-4) near the centre, and the borders are what the sweep is for; the
    lifted window keeps hann2d's shape (every cell's value differs from its neighbours') within [0.5, 1]. The tie,
    threshold and non-finite sets use hann2d itself."""
    return (np.float32(0.5) + np.float32(0.5) * W.hann2d(grid)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sweep(grid, C):
    """Every cell as the argmax: case i has random logits (normal, sigma 1.5, score logits lowered by 4 and capped at -1 so
    that cell i wins under the lifted window) with cell i's score logit raised to 6."""
    ns = grid * grid
    rng = np.random.default_rng(1000 + grid)
    lg = (rng.standard_normal((ns, ns, 5)) * 1.5).astype(np.float32)
    lg[:, :, 0] = np.minimum(lg[:, :, 0] - np.float32(4.0), np.float32(-1.0))
    lg[np.arange(ns), np.arange(ns), 0] = 6.0
    geo, fw, fh = draw_geometry(ns, rng)
    c = Cases(grid, C, lg, lifted_hann(grid), make_states(geo, fw, fh, 2000 + grid), 0.5)
    assert np.array_equal(c.ora["idx"], np.arange(ns)) and np.array_equal(c.f64["idx"], np.arange(ns))
    c.shares = clamp_shares(c.f64, fw, fh)
    assert min(c.shares) >= MIN_CLAMP_SHARE, c.shares
    return c


def _plain_states(n, seed, frame=(1920, 1080), geo=(700.0, 300.0, 1.5, 384.0)):
    return make_states(np.tile(np.array(geo, np.float32), (n, 1)), np.full(n, frame[0], np.int32),
                       np.full(n, frame[1], np.int32), seed)


def _background(n, ns, rng):
    lg = (rng.standard_normal((n, ns, 5)) * 1.5).astype(np.float32)
    lg[:, :, 0] = np.minimum(lg[:, :, 0] - np.float32(4.0), np.float32(-1.0))
    return lg


def tie_sets(grid):
    """name -> cells that share the largest score logit under a flat window. Bands at R = 1 are rows; `same stride` and
    `64 apart` are inside one band for R >= 2 (R * grid >= 66) and in neighbouring bands otherwise, which is the
    `different bands` case again."""
    ns = grid * grid
    sets = {"two in one stride": [grid + 1, grid + 3], "first and last": [0, ns - 1], "all": list(range(ns)),
            "different bands": [2 * grid - 1, ns - grid], "last cell alone": [ns - 1],
            "last cells of the last two rows": [ns - grid - 1, ns - 1]}
    if ns > 64 + 5:
        sets["64 apart"] = [5, 69]
    return sets


@functools.lru_cache(maxsize=None)
def ties(grid, C):
    """Flat window (all ones): the tie sets above with score logit 3 on the tying cells - any value would do, the
    responses are the same float32 whatever expf returns. Then hann2d with score logit 30 on every cell: sigmoid is
    exactly 1.0f (float32) and 1 - 9e-14 (float64) everywhere, the response is the window's value, and on an even
    grid the four central cells tie."""
    ns = grid * grid
    rng = np.random.default_rng(3000 + grid)
    sets = tie_sets(grid)
    lg = _background(len(sets), ns, rng)
    for i, cells in enumerate(sets.values()):
        lg[i, cells, 0] = 3.0
    flat = Cases(grid, C, lg, np.ones(ns, np.float32), _plain_states(len(sets), 3100 + grid), 0.5, list(sets), exact=True, tol=sweep(grid, C).tol)
    want = np.array([min(c) for c in sets.values()])
    assert np.array_equal(flat.ora["idx"], want) and np.array_equal(flat.f64["idx"], want)
    lg = _background(1, ns, rng)
    lg[:, :, 0] = 30.0
    real = Cases(grid, C, lg, W.hann2d(grid), _plain_states(1, 3200 + grid), 0.5, ["saturated"], exact=True, tol=sweep(grid, C).tol)
    centre = (grid // 2 - 1) * grid + grid // 2 - 1 if grid % 2 == 0 else (grid // 2) * grid + grid // 2
    assert real.ora["idx"][0] == centre == real.f64["idx"][0]
    return flat, real


THR_ABOVE_HALF = float(np.nextafter(np.float32(0.5), np.float32(1.0)))


@functools.lru_cache(maxsize=None)
def threshold_cases(grid, C, thr):
    """score logit exactly 0 on the winning cell: the score is exactly 0.5 in every arithmetic (expf(-0) = 1)"""
    ns = grid * grid
    rng = np.random.default_rng(4000 + grid)
    cells = [0, ns // 2 + 1, ns - 1]
    lg = _background(len(cells), ns, rng)
    lg[:, :, 0] -= np.float32(3.0)
    lg[np.arange(len(cells)), cells, 0] = 0.0
    c = Cases(grid, C, lg, np.ones(ns, np.float32), _plain_states(len(cells), 4100 + grid), thr, exact=True, tol=sweep(grid, C).tol)
    assert np.all(c.ora["score"] == np.float32(0.5)) and np.all(c.f64["score"] == 0.5)
    return c


CLAMP_GEOS = {      # name -> (x0m, y0m, side) on a 640 x 480 frame, cell (col, row) as a fraction of the grid, size logits
    "left": (-300.0, 100.0, 256.0), "top": (200.0, -300.0, 256.0), "right": (700.0, 100.0, 256.0),
    "bottom": (200.0, 540.0, 256.0), "top-left": (-400.0, -400.0, 256.0), "top-right": (720.0, -400.0, 256.0),
    "bottom-left": (-400.0, 560.0, 256.0), "bottom-right": (730.0, 560.0, 256.0),
    "straddles left": (-64.0, 100.0, 256.0), "straddles bottom": (200.0, 352.0, 256.0),
    "smaller than 10 px": (200.3125, 100.3125, 64.0), "larger than the frame": (-600.0, -500.0, 1600.0),
}


@functools.lru_cache(maxsize=None)
def clamp_cases(grid, C):
    """boxes pushed past each edge and corner, a predicted size below 10 px, a size larger than the frame"""
    ns = grid * grid
    rng = np.random.default_rng(5000 + grid)
    names = list(CLAMP_GEOS)
    lg = _background(len(names), ns, rng)
    cell = (grid // 2) * grid + grid // 2
    lg[:, cell, 0] = 6.0
    geo = np.array([[g[0], g[1], g[2] / 256.0, g[2]] for g in CLAMP_GEOS.values()], np.float32)
    k = names.index("smaller than 10 px")
    lg[k, :, 3:5] = -4.0            # sigmoid(-4) * 64 px = 1.2 px
    k = names.index("larger than the frame")
    lg[k, :, 3:5] = 4.0             # sigmoid(4) * 1600 px = 1571 px
    st = make_states(geo, np.full(len(names), 640, np.int32), np.full(len(names), 480, np.int32), 5100 + grid)
    c = Cases(grid, C, lg, lifted_hann(grid), st, 0.5, names, tol=sweep(grid, C).tol)
    f = c.f64
    assert f["x1_raw"][names.index("left")] < -10 and f["y1_raw"][names.index("top")] < -10
    assert f["x1_raw"][names.index("right")] > 640 and f["y1_raw"][names.index("bottom")] > 480
    assert np.all(f["fbox"][names.index("smaller than 10 px"), 2:] == 10.0)
    assert np.all(f["fbox"][names.index("larger than the frame")] == [0.0, 0.0, 640.0, 480.0])
    return c


NONFINITE = ("nan far from the window", "nan inside the window", "+inf on one cell", "-inf on the neighbours",
             "all -inf", "all nan", "nan on the first cells only", "nan x-offset inside the window")


@functools.lru_cache(maxsize=None)
def nonfinite_cases(grid, C):
    """Ordinary float arithmetic on non-finite logits, with hann2d. The expected values are vto_decode's, last_idx
    included: a NaN response never compares greater, and where nothing compares the decoded cell is 0."""
    ns = grid * grid
    rng = np.random.default_rng(6000 + grid)
    lg = _background(len(NONFINITE), ns, rng)
    mid = (grid // 2) * grid + grid // 2
    lg[:, mid, 0] = 6.0
    lg[0, 0, :] = np.nan                                # far from the window: ignored
    lg[1, mid + 1, 0] = np.nan                          # a window cell's weight is NaN: the box is (0, 0, 10, 10)
    lg[2, mid, 0] = np.inf                              # sigmoid(+inf) = 1
    lg[3, [mid - 1, mid + 1, mid - grid, mid + grid], 0] = -np.inf      # weight 0 in the window
    lg[4, :, 0] = -np.inf                               # every response 0: cell 0, sw = 0, box NaN -> (0, 0, 10, 10)
    lg[5, :, 0] = np.nan                                # nothing compares: cell 0
    lg[6, :ns // 2, 0] = np.nan                         # the first bands have no candidate, the later ones decide
    lg[7, mid + 1, 1] = np.nan                          # x is NaN -> (0, 10) by the clamp rules, y is an ordinary number
    c = Cases(grid, C, lg, W.hann2d(grid), _plain_states(len(NONFINITE), 6100 + grid), 0.5, list(NONFINITE), exact=True, tol=sweep(grid, C).tol)
    o = c.ora
    assert o["idx"][0] == mid and np.all(np.isfinite(o["fbox"][0]))
    assert np.array_equal(o["ibox"][1], [0, 0, 10, 10]) and o["score"][2] == 1.0
    assert o["idx"][4] == 0 and o["score"][4] == 0.0 and np.array_equal(o["ibox"][4], [0, 0, 10, 10])
    assert o["idx"][5] == 0 and np.isnan(o["score"][5]) and np.array_equal(o["ibox"][5], [0, 0, 10, 10])
    assert o["idx"][6] == mid and o["idx"][1] == mid and o["idx"][7] == mid
    assert o["ibox"][7][0] == 0 and o["ibox"][7][2] == 10 and o["ibox"][7][1] > 0 and o["ibox"][7][3] > 10
    for k in range(len(NONFINITE)):     # the float64 restatement agrees on all of it
        assert c.f64["idx"][k] == o["idx"][k] and np.array_equal(c.f64["ibox"][k], o["ibox"][k]), NONFINITE[k]
    return c


def report_line(name, c):
    return (f"{name:<28} grid {c.grid:>2} C {c.C:>3} cases {c.n:>4}  max |f32 spec - f64| {c.dist:.3e}  TOL {c.tol:.3e}  "
            f"dropped {100.0 * c.dropped:.2f} %")
