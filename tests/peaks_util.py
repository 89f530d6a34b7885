"""Helpers of the response-peaks tests (test_response_peaks_cases.py, test_gpu_response_peaks.py): the reference iteration
and the case sets.

The definition (include/vittrack_hip.h, "response peaks"): vto_decode iterated. Peak k is the decode of the logits with the
SCORE logit of every cell within `radius` (Chebyshev) of an earlier peak set to -inf; peak 0 is always listed, a later one
while resp = score * hann[cell] is > 0 and >= min_resp. `iterate` runs that through a decode of the caller's choice:
du.decode_oracle (vto_decode itself, float32: the specification) or du.decode_f64 (its float64 restatement).

Device expf is not glibc's (a few ulp), so no compared set may let rounding pick a cell or end a list: `margins` measures,
in float64, (1) at every listed round the relative distance between the chosen cell's response and the best other
unsuppressed one, and (2) the relative distance from min_resp of the last listed response and of the response that ended the
list. Both must be >= MARGIN = 1e-3, four orders above the rounding at stake. Sets whose outcome depends on no expf (ties
under a flat window, logit 0, all-NaN) are compared exactly and carry exact=True.

Tolerance: du.sweep(grid, C).tol, the shape's existing bar (4 x the largest float32 - float64 distance of the decode sweep,
measured from the reference alone). Every peaks set's own float32 - float64 distance must stay below a quarter of it
(test_response_peaks_cases.py)."""
import functools

import numpy as np

import decode_util as du

MARGIN = 1e-3
KMAX = 8
MIN_RESP = 0.35         # between du._background (score logits <= -1: responses <= sigmoid(-1) = 0.2689) and every planted response (>= 0.42)
DIRS = [(1, 0), (0, 1), (1, 1), (-1, 0), (0, -1), (-1, -1), (1, -1), (-1, 1)]


def iterate(decode, logits, hann, grid, geo, fw, fh, K, R, min_resp, f64=False):
    """the reference iteration through `decode`, vectorised over the cases -> dict(n [cases], cell [cases, K] (-1 behind
    the list), score, resp [cases, K], fbox [cases, K, 4]) in the decode's precision"""
    lg = np.array(logits, np.float64 if f64 else np.float32)
    n, ns = lg.shape[0], grid * grid
    ft = np.float64 if f64 else np.float32
    hann = np.asarray(hann, ft).reshape(ns)
    out = dict(n=np.zeros(n, np.int64), cell=np.full((n, K), -1, np.int64), score=np.zeros((n, K), ft),
               resp=np.zeros((n, K), ft), fbox=np.zeros((n, K, 4), ft))
    alive = np.ones(n, bool)
    xs, ys = np.arange(ns) % grid, np.arange(ns) // grid
    for k in range(K):
        if not alive.any():
            break
        idx = np.flatnonzero(alive)
        d = decode(lg[idx], hann, grid, np.asarray(geo)[idx], np.asarray(fw)[idx], np.asarray(fh)[idx])
        cell = np.asarray(d["idx"], np.int64)
        score = np.asarray(d["score"], ft)
        resp = (score * hann[cell]).astype(ft)              # one multiply in the decode's precision
        with np.errstate(invalid="ignore"):
            ok = (resp > 0) & (resp >= ft(min_resp)) if k >= 1 else np.ones(len(idx), bool)
        for j, i in enumerate(idx):
            if not ok[j]:
                alive[i] = False
                continue
            out["n"][i] = k + 1
            out["cell"][i, k], out["score"][i, k], out["resp"][i, k] = cell[j], score[j], resp[j]
            out["fbox"][i, k] = d["fbox"][j]
            sq = (np.abs(xs - cell[j] % grid) <= R) & (np.abs(ys - cell[j] // grid) <= R)
            lg[i, sq, 0] = -np.inf
    return out


def iterate_oracle(logits, hann, grid, geo, fw, fh, K, R, min_resp):
    return iterate(du.decode_oracle, logits, hann, grid, geo, fw, fh, K, R, min_resp)


def iterate_f64(logits, hann, grid, geo, fw, fh, K, R, min_resp):
    return iterate(du.decode_f64, logits, hann, grid, geo, fw, fh, K, R, min_resp, f64=True)


def margins(logits, hann, grid, K, R, min_resp):
    """float64, on the response plane alone -> (per case: the smallest relative lead of a listed peak over the best other
    unsuppressed cell, the smallest relative distance from min_resp of the last listed response (k >= 1) and of the response
    that ended the list). inf where there is nothing to measure. NaN responses never compete (they are never chosen)."""
    lg = np.asarray(logits, np.float64)
    n, ns = lg.shape[0], grid * grid
    with np.errstate(over="ignore"):
        plane = 1.0 / (1.0 + np.exp(-lg[:, :, 0])) * np.asarray(hann, np.float64).reshape(ns)
    plane = np.where(np.isnan(plane), -1.0, plane)
    lead, thr = np.full(n, np.inf), np.full(n, np.inf)
    xs, ys = np.arange(ns) % grid, np.arange(ns) // grid
    for i in range(n):
        p = plane[i].copy()
        for k in range(K):
            order = np.argsort(-p, kind="stable")
            c, r1, r2 = order[0], p[order[0]], p[order[1]] if ns > 1 else -1.0
            if k >= 1:
                if min_resp > 0:
                    thr[i] = min(thr[i], abs(r1 - min_resp) / min_resp)
                if not (r1 > 0 and r1 >= min_resp):
                    break
            if r1 > 0:
                lead[i] = min(lead[i], (r1 - max(r2, 0.0)) / r1)
            p[(np.abs(xs - c % grid) <= R) & (np.abs(ys - c // grid) <= R)] = 0.0
    return lead, thr


class PeakSet:
    """logits [n, ns, 5], hann [ns], states [n] (one stream per case), policy (K, R, min_resp) -> the two references, the
    set's own float32 - float64 distance, the shape's bar, the cases compared through the bar (float64 boxes finite)"""

    def __init__(self, name, grid, C, logits, hann, states, K, R, min_resp, exact=False):
        self.name, self.grid, self.C, self.ns, self.n = name, grid, C, grid * grid, len(states)
        self.logits = np.ascontiguousarray(logits, np.float32)
        assert self.logits.shape == (self.n, self.ns, 5)
        self.hann = np.ascontiguousarray(hann, np.float32).reshape(self.ns)
        self.states, self.K, self.R, self.min_resp, self.exact = states, K, R, float(np.float32(min_resp)), exact
        geo, fw, fh = states["geo"], states["frame_w"], states["frame_h"]
        self.ora = iterate_oracle(self.logits, self.hann, grid, geo, fw, fh, K, R, self.min_resp)
        self.f64 = iterate_f64(self.logits, self.hann, grid, geo, fw, fh, K, R, self.min_resp)
        self.lead, self.thr = margins(self.logits, self.hann, grid, K, R, self.min_resp)
        self.tol = du.sweep(grid, C).tol
        listed = np.arange(K)[None, :] < self.f64["n"][:, None]
        self.finite = np.all(np.isfinite(self.f64["fbox"]) | ~listed[:, :, None], axis=(1, 2)) & \
            np.all(np.isfinite(self.f64["score"]) | ~listed, axis=1)
        self.same_cells = bool(np.array_equal(self.ora["n"], self.f64["n"]) and np.array_equal(self.ora["cell"], self.f64["cell"]))
        self.dist = 0.0
        if self.same_cells and self.finite.any():
            m = self.finite[:, None] & listed
            self.dist = float(max(np.abs(self.ora["score"].astype(np.float64) - self.f64["score"])[m].max(),
                                  np.abs(self.ora["resp"].astype(np.float64) - self.f64["resp"])[m].max(),
                                  np.abs(self.ora["fbox"].astype(np.float64) - self.f64["fbox"])[m].max()))

    def head_out(self):
        ho = np.zeros((self.n * self.ns, 8), np.float32)
        ho[:, :5] = self.logits.reshape(-1, 5)
        return ho

    def prefix(self, K):
        """the oracle's lists under max_peaks = K <= self.K: the first K entries (the iteration does not look ahead)"""
        o = {k: v.copy() for k, v in self.ora.items()}
        o["n"] = np.minimum(o["n"], K)
        o["cell"][:, K:] = -1
        return o

    def report(self):
        kept = float(self.finite.mean())
        return (f"{self.name:<34} grid {self.grid:>2} R {self.R} K {self.K} cases {self.n:>4}  lead {self.lead.min():.2e}  "
                f"thr {self.thr.min():.2e}  |f32 - f64| {self.dist:.2e}  bar {self.tol:.2e}  compared {100 * kept:.1f} %")


def _logit_for(resp, h):
    """the float32 score logit whose response under window value h is (about) resp"""
    p = np.float64(resp) / np.float64(h)
    return np.float32(np.log(p / (1.0 - p)))


@functools.lru_cache(maxsize=None)
def planted(grid, C, R, n=48):
    """five planted maxima (score logits 6, 5, 4, 3, 2 at random distinct cells) on du's random background under the lifted
    window, K = 8: the list ends by min_resp. A draw whose float64 margins miss MARGIN is drawn again (deterministic)."""
    ns = grid * grid
    rng = np.random.default_rng(7000 + 10 * grid + R)
    hann = du.lifted_hann(grid).reshape(-1)
    lg = du._background(n, ns, rng)
    for i in range(n):
        base = lg[i, :, 0].copy()
        while True:
            lg[i, :, 0] = base
            lg[i, rng.choice(ns, 5, replace=False), 0] = [6.0, 5.0, 4.0, 3.0, 2.0]
            lead, thr = margins(lg[i:i + 1], hann, grid, KMAX, R, MIN_RESP)
            if lead[0] >= 2 * MARGIN and thr[0] >= 2 * MARGIN:
                break
    return PeakSet("planted", grid, C, lg, hann, du._plain_states(n, 7100 + grid), KMAX, R, MIN_RESP)


def second_cell(c, grid, R, direction):
    """the cell R + 1 away from c along `direction`, turned round where the map ends, clipped where it ends on both sides
    (the cell then lies inside c's square)"""
    bx, by = c % grid, c // grid
    out = []
    for v, d in ((bx, direction[0]), (by, direction[1])):
        w = v + d * (R + 1)
        if not 0 <= w < grid:
            w = v - d * (R + 1)
        out.append(int(np.clip(w, 0, grid - 1)))
    return out[1] * grid + out[0]


def direction_of(c, grid, R):
    """the direction of cell c's second maximum: cycling through the eight with the cell's position, but diagonal towards the
    corner for the four cells that lie R + 1 cells inside a corner, so that every corner is some case's second peak"""
    bx, by = c % grid, c // grid
    lo, hi = R + 1, grid - 2 - R
    if bx in (lo, hi) and by in (lo, hi) and R + 1 < grid:
        return (-1 if bx == lo else 1, -1 if by == lo else 1)
    return DIRS[(bx + 3 * by) % 8]


@functools.lru_cache(maxsize=None)
def border(grid, C, R):
    """every cell as peak 0 (score logit 6: response >= 0.4988 under the lifted window) with a second maximum of response
    0.42 R + 1 cells away, the direction cycling through the eight neighbours' - suppression squares cut by each edge and
    corner, second windows of 4 and 6 cells and windows beside the suppressed square. K = 3."""
    ns = grid * grid
    rng = np.random.default_rng(8000 + 10 * grid + R)
    hann = du.lifted_hann(grid).reshape(-1)
    lg = du._background(ns, ns, rng)
    second = np.array([second_cell(c, grid, R, direction_of(c, grid, R)) for c in range(ns)])
    for c in range(ns):
        if second[c] != c:
            lg[c, second[c], 0] = _logit_for(0.42, hann[second[c]])
        lg[c, c, 0] = 6.0
    s = PeakSet("border", grid, C, lg, hann, du._plain_states(ns, 8100 + grid), 3, R, MIN_RESP)
    s.second = second
    return s


@functools.lru_cache(maxsize=None)
def apart(grid, C, R):
    """two maxima R apart (case 0: one peak) and R + 1 apart (case 1: two); case 2: R + 1 apart with a NaN x-offset logit on
    the cell between them that lies in peak 0's square AND in peak 1's window - suppressed there, weight 0, and 0 * NaN is
    NaN: peak 1's x is NaN before the clamp, (0, 10) behind it, exactly as in the specification"""
    ns = grid * grid
    rng = np.random.default_rng(9000 + 10 * grid + R)
    hann = du.lifted_hann(grid).reshape(-1)
    lg = du._background(3, ns, rng)
    by = grid // 2
    c0 = by * grid + 0
    near, far = c0 + R, c0 + R + 1
    assert far % grid == R + 1 < grid
    lg[:, c0, 0] = 6.0
    lg[0, near, 0] = _logit_for(0.42, hann[near])
    lg[1:, far, 0] = _logit_for(0.42, hann[far])
    lg[2] = lg[1]                   # the same map but for the one NaN
    lg[2, near, 1] = np.nan
    st = du._plain_states(3, 9100 + grid)
    return PeakSet("apart", grid, C, lg, hann, st, KMAX, R, MIN_RESP)


@functools.lru_cache(maxsize=None)
def tie_order(grid, C, R=2):
    """du.tie_sets under a flat window with score logit 3 on the tying cells: equal float32 responses whatever expf returns,
    listed in ascending cell order as far as the squares leave them. Exact."""
    ns = grid * grid
    rng = np.random.default_rng(3000 + grid)
    sets = du.tie_sets(grid)
    lg = du._background(len(sets), ns, rng)
    for i, cells in enumerate(sets.values()):
        lg[i, cells, 0] = 3.0
    return PeakSet("ties", grid, C, lg, np.ones(ns, np.float32), du._plain_states(len(sets), 3100 + grid), KMAX, R, 0.5, exact=True)


def flat_expected(grid, R, K=KMAX):
    """a flat map under a flat window: cells 0, R + 1, 2 (R + 1), ... of row 0, then of row R + 1, ..."""
    per = list(range(0, grid, R + 1))
    return [y * grid + x for y in per for x in per][:K]


@functools.lru_cache(maxsize=None)
def flat(grid, C, R):
    """every logit 0 (sigmoid exactly 0.5), window all ones, min_resp 0.5 (met exactly): exact"""
    ns = grid * grid
    lg = np.zeros((1, ns, 5), np.float32)
    return PeakSet("flat", grid, C, lg, np.ones(ns, np.float32), du._plain_states(1, 3300 + grid), KMAX, R, 0.5, exact=True)


THR_ABOVE_HALF = du.THR_ABOVE_HALF


@functools.lru_cache(maxsize=None)
def at_min_resp(grid, C, min_resp):
    """peak 0 at score logit 6, one more cell at score logit 0 (response exactly 0.5 under the flat window, in every
    arithmetic), background below sigmoid(-4): min_resp = 0.5 lists it, one float above does not. Exact."""
    ns = grid * grid
    rng = np.random.default_rng(4000 + grid)
    lg = du._background(2, ns, rng)
    lg[:, :, 0] -= np.float32(3.0)
    lg[:, 0, 0] = 6.0
    lg[0, ns - 1, 0] = 0.0
    lg[1, (grid // 2) * grid + grid - 1, 0] = 0.0
    return PeakSet("min_resp", grid, C, lg, np.ones(ns, np.float32), du._plain_states(2, 4100 + grid), KMAX, 2, min_resp, exact=True)


@functools.lru_cache(maxsize=None)
def nonfinite(grid, C):
    """du.nonfinite_cases' logits (hann2d): +-inf and NaN logits through the iteration. The background lies below
    min_resp, so no list goes on into it. Its finite values go through the bar, so both margins are asserted like any
    compared set's (cases without a comparable response have nothing to measure: inf); what it may have that the others
    may not is cases without a finite float64 score (all-NaN)."""
    c = du.nonfinite_cases(grid, C)
    s = PeakSet("nonfinite", grid, C, c.logits, c.hann, c.states, KMAX, 2, MIN_RESP)
    s.names, s.allow_nonfinite = c.names, True
    return s


def all_sets(grid, C):
    out = [planted(grid, C, R) for R in (1, 2, 3, 4)] + [border(grid, C, R) for R in (1, 2, 3, 4)]
    out += [apart(grid, C, R) for R in (1, 2, 3, 4) if R + 1 < grid]
    out += [tie_order(grid, C), flat(grid, C, 2), at_min_resp(grid, C, 0.5), at_min_resp(grid, C, THR_ABOVE_HALF), nonfinite(grid, C)]
    return out


def same_or_both_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))
