"""The appearance check ("Appearance check") restated in NumPy float64, for the tests: the score of
k_appearance.hip, its error bound, and the refresh gate with rule 8 on top of template_refresh_util.Rule.

The score. a = anchor rows, p = probe rows, [nt, kpad] bf16 bit patterns, of which the first cols = 3 * patch * patch
columns of every row count (the pad columns are never read); every element the exact binary64 value of its bf16;
n = nt * cols:

    Sa = sum a, Sp = sum p, Saa = sum a*a, Spp = sum p*p, Sap = sum a*p
    cov = Sap - Sa*Sp/n, va = Saa - Sa*Sa/n, vp = Spp - Sp*Sp/n
    sim = cov / sqrt(va * vp) if va > 0 and vp > 0 else 0, clamped to [-1, 1], rounded once to binary32
    status = 1, or 3 when a variance is not positive

The error bound, for ANY order of the additions. u = 2^-53. A bf16 value has 8 significant bits, so every product a*a,
p*p, a*p has at most 16 and is EXACT in binary64: the only errors of a sum are those of its additions. Whatever the order
- a loop, a tree, per-lane partials joined later - the additions form a binary tree with n leaves; every addition errs by
at most u times its own partial sum, and a term passes through at most n - 1 additions, so (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2)

    |S^ - S| <= g * sum |x_i|,   g = (n - 1) u / (1 - (n - 1) u).

With Q = sqrt(Saa * Spp) and Cauchy-Schwarz (sum |a p| <= Q, |Sa| <= sqrt(n Saa), |Sp| <= sqrt(n Spp)):

    Saa, Spp: relative error <= g (their terms are non-negative)
    Sap: absolute error <= g Q;  Sa: <= g sqrt(n Saa);  Sp: <= g sqrt(n Spp)
    Sa*Sp/n: |value| <= Q, two sums in error and two roundings: absolute error <= (2g + 2u) Q (first order)
    cov: <= g Q + (2g + 2u) Q + u (|Sap| + Q) <= (3g + 4u) Q
    va:  <= g Saa + (2g + 2u) Saa + u Saa = (3g + 3u) Saa, and the same for vp with Spp.

PREMISE: va >= f * Saa and vp >= f * Spp for a stated fraction f in (0, 1] - the rows are not a large constant plus a
small signal. Every tolerance test asserts it on its own data (premise()). Then va and vp have relative error
<= (3g + 3u) / f, sqrt(va * vp) =: D >= f Q has relative error <= (3g + 3u) / f + 3u (the product's rounding, half of the
sum of both relative errors, the square root's and the division's roundings), and with |sim| <= 1

    |sim^ - sim| <= (3g + 4u) Q / D + |sim| ((3g + 3u) / f + 3u) <= (6g + 7u) / f + 3u.

That is one evaluation against the exact value. What the tests compare are TWO evaluations in different orders - the
kernel's and NumPy's pairwise sums -, neither of them exact: each lies within the expression above of the exact value, so
THE DERIVED BOUND on their difference is twice it,

    |sim_1^ - sim_2^| <= 2 ((6g + 7u) / f + 3u),

which sim_bound() returns, times 1.01 for the second-order terms (n u < 1e-9 at every shape in use). Rounding both to
binary32 adds at most one binary32 ulp of the value: the tolerance is the derived bound plus that ulp (sim_tolerance()).

The five sums themselves are exact, in any order, when the data are small integers: with |v| <= 16 every partial sum is an
integer below 2^53.
"""
import numpy as np

from template_refresh_util import F, Rule as RefreshRule, inside, tap_rect, tap_rect_geo

U = 2.0 ** -53


def bits_to_f64(bits):
    b = np.ascontiguousarray(bits, np.uint16)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def f32_to_bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def sums(anchor_bits, probe_bits, cols):
    """-> (Sa, Sp, Saa, Spp, Sap) float64 over columns [0, cols) of [nt, kpad] bf16 bit patterns"""
    a = bits_to_f64(np.asarray(anchor_bits)[:, :cols])
    p = bits_to_f64(np.asarray(probe_bits)[:, :cols])
    return np.array([a.sum(), p.sum(), (a * a).sum(), (p * p).sum(), (a * p).sum()], np.float64)


def finish(s, n):
    """the five sums -> (similarity as binary32, status)"""
    sa, sp, saa, spp, sap = (np.float64(v) for v in s)
    n = np.float64(n)
    cov = sap - sa * sp / n
    va = saa - sa * sa / n
    vp = spp - sp * sp / n
    if not (va > 0 and vp > 0):
        return np.float32(0.0), 3
    sim = cov / np.sqrt(va * vp)
    return np.float32(min(max(sim, -1.0), 1.0)), 1


def score(anchor_bits, probe_bits, cols):
    """-> dict(sums, similarity (np.float32), status)"""
    s = sums(anchor_bits, probe_bits, cols)
    sim, status = finish(s, np.asarray(anchor_bits).shape[0] * cols)
    return dict(sums=s, similarity=sim, status=status)


def premise(anchor_bits, probe_bits, cols):
    """-> the largest f with va >= f * Saa and vp >= f * Spp on these rows (0 when a variance is not positive)"""
    sa, sp, saa, spp, _ = sums(anchor_bits, probe_bits, cols)
    n = np.asarray(anchor_bits).shape[0] * cols
    va, vp = saa - sa * sa / n, spp - sp * sp / n
    if not (va > 0 and vp > 0):
        return 0.0
    return float(min(va / saa, vp / spp))


def gamma(n):
    return (n - 1) * U / (1.0 - (n - 1) * U)


def sim_bound(n, f):
    """the derived bound: |difference| of two evaluations of one similarity in binary64, each in any summation order, under
    the premise with fraction f"""
    g = gamma(n)
    return 1.01 * 2.0 * ((6.0 * g + 7.0 * U) / f + 3.0 * U)


def sim_tolerance(n, f, value):
    """two evaluations of one similarity, each rounded once to binary32: the derived bound plus one binary32 ulp of the value"""
    return sim_bound(n, f) + float(np.spacing(np.float32(max(abs(float(value)), 2.0 ** -126))))


class Rule(RefreshRule):
    """template_refresh_util.Rule plus rule 8: with tau > 0 a refresh that rules 1-7 allow also needs the similarity of
    this update's probe (status 1) to be >= tau; else nothing is cut, `gated` counts it and the stream tries again at its
    next update. step() takes the update's record as (status, similarity) and returns "fire", "gate", "skip" or None."""

    def __init__(self, T, S, period, min_score=0.0, gate_pm=0):
        super().__init__(T, S, period, min_score)
        self.gate_pm = int(gate_pm)
        self.tau = F(gate_pm) / F(1000.0)
        self.gated = []

    def step(self, result, pre_box=None, geo=None, window_miss=False, winner=True, record=None):
        if not (self.tau > 0):
            return super().step(result, pre_box=pre_box, geo=geo, window_miss=window_miss, winner=winner)
        done = self.done + 1
        # rules 1-7 exactly as the parent decides them, then rule 8 in front of the effect
        if self.period < 2 or not winner or not result.success or not (F(result.score) >= self.min_score) or \
                done - self.last_frame < self.period or window_miss:
            self.done = done
            return None
        s = tap_rect_geo(geo, self.S) if geo is not None else tap_rect(pre_box, 4.0, self.S)
        if inside(tap_rect(np.asarray(result.bbox, F), 2.0, self.T), s):
            status, sim = record
            if not (status == 1 and F(sim) >= self.tau):
                self.done = done
                self.gated.append(done)
                return "gate"
        return super().step(result, pre_box=pre_box, geo=geo, window_miss=window_miss, winner=winner)


def due(rule, result, frames_done, last_frame, period, window_miss=False, winner=True, on=True):
    """the probe launch's due rule (a)-(e) for an update that left the stream at frames_done; rule: the stream's refresh
    Rule or None; last_frame: the stream's tpl_frame in front of this pass's refresh launch"""
    if not on or not winner or not result.success or window_miss:
        return False
    if frames_done % period == 0:
        return True
    if rule is None or not (getattr(rule, "tau", F(0)) > 0):
        return False
    return rule.period >= 2 and F(result.score) >= rule.min_score and frames_done - last_frame >= rule.period
