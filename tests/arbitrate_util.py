"""The peak arbitration ("Peak arbitration"; the rule to the bit: include/vittrack_hip_ops.h above
vt_op_arbitrate) restated in NumPy, for the tests. Nothing here is new arithmetic; three existing restatements are combined:

  * the list: peaks_util.iterate_oracle (vto_decode iterated) under the policy's K, R and min_resp;
  * the geometry: template_refresh_util's tap rectangles (refresh rule 6) and the stored window (rule 7);
  * the score: appearance_util.score on the anchor rows and the rows cut at each peak's integer box.

examine() is the list launch's decision per slot, commit() the commit launch's, apply() what a switch rewrites. The crop itself
is not restated: the tests take the rows from wherever the caller cuts them (vt_group_init_* on the GPU, oracle.preproc on the
CPU) and feed their similarities in."""
import numpy as np

import appearance_util as au
import peaks_util as pk
from template_refresh_util import F, inside, tap_rect, tap_rect_geo

KMAX = 4
DEFAULTS = dict(on=0, max_peaks=3, radius=2, min_resp_pm=50, low_pm=300, high_pm=500)
# record status
NOT_DUE, KEPT, SWITCHED, CANDIDATE, RULE6, WINDOW_MISS = 0, 1, 2, 3, 4, 5
# peak status
P_NONE, P_SCORED, P_RULE6, P_FLAT = 0, 1, 2, 3


def threshold(pm):
    """(float)pm / 1000.0f: one binary32 divide"""
    return F(F(pm) / F(1000.0))


def int_box(fbox):
    """floorf(v + 0.5f) of the four floats, as the decode rounds -> float32 [4] of integers"""
    return np.floor(np.asarray(fbox, F) + F(0.5)).astype(F)


def taps_rule(ibox, geo, T, S, frame_wh, window=None):
    """refresh rules 6 and 7 for a template crop at the integer box against the search crop the pass sampled (geo) and the
    window stored of the frame (x0, y0, ww, wh; None: the whole frame) -> 0, 6 or 7"""
    t = tap_rect(np.asarray(ibox, F), 2.0, T)
    if not inside(t, tap_rect_geo(geo, S)):
        return 6
    w, h = frame_wh
    x0, y0, ww, wh = (0, 0, w, h) if window is None else window
    cx0, cx1, cy0, cy1 = max(t[0], 0), min(t[1], w - 1), max(t[2], 0), min(t[3], h - 1)
    if cx0 <= cx1 and cy0 <= cy1 and (cx0 < x0 or cx1 >= x0 + ww or cy0 < y0 or cy1 >= y0 + wh):
        return 7
    return 0


def lists(logits, hann, grid, geo, fw, fh, K, R, min_resp_pm):
    """the list launch's iteration over the cases -> peaks_util.iterate_oracle's dict"""
    return pk.iterate_oracle(logits, hann, grid, geo, fw, fh, K, R, float(threshold(min_resp_pm)))


def examine(lst, i, *, on, success, frames_done, window_miss, geo, frame_wh, T, S, success_threshold, window=None, candidate=False):
    """the list launch's decision for case i of `lst` -> dict(status (KEPT stands for "due": commit() completes it), n,
    peak_status [KMAX], mark (the rule-7 failure sets window_miss = frames_done))"""
    out = dict(status=NOT_DUE, n=0, peak_status=[P_NONE] * KMAX, mark=False)
    if not on or candidate or not success or window_miss == frames_done:
        out["status"] = CANDIDATE if on and candidate else NOT_DUE
        return out
    n = int(lst["n"][i])
    out["n"] = n
    status, eligible, ps = 0, 0, [P_NONE] * KMAX
    for k in range(n):
        if k >= 1 and not (F(lst["score"][i, k]) >= F(success_threshold)):
            continue
        rule = taps_rule(int_box(lst["fbox"][i, k]), geo, T, S, frame_wh, window)
        if rule == 7:
            status = WINDOW_MISS
        elif rule == 6:
            if k == 0:
                status = RULE6
            else:
                ps[k] = P_RULE6
        else:
            ps[k] = P_SCORED
            eligible += k >= 1
        if status:
            break
    if status == 0 and eligible > 0:
        out["status"], out["peak_status"] = KEPT, ps
        return out
    out["status"] = status
    out["peak_status"] = [P_NONE if s == P_SCORED else s for s in ps]
    out["mark"] = status == WINDOW_MISS
    return out


def commit(peak_status, sims, n, low_pm, high_pm):
    """the commit launch on a due slot. peak_status: examine()'s; sims[k] = (score status 1 / 3, similarity as binary32) of
    the peaks examine() marked P_SCORED -> (record status, chosen, final peak statuses)"""
    low, high = threshold(low_pm), threshold(high_pm)
    ps = list(peak_status)
    sim = [F(0)] * KMAX
    for k in range(n):
        if ps[k] == P_SCORED:
            st, v = sims[k]
            ps[k] = P_SCORED if st == 1 else P_FLAT
            sim[k] = F(v) if st == 1 else F(0)
    chosen, best = 0, F(0)
    if ps[0] == P_SCORED and low > 0 and sim[0] < low:          # low 0 challenges nobody, a negative similarity included
        for k in range(1, n):
            if ps[k] != P_SCORED or not (sim[k] >= high):
                continue
            if chosen == 0 or sim[k] > best:
                chosen, best = k, sim[k]
    return (SWITCHED if chosen else KEPT), chosen, ps, sim


def apply(state, result, lst, i, k):
    """what a switch to peak k rewrites, in place: the result record (success, score, bbox) and the state's last_fbox,
    last_score, last_idx and box. frames_done and success_count stay."""
    ib = int_box(lst["fbox"][i, k])
    result["success"] = 1
    result["score"] = F(lst["score"][i, k])
    result["bbox"] = ib.astype(np.int32)
    state["last_fbox"] = np.asarray(lst["fbox"][i, k], F)
    state["last_score"] = F(lst["score"][i, k])
    state["last_idx"] = int(lst["cell"][i, k])
    state["box"] = ib


def similarity(anchor_bits, probe_bits, cols):
    """-> (status, similarity) of appearance_util.score"""
    s = au.score(anchor_bits, probe_bits, cols)
    return s["status"], s["similarity"]


def lists_of_records(recs, K):
    """vt_peaks records (PEAKS_DTYPE, the response-peaks launch's) as iterate_oracle's dict, the first K entries"""
    n = len(recs)
    out = dict(n=np.minimum(recs["n"], K).astype(np.int64), cell=np.full((n, K), -1, np.int64), score=np.zeros((n, K), F),
               resp=np.zeros((n, K), F), fbox=np.zeros((n, K, 4), F))
    for i in range(n):
        for k in range(int(out["n"][i])):
            p = recs["peak"][i][k]
            out["cell"][i, k], out["score"][i, k], out["resp"][i, k], out["fbox"][i, k] = p["cell"], p["score"], p["resp"], p["box"]
    return out


def decide(lst, i, sims_of, *, state, success, frame_wh, T, S, success_threshold, policy, window=None, candidate=False):
    """examine() and, where the slot is due, commit() with the similarities sims_of(k, integer box) supplies for the marked
    peaks -> dict(status, n, chosen, peak_status, sim)"""
    ex = examine(lst, i, on=policy["on"], success=success, frames_done=int(state["frames_done"]), window_miss=int(state["window_miss"]),
                 geo=state["geo"], frame_wh=frame_wh, T=T, S=S, success_threshold=success_threshold, window=window, candidate=candidate)
    out = dict(status=ex["status"], n=ex["n"], chosen=0, peak_status=ex["peak_status"], sim=[F(0)] * KMAX, mark=ex["mark"])
    if ex["status"] == KEPT:
        sims = {k: sims_of(k, int_box(lst["fbox"][i, k])) for k in range(ex["n"]) if ex["peak_status"][k] == P_SCORED}
        out["status"], out["chosen"], out["peak_status"], out["sim"] = commit(ex["peak_status"], sims, ex["n"], policy["low_pm"],
                                                                             policy["high_pm"])
    return out


# ---- the planted scene of the operator tests: five streams on the tiny model's shapes -------------------------------------
# Every stream searched around the box (120, 90, 48, 48) of a 320 x 240 frame: the search crop has side 192 and origin
# (48, 18), a cell of the 8 x 8 map covers 24 px, and a 48-px box passes refresh rule 6 while its centre lies within 48 px of
# the crop's centre - cells 2..5 of either axis. The TARGET is a 48-px high-contrast texture on a low-contrast background, the
# DECOY another texture; the anchor is the template crop at the target in a picture of its own.
W, H, T, S, PATCH, KPAD, GRID = 320, 240, 64, 128, 16, 768, 8
COLS = 3 * PATCH * PATCH
PREV_BOX = (120.0, 90.0, 48.0, 48.0)
ANCHOR_BOX = (100, 80, 48, 48)
SUCCESS_THRESHOLD = 0.5
SIZE_LOGIT = float(np.log(0.25 / 0.75))         # sigmoid = 0.25: a box of a quarter of the crop's side
# stream -> planted peaks in listing order: (cell x, cell y, score logit, what the picture shows there)
PLAN = {
    0: [(2, 3, 5.0, "decoy"), (5, 4, 2.5, "target")],                                     # switched to peak 1
    1: [(4, 3, 5.0, "target"), (2, 5, 2.5, "decoy")],                                     # kept: peak 0 matches
    2: [(3, 4, 5.0, "decoy")],                                                            # no runner-up: not due
    3: [(1, 3, 5.0, "decoy"), (4, 4, 2.5, "target")],                                     # peak 0 fails rule 6: status 4
    4: [(3, 2, 5.0, "decoy"), (6, 5, 2.5, "target"), (5, 2, 1.5, "target"), (3, 5, -0.5, "target")],
    # K = 2: the one runner-up fails rule 6 - not due; K = 3: switched to peak 2; K = 4: the fourth scores below the threshold
}


def window():
    """the scene's Hann stand-in, 0.97..1: with score logits 5, 2.5, 1.5 and -0.5 the responses list in the plan's order
    wherever the peaks sit, with more than 1 % between neighbours"""
    import decode_util as du
    return (F(0.94) + F(0.06) * du.lifted_hann(GRID).reshape(-1)).astype(F)


def _texture(seed):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 2, (8, 8, 3)) * 255, np.ones((6, 6, 1))).astype(np.uint8)


def cell_box(ix, iy, geo):
    """the 48-px box centred on the cell's centre under offset logits 0 (an offset of half a cell)"""
    cx = float(geo[0]) + 0.5 + (ix + 0.5) / GRID * float(geo[3])
    cy = float(geo[1]) + 0.5 + (iy + 0.5) / GRID * float(geo[3])
    return int(round(cx - 24)), int(round(cy - 24))


def scene(geo):
    """-> dict(pictures [5, H, W, 3] uint8, logits [5, 64, 5] float32, anchor_picture [H, W, 3]); geo: the search crop's"""
    target, decoy = _texture(11), _texture(12)
    rng = np.random.default_rng(13)
    pics = np.kron(rng.integers(100, 141, (len(PLAN), H // 8, W // 8, 3)), np.ones((1, 8, 8, 1))).astype(np.uint8)
    lg = np.zeros((len(PLAN), GRID * GRID, 5), np.float32)
    lg[:, :, 0] = rng.uniform(-7.0, -5.0, lg.shape[:2])
    lg[:, :, 3:] = SIZE_LOGIT + rng.uniform(-0.02, 0.02, lg[:, :, 3:].shape)
    lg[:, :, 1:3] = rng.uniform(-0.05, 0.05, lg[:, :, 1:3].shape)
    for s, peaks in PLAN.items():
        for ix, iy, logit, what in peaks:
            lg[s, iy * GRID + ix, 0] = logit
            x, y = cell_box(ix, iy, geo)
            pics[s, y:y + 48, x:x + 48] = target if what == "target" else decoy
    anchor = np.kron(rng.integers(100, 141, (H // 8, W // 8, 3)), np.ones((8, 8, 1))).astype(np.uint8)
    anchor[ANCHOR_BOX[1]:ANCHOR_BOX[1] + 48, ANCHOR_BOX[0]:ANCHOR_BOX[0] + 48] = target
    return dict(pictures=pics, logits=lg, anchor_picture=anchor)
