"""The stream conflicts ("Stream conflicts"; the rule to the bit: include/vittrack_hip.h above the
"conflicts*" keys) restated in NumPy float32, for the tests: the one launch of k_conflicts.hip, and the refresh gate with rule
9 on top of appearance_util.Rule (rules 1-8).

Every operation below is one binary32 operation: the operands are np.float32 scalars or arrays, and NumPy rounds each
result to binary32. `mut` names a deliberate slip (tests/test_conflicts_cases.py shows that the cases catch each of them):
    "gt"       iou > tau instead of iou >= tau
    "slot"     ties between equal IoUs broken by the slot, not by the stream index
    "fused"    w_s * h_s + w_t * h_t with one rounding instead of two (what -ffp-contract=fast would make of it)
    "failed"   streams whose update failed stay partners of the others
"""
import numpy as np

import appearance_util as ap

F = np.float32
REC = np.dtype([("status", "<i4"), ("frames_done", "<i4"), ("n_over", "<i4"), ("reserved", "<i4"), ("partner", "<i4", 4),
                ("iou", "<f4", 4)])
COUNT = np.dtype([("evaluated", "<i4"), ("conflicting", "<i4"), ("gated", "<i4"), ("reserved", "<i4")])
assert REC.itemsize == 48 and COUNT.itemsize == 16


def tau_of(pm):
    return F(pm) / F(1000.0)


def iou(s, t, mut=None):
    """box s (x, y, w, h) against box t, or against boxes t [k, 4] -> the IoU as binary32 (an array for an array); 0 where
    they do not overlap. Array operations on float32 round every element's result to binary32 like the scalar ones."""
    s, t = np.asarray(s, F), np.asarray(t, F)
    xs, ys, ws, hs = s
    xt, yt, wt, ht = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    ix = np.minimum(xs + ws, xt + wt) - np.maximum(xs, xt)
    iy = np.minimum(ys + hs, yt + ht) - np.maximum(ys, yt)
    inter = ix * iy
    if mut == "fused":      # fma(w_s, h_s, w_t * h_t): the first product exact, one rounding of the sum
        both = (np.float64(ws) * np.float64(hs) + (wt * ht).astype(np.float64)).astype(F)
    else:
        both = ws * hs + wt * ht
    uni = both - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        v = inter / uni
    assert v.dtype == F
    return np.where((ix > 0) & (iy > 0), v, F(0.0))


def record(status, frames_done, n_over=0, partners=()):
    r = np.zeros((), REC)
    r["status"], r["frames_done"], r["n_over"] = status, frames_done, n_over
    r["partner"][:] = -1
    for k, (p, v) in enumerate(partners[:4]):
        r["partner"][k], r["iou"][k] = p, v
    return r


def check(boxes, success, scenes, pm=300, frames_done=None, initialized=None, window_miss=None, slot_stream=None, winner=None,
          on=1, mut=None):
    """One launch. By stream: boxes [B, 4], scenes [B], frames_done / initialized / window_miss [B] (None: 1 / 1 / 0: a
    stream after its first update, without a window miss); by slot: success [n], slot_stream [n] (None: the identity), winner
    [n] (None: the first slot that names a stream works for it). -> {stream: record} of the streams the pass wrote - none
    with on == 0 - in REC layout; a record with status 1 or 2 counts once in `evaluated`, with status 2 in `conflicting`."""
    if not on:
        return {}
    boxes = np.asarray(boxes, F).reshape(-1, 4)
    B, n = len(boxes), len(success)
    scenes = np.asarray(scenes, np.int64)
    fd = np.ones(B, np.int64) if frames_done is None else np.asarray(frames_done, np.int64)
    init = np.ones(B, np.int64) if initialized is None else np.asarray(initialized, np.int64)
    miss = np.zeros(B, np.int64) if window_miss is None else np.asarray(window_miss, np.int64)
    smap = np.arange(n) if slot_stream is None else np.asarray(slot_stream, np.int64)
    tau = tau_of(pm)
    work, seen = [], set()      # (slot, stream, eligible)
    for i in range(n):
        s = int(smap[i])
        if winner is not None:
            if int(winner[i]) != i:
                continue
        elif s in seen:
            continue
        seen.add(s)
        ok = scenes[s] != 0 and init[s] != 0 and bool(success[i]) and miss[s] != fd[s]
        work.append((i, s, bool(ok)))
    out = {}
    for i, s, ok in work:
        if not ok:
            out[s] = record(3, fd[s])
            continue
        cand = [(j, t) for j, t, ok_t in work
                if t != s and scenes[t] == scenes[s] and
                (ok_t or (mut == "failed" and scenes[t] != 0 and init[t] != 0 and miss[t] != fd[t]))]
        over = []
        if cand:
            v = iou(boxes[s], boxes[[t for _, t in cand]], mut)
            hit = (v > 0) & ((v > tau) if mut == "gt" else (v >= tau))
            over = [(-float(v[k]), cand[k][0] if mut == "slot" else cand[k][1], cand[k][1], v[k]) for k in np.flatnonzero(hit)]
        over.sort(key=lambda e: e[:2])
        out[s] = record(2 if over else 1, fd[s], len(over), [(t, v) for _, _, t, v in over])
    return out


def check_states(states, results, scenes, **kw):
    """check() on snapshot.STATE records by stream and result records by slot (fields .success or ["success"])"""
    st = np.asarray(states).reshape(-1)
    succ = [int(r["success"]) if isinstance(r, np.void) else int(r.success) for r in results]
    return check(st["box"], succ, scenes, frames_done=st["frames_done"], initialized=st["initialized"],
                 window_miss=st["window_miss"], **kw)


def apply(records, counts, out):
    """what one launch leaves: the written records over `records`, the counters advanced (both REC / COUNT arrays by stream)"""
    records, counts = records.copy(), counts.copy()
    for s, r in out.items():
        records[s] = r
        if r["status"] in (1, 2):
            counts["evaluated"][s] += 1
            counts["conflicting"][s] += int(r["status"] == 2)
    return records, counts


class Rule(ap.Rule):
    """appearance_util.Rule (rules 1-8) plus rule 9: with the gate on, a refresh that rules 1-5 allow is suppressed where this
    update's conflict record of the stream has status 2; checked AHEAD of rules 6-8, so it counts no geometry skip. step()
    takes the update's conflict status as `conflict` and returns "conflict" where the rule fires, else what the parent returns."""

    def __init__(self, T, S, period, min_score=0.0, gate_pm=0, conflicts_gate=False):
        super().__init__(T, S, period, min_score, gate_pm)
        self.conflicts_gate = bool(conflicts_gate)
        self.conflict_gated = []

    def step(self, result, pre_box=None, geo=None, window_miss=False, winner=True, record=None, conflict=0):
        done = self.done + 1
        due = self.period >= 2 and winner and result.success and (F(result.score) >= self.min_score) and \
            done - self.last_frame >= self.period and not window_miss
        if self.conflicts_gate and due and conflict == 2:
            self.done = done
            self.conflict_gated.append(done)
            return "conflict"
        return super().step(result, pre_box=pre_box, geo=geo, window_miss=window_miss, winner=winner, record=record)
