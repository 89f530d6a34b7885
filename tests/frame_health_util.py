"""The NumPy model of the frame health (include/vittrack_hip_ops.h, vt_op_frame_health; csrc/k_health.hip).

Every number of the rule is an exact integer: Python integers and int64 arrays throughout, so the kernels are held to these
values with np.array_equal. The thumbnail is camera motion's. Nothing in here reads the engine."""
import numpy as np

from camera_motion_util import thumbnail, auto_cell, texture            # noqa: F401
from proposals_util import DevFrame, FORMATS, from_rgb, to_rgb          # noqa: F401  (the GPU tests' device frames)

FROZEN, FLAT, CUT = 1, 2, 4
BINS = 32
STILL_CAP = 1 << 30
MEASURED = (1, 5)


def geometry(W, H, cell, max_cells):
    """-> dict(status 1 | 2, c, Wg, Hg); c, Wg, Hg are 0 where no cell exists"""
    c = cell if cell else auto_cell(W, H, max_cells)
    g = dict(status=2, c=c, Wg=W // c if c else 0, Hg=H // c if c else 0)
    if c and g["Wg"] * g["Hg"] <= max_cells and g["Wg"] >= 8 and g["Hg"] >= 8:
        g["status"] = 1
    return g


def measures(t, shift=7, vertical=True):
    """the thumbnail [Hg, Wg] -> (S1, S2, G) Python integers and hist [32] int64. shift 6, vertical False: mutations"""
    t = np.asarray(t, np.int64)
    G = int(np.abs(t[:, 1:] - t[:, :-1]).sum())
    if vertical:
        G += int(np.abs(t[1:, :] - t[:-1, :]).sum())
    hist = np.bincount((t >> shift).ravel(), minlength=BINS << (7 - shift)).astype(np.int64)
    return int(t.sum()), int((t * t).sum()), G, hist


def is_flat(n, S1, S2, flat_q, strict=False):
    lhs, rhs = n * S2 - S1 * S1, flat_q * flat_q * n * n
    return lhs < rhs if strict else lhs <= rhs


class Stream:
    """one stream's side of the rule: the thumbnails' bookkeeping, still, G_ref, the counters, and one pass at a time"""

    def __init__(self):
        self.has_prev, self.cur, self.geom = 0, 0, None
        self.thumbs = [None, None]
        self.hists = [None, None]
        self.still = self.G_ref = 0
        self.evaluated = self.flagged = self.gated = 0
        self.rec = None             # the last record written (a pass that is not due writes none)

    def reset(self):        # init, import, the destination of a copy, "health" 0
        self.has_prev = self.still = 0
        self.rec = None

    def step(self, rgb, on=1, period=1, cell=0, still_run=3, flat_q=32, cut_pm=500, max_cells=65536, initialised=True,
             device=True, whole=True, frames_done=0, **mut):
        """one pass that lists the stream (its first slot). rgb: [H, W, 3] integers as the pixel fetch reads the frame. ->
        the record as a dict with "thumb" and "hist" (what the pass took, or None) and the counters; status 0: dict(status=0)
        and nothing else changes. mut: strict (< for <=), shift (the bin shift), vertical (G's second term), still5 (still
        counted from the status-5 pass), drop (a pass that is not due drops the thumbnail)"""
        H, W = rgb.shape[:2]
        if not (on and initialised and frames_done % period == 0):
            if mut.get("drop"):
                self.has_prev = 0
            return dict(status=0, thumb=None, hist=None)
        rec = dict(status=1, frames_done=frames_done, flags=0, c=0, Wg=0, Hg=0, still=0, S1=0, S2=0, G=0, D=0, HD=0, G_ref=0,
                   thumb=None, hist=None)
        if not (device and whole):
            rec["status"] = 4
        else:
            g = geometry(W, H, cell, max_cells)
            rec.update(c=g["c"], Wg=g["Wg"], Hg=g["Hg"], status=g["status"])
        if rec["status"] != 1:
            self.has_prev = self.still = self.G_ref = 0
            return self._done(rec)
        geom = (W, H, rec["c"])
        prev_ok = bool(self.has_prev) and self.geom == geom
        cur = (self.cur ^ 1) if self.has_prev else 0
        p, hp = self.thumbs[cur ^ 1], self.hists[cur ^ 1]
        t = thumbnail(rgb, rec["c"], rec["Wg"], rec["Hg"])
        S1, S2, G, hist = measures(t, shift=mut.get("shift", 7), vertical=mut.get("vertical", True))
        self.thumbs[cur], self.hists[cur] = t, hist
        self.has_prev, self.cur, self.geom = 1, cur, geom
        n = rec["Wg"] * rec["Hg"]
        rec.update(S1=S1, S2=S2, G=G, thumb=t, hist=hist)
        flags = FLAT if is_flat(n, S1, S2, flat_q, strict=mut.get("strict", False)) else 0
        if not prev_ok:
            rec["status"] = 5
            self.still = 1 if mut.get("still5") else 0
            self.G_ref = G
        else:
            D = int(np.abs(t.astype(np.int64) - p.astype(np.int64)).sum())
            HD = int(np.abs(hist - hp).sum())
            self.still = min(self.still + 1, STILL_CAP) if D == 0 else 0
            rec.update(D=D, HD=HD)
            if self.still >= still_run:
                flags |= FROZEN
            if cut_pm > 0 and HD * 1000 >= cut_pm * 2 * n:
                flags |= CUT
                self.G_ref = G
        rec["flags"] = flags
        rec["still"] = 0 if rec["status"] == 5 else self.still
        self.evaluated += 1
        self.flagged += flags != 0
        return self._done(rec)

    def _done(self, rec):
        rec["G_ref"] = self.G_ref
        rec["evaluated"], rec["flagged"], rec["gated"] = self.evaluated, self.flagged, self.gated
        self.rec = rec
        return rec


# ---- pictures ---------------------------------------------------------------------------------------------------------

def grey(h, w, v):
    return np.full((h, w, 3), v, np.uint8)


def halves(h, w, v1, v2):
    """left half v1, right half v2 (w / 2 a multiple of the cell): the thumbnail's standard deviation is 8 |v1 - v2|"""
    a = grey(h, w, v1)
    a[:, w // 2:] = v2
    return a


# ---- the operator hook's outputs against the model (GPU tests) -----------------------------------------------------------

REC_FIELDS = ("status", "frames_done", "flags", "c", "Wg", "Hg", "still", "S1", "S2", "G", "D", "HD", "G_ref")


def check_stream(got, stream, want, model, before=None):
    """the hook's outputs of one worked stream against step()'s dict and the Stream behind it, value for value. before: the
    call's inputs (dict of thumbs, hist, records, counts) - a stream that was not due must equal them byte for byte"""
    rec, cnt = got["records"][stream], got["counts"][stream]
    if want["status"] == 0:
        assert before is not None
        for k in ("thumbs", "hist", "records", "counts"):
            assert got[k][stream].tobytes() == before[k][stream].tobytes(), (stream, k)
        assert (got["accs"][stream] == -1).all(), stream
        return
    for k in REC_FIELDS:
        assert int(rec[k]) == int(want[k]), (stream, k, int(rec[k]), int(want[k]))
    assert (int(cnt["evaluated"]), int(cnt["flagged"])) == (want["evaluated"], want["flagged"]), (stream, cnt)
    assert int(rec["has_prev"]) == model.has_prev, stream
    if want["thumb"] is None:
        assert (got["accs"][stream] == -1).all(), stream
        return
    n = want["Wg"] * want["Hg"]
    assert int(rec["cur"]) == model.cur and (int(rec["pW"]), int(rec["pH"]), int(rec["pc"])) == model.geom, stream
    assert np.array_equal(got["thumbs"][stream, model.cur, :n].reshape(want["Hg"], want["Wg"]), want["thumb"]), stream
    assert np.array_equal(got["hist"][stream, model.cur], want["hist"]), stream
    acc = [want["S1"], want["S2"], want["G"], want["D"]]
    if want["status"] == 5:
        acc[3] = 0                  # zeroed by the prepare launch, added to by nobody
    assert got["accs"][stream].tolist() == acc, (stream, got["accs"][stream], acc)
    if before is not None:          # the cells behind the grid and the other buffer stay
        assert np.array_equal(got["thumbs"][stream, model.cur, n:], before["thumbs"][stream, model.cur, n:]), stream
        assert np.array_equal(got["thumbs"][stream, model.cur ^ 1], before["thumbs"][stream, model.cur ^ 1]), stream
        assert np.array_equal(got["hist"][stream, model.cur ^ 1], before["hist"][stream, model.cur ^ 1]), stream
