"""The NumPy model of the moving regions (include/vittrack_hip_ops.h, vt_op_movers; csrc/k_movers.hip).

Every number of the rule is an exact integer (the corners of the own box: binary32 scaled by a power of two): Python integers
and int64 arrays throughout, so the kernels are held to these values with np.array_equal. The thumbnail and the geometry are
frame health's. Nothing in here reads the engine."""
import numpy as np

from frame_health_util import geometry, thumbnail, texture, grey, DevFrame, FORMATS, from_rgb, to_rgb     # noqa: F401

STILL_CAP = 1 << 30
MAX_BOXES = 8
REC_FIELDS = ("status", "frames_done", "c", "Wg", "Hg", "n", "moving", "kept", "components", "own_cells", "own_kept", "still")


def difference(t, bg):
    """d = 16 t - bg, int64"""
    return 16 * np.asarray(t, np.int64) - np.asarray(bg, np.int64)


def moving_mask(d, thr, ge=False):
    """|d| > 16 thr. ge: the mutation >="""
    return np.abs(d) >= 16 * thr if ge else np.abs(d) > 16 * thr


def updated(bg, d, learn):
    """bg + (d >> learn): NumPy's >> of a signed integer is the arithmetic shift, floor(d / 2^learn)"""
    return np.asarray(bg, np.int64) + (d >> learn)


def clean(moving, min_nb, outside=False):
    """kept: moving and at least min_nb moving cells in the 3x3 neighbourhood, itself included. outside: the mutation that
    counts the cells beyond the border as moving"""
    m = np.pad(moving.astype(np.int64), 1, constant_values=1 if outside else 0)
    H, W = moving.shape
    nb = sum(m[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return moving & (nb >= min_nb)


def components(kept, conn=8, label="min"):
    """-> labels [Hg, Wg] int64: -1, or the least (label "max": the mutation, the largest) row-major index of the cell's
    component under 8-connectivity (conn 4: the mutation). A flood fill from every unvisited kept cell in row-major order"""
    H, W = kept.shape
    lab = np.full((H, W), -1, np.int64)
    nbrs = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn == 8 else [])
    for j0 in range(H):
        for i0 in range(W):
            if not kept[j0, i0] or lab[j0, i0] >= 0:
                continue
            cells, todo = [], [(j0, i0)]
            lab[j0, i0] = 0
            while todo:
                j, i = todo.pop()
                cells.append((j, i))
                for dj, di in nbrs:
                    v, u = j + dj, i + di
                    if 0 <= v < H and 0 <= u < W and kept[v, u] and lab[v, u] < 0:
                        lab[v, u] = 0
                        todo.append((v, u))
            idx = [j * W + i for j, i in cells]
            for j, i in cells:
                lab[j, i] = max(idx) if label == "max" else min(idx)
    return lab


def listing(lab, c, min_area, max_n, ties="label"):
    """-> (components, [dict(box=(x, y, w, h), area, label)]): by area descending, then label ascending (ties "reverse": the
    mutation, label descending)"""
    out = []
    for l in np.unique(lab[lab >= 0]):
        jj, ii = np.nonzero(lab == l)
        out.append(dict(box=(int(ii.min()) * c, int(jj.min()) * c, int(ii.max() - ii.min() + 1) * c, int(jj.max() - jj.min() + 1) * c),
                        area=int(jj.size), label=int(l)))
    n = len(out)
    out = [o for o in out if o["area"] >= min_area]
    out.sort(key=lambda o: (-o["area"], -o["label"] if ties == "reverse" else o["label"]))
    return n, out[:max_n]


def own_rect(box, c, Wg, Hg):
    """the cells of the committed box: corners floored (left, top) and ceiled (right, bottom), clipped to the grid; binary32"""
    x, y, w, h = (np.float32(v) for v in box)
    inv = np.float32(1.0) / np.float32(c)
    clip = lambda v, hi: int(min(max(float(v), 0.0), float(hi)))      # noqa: E731
    x0, y0 = clip(np.floor(x * inv), Wg), clip(np.floor(y * inv), Hg)
    x1, y1 = clip(np.ceil(np.float32(x + w) * inv), Wg), clip(np.ceil(np.float32(y + h) * inv), Hg)
    return x0, y0, max(x1, x0), max(y1, y0)


class Stream:
    """one stream's side of the rule: the background and its bookkeeping, still, the counters, and one pass at a time"""

    def __init__(self):
        self.has_bg, self.geom = 0, None
        self.bg = self.thumb = self.mask = self.labels = None
        self.still = 0
        self.evaluated = self.listed = 0
        self.rec = None             # the last record written (a pass that is not due writes none)

    def reset(self):        # init, import, the destination of a copy, "movers" 0
        self.has_bg = self.still = 0
        self.rec = None

    def step(self, rgb, box=(0, 0, 0, 0), cell=0, max_cells=65536, device=True, whole=True, **kw):
        """one pass that lists the stream (its first slot). rgb: [H, W, 3] integers as the pixel fetch reads the frame"""
        H, W = rgb.shape[:2]
        g = geometry(W, H, cell, max_cells) if device and whole else dict(status=4, c=0, Wg=0, Hg=0)
        t = thumbnail(rgb, g["c"], g["Wg"], g["Hg"]) if g["status"] == 1 else None
        return self.step_thumb(t, g, (W, H), box, **kw)

    def step_thumb(self, t, g, size=(0, 0), box=(0, 0, 0, 0), on=1, period=1, learn=4, thr=96, min_nb=3, min_area=4, global_pm=400,
                   max_n=4, initialised=True, frames_done=0, **mut):
        """the pass from the thumbnail t [Hg, Wg] on (None: g["status"] is 2 or 4). g: dict(status, c, Wg, Hg). -> the record as
        a dict with boxes, thumb, bg, mask (0 / 1 / 2), labels and the counters; status 0: dict(status=0) and nothing changes.
        mut: ge (>= at the threshold), conn (4), label ("max"), ties ("reverse"), outside (cells beyond the border count as
        moving), update_first (the mask from the updated background)"""
        if not (on and initialised and frames_done % period == 0):
            return dict(status=0)
        rec = dict(status=g["status"], frames_done=frames_done, c=g["c"], Wg=g["Wg"], Hg=g["Hg"], n=0, moving=0, kept=0, components=0,
                   own_cells=0, own_kept=0, still=0, boxes=[], thumb=None, bg=None, mask=None, labels=None)
        if rec["status"] != 1:
            self.has_bg = self.still = 0
            return self._done(rec)
        geom = (size[0], size[1], g["c"])
        t = np.asarray(t, np.int64)
        prev_ok = bool(self.has_bg) and self.geom == geom
        self.has_bg, self.geom, self.thumb = 1, geom, t
        if not prev_ok:
            rec["status"] = 5
            self.bg, self.mask, self.still = 16 * t, np.zeros(t.shape, np.uint8), 0
            rec.update(thumb=t, bg=self.bg, mask=self.mask)
            return self._done(rec)
        d = difference(t, self.bg)
        new_bg = updated(self.bg, d, learn)
        moving = moving_mask(difference(t, new_bg) if mut.get("update_first") else d, thr, ge=mut.get("ge", False))
        kept = clean(moving, min_nb, outside=mut.get("outside", False))
        self.bg = new_bg
        self.mask = moving.astype(np.uint8) + kept.astype(np.uint8)
        x0, y0, x1, y1 = own_rect(box, g["c"], g["Wg"], g["Hg"])
        rec.update(moving=int(moving.sum()), kept=int(kept.sum()), own_cells=(x1 - x0) * (y1 - y0), own_kept=int(kept[y0:y1, x0:x1].sum()),
                   thumb=t, bg=self.bg, mask=self.mask)
        self.evaluated += 1
        if rec["moving"] * 1000 > global_pm * g["Wg"] * g["Hg"]:
            rec["status"], self.still, self.labels = 6, 0, None
            return self._done(rec)
        self.labels = components(kept, conn=mut.get("conn", 8), label=mut.get("label", "min"))
        rec["components"], rec["boxes"] = listing(self.labels, g["c"], min_area, max_n, ties=mut.get("ties", "label"))
        rec["n"], rec["labels"] = len(rec["boxes"]), self.labels
        self.listed += rec["n"]
        self.still = min(self.still + 1, STILL_CAP) if rec["own_kept"] == 0 and rec["kept"] > 0 else 0
        rec["still"] = self.still
        return self._done(rec)

    def _done(self, rec):
        rec["evaluated"], rec["listed"], rec["has_bg"] = self.evaluated, self.listed, self.has_bg
        self.rec = rec
        return rec


# ---- pictures ---------------------------------------------------------------------------------------------------------

def paint(cells, c, base=60, value=200):
    """a grey picture of cells.shape * c pixels: `base`, and `value` in the cells that are set. A uniform grey cell of v has
    the thumbnail value 16 v (sixteen taps of luma v)"""
    cells = np.asarray(cells)
    v = np.where(cells.astype(bool), value, base).astype(np.uint8)
    return np.repeat(np.repeat(v, c, 0), c, 1)[:, :, None].repeat(3, 2)


def parse(rows):
    """a mask from rows of '#' and '.'"""
    return np.array([[ch == "#" for ch in r] for r in rows])


SPIRAL = parse(["#########",        # two turns, one 8-connected (and 4-connected) component
                "........#",
                "#######.#",
                "#.....#.#",
                "#.###.#.#",
                "#.#...#.#",
                "#.#####.#",
                "#.......#",
                "#########"])
U_SHAPE = parse(["#...#",
                 "#...#",
                 "#...#",
                 "#####"])
COMB = parse(["#.#.#.#.#.#",         # the teeth meet in the LAST row only: labels must travel up every tooth
              "#.#.#.#.#.#",
              "#.#.#.#.#.#",
              "###########"])


def serpentine(Hg, Wg):
    """one 4-connected path through the whole grid: full rows 0, 2, 4, ... joined alternately at the right and left ends"""
    m = np.zeros((Hg, Wg), bool)
    m[0::2] = True
    for k, j in enumerate(range(1, Hg - 1, 2)):
        m[j, Wg - 1 if k % 2 == 0 else 0] = True
    return m


def place(shape, Hg, Wg, j=0, i=0):
    m = np.zeros((Hg, Wg), bool)
    m[j:j + shape.shape[0], i:i + shape.shape[1]] = shape
    return m


# ---- the operator hook's outputs against the model (GPU tests) -----------------------------------------------------------

def check_record(rec, want, tag=""):
    for k in REC_FIELDS:
        assert int(rec[k]) == int(want[k]), (tag, k, int(rec[k]), int(want[k]))
    assert int(rec["has_bg"]) == want["has_bg"], tag
    for k in range(MAX_BOXES):
        e = rec["box"][k]
        got = (int(e["x"]), int(e["y"]), int(e["w"]), int(e["h"]), int(e["area"]), int(e["label"]))
        b = want["boxes"][k] if k < want["n"] else None
        assert got == ((*b["box"], b["area"], b["label"]) if b else (0,) * 6), (tag, k, got, b)


def check_stream(got, stream, want, model, before):
    """the hook's outputs of one worked stream against step()'s dict and the Stream behind it, value for value. before: the
    call's inputs (dict of bg, mask, records, counts) - what a launch must leave alone equals them byte for byte"""
    rec, cnt = got["records"][stream], got["counts"][stream]
    if want["status"] == 0:
        for k in ("bg", "mask", "records", "counts"):
            assert got[k][stream].tobytes() == before[k][stream].tobytes(), (stream, k)
        for k in ("accs", "thumbs", "labels", "exts"):
            assert (got[k][stream] == -1).all() or (got[k][stream] == 0xFFFF).all(), (stream, k)
        return
    check_record(rec, want, stream)
    assert (int(cnt["evaluated"]), int(cnt["listed"])) == (want["evaluated"], want["listed"]), (stream, cnt)
    assert cnt["reserved"].tobytes() == before["counts"][stream]["reserved"].tobytes(), stream
    if want["thumb"] is None:       # statuses 2 and 4
        for k in ("bg", "mask"):
            assert got[k][stream].tobytes() == before[k][stream].tobytes(), (stream, k)
        assert (got["thumbs"][stream] == 0xFFFF).all() and (got["accs"][stream] == -1).all() and (got["labels"][stream] == -1).all()
        return
    Wg, Hg = want["Wg"], want["Hg"]
    n = Wg * Hg
    assert (int(rec["pW"]), int(rec["pH"]), int(rec["pc"])) == model.geom, stream
    assert np.array_equal(got["thumbs"][stream, :n].reshape(Hg, Wg), want["thumb"]), stream
    assert np.array_equal(got["bg"][stream, :n].reshape(Hg, Wg), want["bg"]), stream
    assert np.array_equal(got["mask"][stream, :n].reshape(Hg, Wg), want["mask"]), stream
    assert (got["thumbs"][stream, n:] == 0xFFFF).all(), stream
    for k in ("bg", "mask"):
        assert got[k][stream, n:].tobytes() == before[k][stream, n:].tobytes(), (stream, k)
    assert (got["labels"][stream, n:] == -1).all() and (got["exts"][stream, :, n:] == -1).all(), stream
    if want["status"] == 5:
        assert got["accs"][stream].tolist() == [0, 0, -1, -1] and (got["labels"][stream] == -1).all(), stream
        return
    assert got["accs"][stream].tolist() == [want["moving"], want["kept"], -1, -1], stream
    if want["status"] == 6:         # the labels' start ran, nothing was merged: a kept cell points at itself or to its left
        lab, own = got["labels"][stream, :n].reshape(Hg, Wg), np.arange(n).reshape(Hg, Wg)
        assert np.array_equal(lab >= 0, want["mask"] == 2) and (lab <= own).all() and (lab[lab >= 0] // Wg == own[lab >= 0] // Wg).all(), stream
        return
    lab = got["labels"][stream, :n].reshape(Hg, Wg)
    assert np.array_equal(lab, want["labels"]), stream
    ext = got["exts"][stream, :, :n]
    for l in np.unique(want["labels"][want["labels"] >= 0]):
        jj, ii = np.nonzero(want["labels"] == l)
        assert ext[:, l].tolist() == [ii.min(), ii.max(), jj.max(), jj.size], (stream, l)
