"""The NumPy model of the camera motion (include/vittrack_hip_ops.h, vt_op_camera_motion; csrc/k_camera_motion.hip).

Every number of the rule is an exact integer (int64 sums) until the three binary32 operations per axis of the sub-cell
shift, each one np.float32 operation here: the kernels are held to these arrays with np.array_equal. Nothing in here reads
the engine."""
import numpy as np

from proposals_util import DevFrame, FORMATS, from_rgb, to_rgb     # noqa: F401  (the GPU tests' device frames)

F = np.float32
R_MAX = 16
TABLE = (2 * R_MAX + 1) ** 2
SEARCHED = (1, 3, 6, 7)


def auto_cell(W, H, max_cells):
    for c in (4, 8, 16, 32, 64):
        if (W // c) * (H // c) <= max_cells:
            return c
    return 0


def geometry(W, H, cell, R, max_cells):
    """-> dict(status 1 | 2, c, Wg, Hg); c, Wg, Hg are 0 where no cell exists"""
    c = cell if cell else auto_cell(W, H, max_cells)
    g = dict(status=2, c=c, Wg=W // c if c else 0, Hg=H // c if c else 0)
    if c and g["Wg"] * g["Hg"] <= max_cells and g["Wg"] - 2 * R >= 8 and g["Hg"] - 2 * R >= 8:
        g["status"] = 1
    return g


def luma(rgb):
    r, g, b = (np.asarray(rgb[..., k], np.int64) for k in range(3))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def thumbnail(rgb, c, Wg, Hg):
    """[Hg, Wg] uint16: the sum of sixteen integer lumas per cell, taps at i * c + u * (c / 4) + c / 8"""
    Y = luma(rgb)
    tx = (np.arange(Wg)[:, None] * c + np.arange(4)[None, :] * (c // 4) + c // 8)        # [Wg, 4]
    ty = (np.arange(Hg)[:, None] * c + np.arange(4)[None, :] * (c // 4) + c // 8)
    assert tx.max() < rgb.shape[1] and ty.max() < rgb.shape[0]
    s = np.zeros((Hg, Wg), np.int64)
    for v in range(4):
        for u in range(4):
            s += Y[ty[:, v][:, None], tx[:, u][None, :]]
    return s.astype(np.uint16)


def sad_table(cur, prev, R, sign=1):
    """[2R + 1, 2R + 1] int64, row dy + R, column dx + R: S(dx, dy) = sum over the central cells of |cur(i, j) - prev(i - dx,
    j - dy)|. sign -1: the mutation prev(i + dx, j + dy)"""
    Hg, Wg = cur.shape
    c, p = cur.astype(np.int64), prev.astype(np.int64)
    S = np.zeros((2 * R + 1, 2 * R + 1), np.int64)
    mid = c[R:Hg - R, R:Wg - R]
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sy, sx = R - sign * dy, R - sign * dx
            S[dy + R, dx + R] = np.abs(mid - p[sy:sy + Hg - 2 * R, sx:sx + Wg - 2 * R]).sum()
    return S


def decide(S, R, c, conf_pm, tie="small", s2_dist=1):
    """the table -> dict(status, dx, dy, S_best, S0, S2, off [2] float32, shift [2] float32). tie "index": the mutation that
    drops the squared length from the order; s2_dist 0: the mutation that excludes the best displacement alone"""
    side = 2 * R + 1
    ys, xs = np.mgrid[0:side, 0:side]
    r2 = (xs - R) ** 2 + (ys - R) ** 2
    idx = ys * side + xs
    keys = (idx.ravel(), r2.ravel() if tie == "small" else np.zeros(side * side, np.int64), S.ravel())
    best = int(np.lexsort(keys)[0])     # the last key is the primary one
    by, bx = divmod(best, side)
    dx, dy = bx - R, by - R
    Sb = int(S[by, bx])
    far = np.maximum(np.abs(xs - bx), np.abs(ys - by)) > s2_dist
    S2 = int(S[far].min())
    out = dict(status=1, dx=dx, dy=dy, S_best=Sb, S0=int(S[R, R]), S2=S2, off=np.zeros(2, F), shift=np.zeros(2, F))
    if S2 == 0:
        out["status"] = 3
    elif abs(dx) == R or abs(dy) == R:
        out["status"] = 6
    elif Sb * 1000 > conf_pm * S2:
        out["status"] = 7
    if out["status"] == 1:
        nb = ((int(S[by, bx - 1]), int(S[by, bx + 1])), (int(S[by - 1, bx]), int(S[by + 1, bx])))
        for k, (Sm, Sp) in enumerate(nb):
            den = Sm - 2 * Sb + Sp
            num = F(0.5) * F(np.int64(Sm - Sp))
            off = num / F(np.int64(den)) if den > 0 and Sb > 0 else F(0)      # an exact match is a whole-cell shift
            out["off"][k] = off
            out["shift"][k] = (F((dx, dy)[k]) + off) * F(c)
    return out


def apply_shift(box, shift, frame_w, frame_h):
    """the place rule of the motion prior on (x + shift_x, y + shift_y): -> (box [4] float32, applied)"""
    b = np.asarray(box, F).copy()
    if shift[0] == 0 and shift[1] == 0:
        return b, 0
    px, py = b[0] + F(shift[0]), b[1] + F(shift[1])
    cx, cy = px + F(0.5) * b[2], py + F(0.5) * b[3]
    if 0 <= cx < F(frame_w) and 0 <= cy < F(frame_h):
        b[0], b[1] = px, py
        return b, 1
    return b, 0


class Stream:
    """one stream's side of the rule: the thumbnails' bookkeeping, the counters, and one pass at a time"""

    def __init__(self):
        self.has_prev, self.cur, self.geom = 0, 0, None
        self.thumbs = [None, None]
        self.evaluated = self.moved = 0

    def reset(self):        # init, import, the destination of a copy
        self.has_prev = 0

    def step(self, rgb, box, mode=2, cell=0, R=8, conf_pm=800, max_cells=65536, frame=None, initialised=True, device=True,
             whole=True, frames_done=0, **mut):
        """one pass that lists the stream (its first slot). rgb: [H, W, 3] integers as the pixel fetch reads the frame; box:
        the state box; frame: (frame_w, frame_h) of the state (None: the picture's). -> the record as a dict, with "box" (the
        box behind the decision), "thumb" (the thumbnail taken, or None) and "sad" (the table, or None)"""
        H, W = rgb.shape[:2]
        fw, fh = frame or (W, H)
        rec = dict(status=0, frames_done=frames_done, c=0, Wg=0, Hg=0, R=R, dx=0, dy=0, shift=np.zeros(2, F), applied=0, n=0,
                   S_best=0, S0=0, S2=0, box=np.asarray(box, F).copy(), thumb=None, sad=None)
        status = 1 if mode != 0 and initialised else 0
        if status == 1 and not (device and whole):
            status = 4
        if status == 1:
            g = geometry(W, H, cell, R, max_cells)
            rec.update(c=g["c"], Wg=g["Wg"], Hg=g["Hg"])
            status = g["status"]
        if status != 1:
            self.has_prev = 0
            rec["status"] = status
            return self._count(rec)
        geom = (W, H, rec["c"])
        prev_ok = self.has_prev and self.geom == geom
        cur = (self.cur ^ 1) if self.has_prev else 0
        prev = self.thumbs[cur ^ 1]
        self.thumbs[cur] = rec["thumb"] = thumbnail(rgb, rec["c"], rec["Wg"], rec["Hg"])
        self.has_prev, self.cur, self.geom = 1, cur, geom
        if not prev_ok:
            rec["status"] = 5
            return self._count(rec)
        S = sad_table(rec["thumb"], prev, R, sign=mut.get("sign", 1))
        d = decide(S, R, rec["c"], conf_pm, tie=mut.get("tie", "small"), s2_dist=mut.get("s2_dist", 1))
        rec.update(sad=S, n=(rec["Wg"] - 2 * R) * (rec["Hg"] - 2 * R), **{k: d[k] for k in ("status", "dx", "dy", "S_best", "S0", "S2", "shift")})
        rec["off"] = d["off"]
        if mode == 2 and rec["status"] == 1:
            rec["box"], rec["applied"] = apply_shift(box, rec["shift"], fw, fh)
        return self._count(rec)

    def _count(self, rec):
        self.evaluated += rec["status"] in SEARCHED
        self.moved += rec["applied"]
        rec["evaluated"], rec["moved"] = self.evaluated, self.moved
        return rec


# ---- pictures ---------------------------------------------------------------------------------------------------------

def texture(h, w, seed, smooth=3):
    """an [h, w, 3] uint8 canvas: noise smoothed over `smooth` pixels (box filter), stretched to the whole range"""
    rng = np.random.default_rng(seed)
    a = rng.random((h + 2 * smooth, w + 2 * smooth, 3))
    if smooth:
        k = 2 * smooth + 1
        cs = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0), (0, 0))), 0), 1)
        a = (cs[k:, k:] - cs[:-k, k:] - cs[k:, :-k] + cs[:-k, :-k]) / (k * k)
        a = a[:h, :w]
    else:
        a = a[:h, :w]
    a = (a - a.min()) / max(a.max() - a.min(), 1e-9)
    return np.clip(np.rint(a * 255), 0, 255).astype(np.uint8)


def view(canvas, x, y, w, h):
    """the [h, w, 3] window of the canvas with its top-left corner at (x, y): content moves by -(x, y)"""
    assert 0 <= x and x + w <= canvas.shape[1] and 0 <= y and y + h <= canvas.shape[0], (x, y, w, h, canvas.shape)
    return canvas[y:y + h, x:x + w]


# ---- the operator hook's outputs against the model (GPU tests) -----------------------------------------------------------

REC_FIELDS = ("status", "frames_done", "c", "Wg", "Hg", "R", "dx", "dy", "applied", "n", "S_best", "S0", "S2", "evaluated", "moved")


def check_stream(got, stream, want, model, max_cells):
    """the hook's outputs of one worked stream against step()'s dict and the Stream behind it, bit for bit"""
    rec = got["records"][stream]
    for k in REC_FIELDS:
        assert int(rec[k]) == int(want[k]), (stream, k, int(rec[k]), int(want[k]))
    assert rec["shift"].tobytes() == np.asarray(want["shift"], F).tobytes(), (stream, rec["shift"], want["shift"])
    assert (int(rec["has_prev"]), int(rec["cur"])) == (model.has_prev, model.cur) or not model.has_prev and not rec["has_prev"], stream
    assert got["states"][stream]["box"].tobytes() == np.asarray(want["box"], F).tobytes(), (stream, got["states"][stream]["box"], want["box"])
    if want["thumb"] is not None:
        n = want["Wg"] * want["Hg"]
        assert np.array_equal(got["thumbs"][stream, model.cur, :n].reshape(want["Hg"], want["Wg"]), want["thumb"]), stream
        assert (int(rec["pW"]), int(rec["pH"]), int(rec["pc"])) == model.geom, stream
    side = 2 * want["R"] + 1
    if want["sad"] is not None:
        assert np.array_equal(got["sad"][stream, :side * side].reshape(side, side), want["sad"]), stream
        assert (got["sad"][stream, side * side:] == -1).all(), stream
    else:
        assert (got["sad"][stream] == -1).all(), stream
