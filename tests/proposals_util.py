"""The NumPy model of the reacquire proposals (include/vittrack_hip.h, the "proposals*" keys; csrc/k_proposals.hip).

Every binary32 operation of the rule is one np.float32 operation here, every integer sum an int64 sum, the similarity
three binary64 operations: the kernels are held to these arrays with np.array_equal. Nothing in here reads the engine."""
import numpy as np

F = np.float32
MAX_PROPOSALS = 8
MAX_GRID = 4194304
REC_DTYPE = np.dtype([("sim", "<f4"), ("box", "<f4", 4), ("pos", "<i4")])
FORMATS = ("rgb8", "nv12", "yuy2", "bgrx", "i420", "gray8", "p010")


# ---- pixels ---------------------------------------------------------------------------------------------------------

def _yuv_to_rgb(y, u, v):
    y, u, v = (np.asarray(a, np.int64) for a in (y, u, v))
    yv = 298 * (y - 16)
    r = yv + 409 * (v - 128) + 128
    g = yv - 100 * (u - 128) - 208 * (v - 128) + 128
    b = yv + 516 * (u - 128) + 128
    return np.stack([np.clip(c, 0, 0xffff) >> 8 for c in (r, g, b)], -1)


def frame_bytes(fmt, w, h):
    cw, ch = (w + 1) // 2, (h + 1) // 2
    return {"rgb8": 3 * w * h, "bgrx": 4 * w * h, "gray8": w * h, "yuy2": 2 * w * h, "nv12": w * h + 2 * cw * ch,
            "i420": w * h + 2 * cw * ch, "p010": 2 * w * h + 4 * cw * ch}[fmt]


def planes(fmt, w, h):
    """(row bytes, rows) of every plane of a packed buffer, in buffer order"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt == "nv12":
        return [(w, h), (2 * cw, ch)]
    if fmt == "i420":
        return [(w, h), (cw, ch), (cw, ch)]
    if fmt == "p010":
        return [(2 * w, h), (4 * cw, ch)]
    return [(frame_bytes(fmt, w, h) // h, h)]


def to_rgb(fmt, buf, w, h):
    """[h, w, 3] integer RGB of a packed frame buffer, as the library's pixel fetch reads it"""
    b = np.asarray(buf, np.uint8).reshape(-1)
    assert b.size == frame_bytes(fmt, w, h), (fmt, b.size, w, h)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    xs, ys = np.arange(w), np.arange(h)
    if fmt == "rgb8":
        return b.reshape(h, w, 3).astype(np.int64)
    if fmt == "bgrx":
        return b.reshape(h, w, 4)[:, :, 2::-1].astype(np.int64)
    if fmt == "gray8":
        return np.repeat(b.reshape(h, w, 1), 3, 2).astype(np.int64)
    if fmt == "yuy2":
        p = b.reshape(h, w // 2, 4)
        y = p[:, :, (0, 2)].reshape(h, w)
        return _yuv_to_rgb(y, np.repeat(p[:, :, 1], 2, 1), np.repeat(p[:, :, 3], 2, 1))
    if fmt == "nv12":
        y = b[:w * h].reshape(h, w)
        uv = b[w * h:].reshape(ch, cw, 2)
        return _yuv_to_rgb(y, uv[ys[:, None] // 2, xs[None, :] // 2, 0], uv[ys[:, None] // 2, xs[None, :] // 2, 1])
    if fmt == "i420":
        y = b[:w * h].reshape(h, w)
        u = b[w * h:w * h + cw * ch].reshape(ch, cw)
        v = b[w * h + cw * ch:].reshape(ch, cw)
        return _yuv_to_rgb(y, u[ys[:, None] // 2, xs[None, :] // 2], v[ys[:, None] // 2, xs[None, :] // 2])
    if fmt == "p010":       # the high byte of every little-endian 16-bit sample
        y = b[:2 * w * h].reshape(h, w, 2)[:, :, 1]
        uv = b[2 * w * h:].reshape(ch, cw, 2, 2)[:, :, :, 1]
        return _yuv_to_rgb(y, uv[ys[:, None] // 2, xs[None, :] // 2, 0], uv[ys[:, None] // 2, xs[None, :] // 2, 1])
    raise ValueError(fmt)


def from_rgb(fmt, rgb, rng=None):
    """a packed buffer of `fmt` that shows (about) the [h, w, 3] uint8 picture: the tests' way to one scene in every format"""
    rgb = np.asarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if fmt == "rgb8":
        return rgb.reshape(-1).copy()
    if fmt == "bgrx":
        return np.concatenate([rgb[:, :, ::-1], np.full((h, w, 1), 0x5a, np.uint8)], 2).reshape(-1)
    f = rgb.astype(np.float64)
    y = np.clip(np.rint(16 + 0.257 * f[..., 0] + 0.504 * f[..., 1] + 0.098 * f[..., 2]), 0, 255).astype(np.uint8)
    if fmt == "gray8":
        return y.reshape(-1)
    u = np.clip(np.rint(128 - 0.148 * f[..., 0] - 0.291 * f[..., 1] + 0.439 * f[..., 2]), 0, 255).astype(np.uint8)
    v = np.clip(np.rint(128 + 0.439 * f[..., 0] - 0.368 * f[..., 1] - 0.071 * f[..., 2]), 0, 255).astype(np.uint8)
    if fmt == "yuy2":
        out = np.empty((h, w // 2, 4), np.uint8)
        out[:, :, 0], out[:, :, 2] = y[:, 0::2], y[:, 1::2]
        out[:, :, 1], out[:, :, 3] = u[:, 0::2], v[:, 0::2]
        return out.reshape(-1)
    us, vs = np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.uint8)
    us[:, :] = u[0::2, 0::2]
    vs[:, :] = v[0::2, 0::2]
    if fmt == "nv12":
        return np.concatenate([y.reshape(-1), np.stack([us, vs], -1).reshape(-1)])
    if fmt == "i420":
        return np.concatenate([y.reshape(-1), us.reshape(-1), vs.reshape(-1)])
    if fmt == "p010":
        rng = rng or np.random.default_rng(0)
        lo = lambda a: rng.integers(0, 4, a.shape).astype(np.uint8) << 6     # the low bytes are never read
        y16 = np.stack([lo(y), y], -1)
        uv = np.stack([us, vs], -1)
        return np.concatenate([y16.reshape(-1), np.stack([lo(uv), uv], -1).reshape(-1)])
    raise ValueError(fmt)


# ---- template rows --------------------------------------------------------------------------------------------------

def f32_to_bf16_bits(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f64(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def rows_from_template(tpl, patch, kpad):
    """[T, T, 3] float values -> the [nt, kpad] bf16 bit patterns of template rows (patch-row layout, pad columns zero)"""
    T = tpl.shape[0]
    gt = T // patch
    rows = np.zeros((gt * gt, kpad), np.uint16)
    t = f32_to_bf16_bits(tpl).reshape(gt, patch, gt, patch, 3)        # ty, py, tx, px, c
    rows[:, :3 * patch * patch] = t.transpose(0, 2, 4, 1, 3).reshape(gt * gt, 3 * patch * patch)
    return rows


def template_from_rows(rows, T, patch):
    """the inverse: [T, T, 3] binary64, every value the exact value of its bf16"""
    gt = T // patch
    v = bf16_bits_to_f64(np.asarray(rows)[:, :3 * patch * patch]).reshape(gt, gt, 3, patch, patch)
    return v.transpose(0, 3, 1, 4, 2).reshape(T, T, 3)


def crop_template(rgb, box, T, norm_a, norm_b):
    """a factor-2 template crop for the model's own cases: nearest sampling of the (x, y, w, h) box's context square,
    normalised. It is NOT the library's crop - the CPU cases only need rows that show the planted picture."""
    x, y, w, h = box
    s = float(np.sqrt(w * h)) * 2.0
    cx, cy = x + 0.5 * w, y + 0.5 * h
    H, W, _ = rgb.shape
    idx = (np.arange(T) + 0.5) * (s / T)
    px = np.floor(cx - 0.5 * s + idx).astype(int)
    py = np.floor(cy - 0.5 * s + idx).astype(int)
    ok = ((px >= 0) & (px < W))[None, :] & ((py >= 0) & (py < H))[:, None]
    pix = np.where(ok[..., None], rgb[np.clip(py, 0, H - 1)[:, None], np.clip(px, 0, W - 1)[None, :]], 0).astype(np.float32)
    return pix * np.asarray(norm_a, F) + np.asarray(norm_b, F)


# ---- the rule -------------------------------------------------------------------------------------------------------

def pattern_side(T):
    return 16 if T % 16 == 0 else 14 if T % 14 == 0 else 0


def pattern(rows, T, patch):
    """[M, M] int16 from template rows: binary64 sums in ascending (y, x, channel) order"""
    M = pattern_side(T)
    blk = T // M
    t = template_from_rows(rows, T, patch).reshape(M, blk, M, blk, 3).transpose(0, 2, 1, 3, 4).reshape(M, M, blk * blk * 3)
    s = np.zeros((M, M), np.float64)
    for k in range(t.shape[2]):
        s = s + t[:, :, k]
    return np.clip(np.rint(s * (4096.0 / (3 * blk * blk))), -32767, 32767).astype(np.int16)


def geometry(box, frame_w, frame_h, M, max_cells):
    """-> dict(status 1 | 2, c, X0, Wg, Hg): binary32 throughout"""
    w, h = F(box[2]), F(box[3])
    with np.errstate(all="ignore"):
        s = np.sqrt(w * h)
        c = F(2.0) * s / F(M)
        qw, qh = F(frame_w) / c, F(frame_h) / c
    g = dict(status=2, c=F(0), X0=F(0), Wg=0, Hg=0)
    if c > 0 and qw <= F(MAX_GRID) and qh <= F(MAX_GRID):
        Wg, Hg = int(np.ceil(qw)) + M // 2, int(np.ceil(qh)) + M // 2
        g.update(c=c, X0=-F(M // 4) * c, Wg=Wg, Hg=Hg)
        if Wg * Hg <= max_cells and Wg >= M and Hg >= M:
            g["status"] = 1
    return g


OUTSIDE = -32768        # the thumbnail's mark of a cell with a sub-tap outside the frame: no value clamps to it


def thumbnail(rgb, g, norm_a, norm_b):
    """[Hg, Wg] int16: sixteen sub-taps per cell, binary32 sums in (v, u) order; OUTSIDE where any sub-tap leaves the frame"""
    H, W, _ = rgb.shape
    na, nb = np.asarray(norm_a, F), np.asarray(norm_b, F)
    px3 = np.zeros((H + 1, W + 1, 3), F)           # the last row and column: black, for every tap outside the frame
    px3[:H, :W] = rgb
    G = (px3[..., 0] * na[0] + nb[0]) + (px3[..., 1] * na[1] + nb[1]) + (px3[..., 2] * na[2] + nb[2])
    c, X0 = g["c"], g["X0"]

    def taps(n, size):
        i = np.arange(n, dtype=F)[:, None]
        u = ((np.arange(4, dtype=F) + F(0.5)) * F(0.25))[None, :]
        p = np.floor(X0 + (i + u) * c).astype(np.int64)         # [n, 4]
        inside = (p >= 0) & (p < size)
        return np.where(inside, p, size), inside.all(axis=1)
    (tx, vx), (ty, vy) = taps(g["Wg"], W), taps(g["Hg"], H)
    s = np.zeros((g["Hg"], g["Wg"]), F)
    for v in range(4):
        for u in range(4):
            s = s + G[ty[:, v][:, None], tx[:, u][None, :]]
    q = np.clip(np.rint(s * (F(4096.0) / F(48.0))), F(-32767), F(32767)).astype(np.int16)
    return np.where(vy[:, None] & vx[None, :], q, np.int16(OUTSIDE))


def similarity_map(Q, A):
    """[Hg - M + 1, Wg - M + 1] float32 from exact int64 sums over the window's cells INSIDE the frame -> (map, va of the
    whole pattern)"""
    M = A.shape[0]
    q, a = Q.astype(np.int64), A.astype(np.int64)
    Ph, Pw = Q.shape[0] - M + 1, Q.shape[1] - M + 1
    n, Sa, Saa, Sp, Spp, Sap = (np.zeros((Ph, Pw), np.int64) for _ in range(6))
    for y in range(M):
        for x in range(M):
            w = q[y:y + Ph, x:x + Pw]
            v = (w != OUTSIDE).astype(np.int64)
            w = w * v
            n += v
            Sa += a[y, x] * v
            Saa += a[y, x] * a[y, x] * v
            Sp += w
            Spp += w * w
            Sap += a[y, x] * w
    cov, va, vp = n * Sap - Sa * Sp, n * Saa - Sa * Sa, n * Spp - Sp * Sp
    ok = (va > 0) & (vp > 0)
    with np.errstate(all="ignore"):
        sim = np.where(ok, cov.astype(np.float64) / np.sqrt(np.where(ok, va.astype(np.float64) * vp.astype(np.float64), 1.0)), 0.0)
    return np.clip(sim, -1.0, 1.0).astype(F), M * M * int((a * a).sum()) - int(a.sum()) ** 2


def listing(smap, M, g, box, max_n, tau):
    """the listed proposals, best first: REC_DTYPE records"""
    Ph, Pw = smap.shape
    R = M // 2
    open_ = np.ones(smap.shape, bool)
    out = []
    ys, xs = np.mgrid[0:Ph, 0:Pw]
    for _ in range(min(max_n, MAX_PROPOSALS)):
        if not open_.any():
            break
        cand = np.where(open_, smap, F(-2))
        pos = int(np.argmax(cand))          # the first of the greatest: the lowest position
        s = cand.reshape(-1)[pos]
        if not (s >= F(tau) and s > 0):
            break
        py, px = divmod(pos, Pw)
        cx = g["X0"] + F(px + R) * g["c"]
        cy = g["X0"] + F(py + R) * g["c"]
        w, h = F(box[2]), F(box[3])
        out.append((s, (cx - F(0.5) * w, cy - F(0.5) * h, w, h), pos))
        open_ &= (np.abs(xs - px) > R) | (np.abs(ys - py) > R)
    return np.array(out, REC_DTYPE) if out else np.zeros(0, REC_DTYPE)


def due_status(mode, period, success, frames_done, winner_ok=True, device=True, whole=True):
    due = mode != 0 and winner_ok and (mode == 2 or not success) and frames_done % period == 0
    return 0 if not due else 1 if device and whole else 4


def evaluate(rgb, box, rows, T, patch, norm_a, norm_b, max_cells=262144, max_n=4, min_sim_pm=500):
    """a due slot with a whole device frame -> dict(status, c, Wg, Hg, pattern, thumb, map, proposals)"""
    M = pattern_side(T)
    H, W, _ = rgb.shape
    g = geometry(box, W, H, M, max_cells)
    out = dict(status=g["status"], c=g["c"], Wg=g["Wg"], Hg=g["Hg"], pattern=None, thumb=None, map=None,
               proposals=np.zeros(0, REC_DTYPE), M=M, X0=g["X0"])
    if g["status"] != 1:
        return out
    A = pattern(rows, T, patch)
    out["pattern"] = A
    a = A.astype(np.int64)
    if M * M * int((a * a).sum()) - int(a.sum()) ** 2 == 0:
        out["status"] = 3
        return out
    Q = thumbnail(rgb, g, norm_a, norm_b)
    smap, _ = similarity_map(Q, A)
    tau = F(min_sim_pm) / F(1000.0)
    out.update(thumb=Q, map=smap, proposals=listing(smap, M, g, box, max_n, tau))
    return out


# ---- device frames and the operator hook's operands (GPU tests) ------------------------------------------------------

class DevFrame:
    """a packed frame of `fmt` in device memory and its vt_frame with DEVICE planes"""

    def __init__(self, gpu, fmt, buf, w, h):
        import torch
        self.fmt, self.w, self.h = fmt, w, h
        host = np.ascontiguousarray(buf, np.uint8).reshape(-1)
        assert host.size == frame_bytes(fmt, w, h)
        self.rgb = to_rgb(fmt, host, w, h)
        self.t = torch.from_numpy(host.copy()).cuda()
        pl = planes(fmt, w, h)
        base = self.t.data_ptr()
        p1 = base + pl[0][0] * pl[0][1] if len(pl) > 1 else None
        self.frame = gpu.CFrame(base, p1, w, h, pl[0][0], pl[1][0] if len(pl) > 1 else 0, getattr(gpu, "PIX_" + fmt.upper()),
                                0, 0, 0, 0, 0)


def check_slot(got, slot, stream, want, max_cells):
    """the hook's outputs of one slot against evaluate()'s dict, bit for bit; what the launches left alone is 0xff bytes"""
    M = want["M"]
    rec = got["records"][stream]
    assert rec["status"] == want["status"], (slot, rec["status"], want["status"])
    pat, th, mp = got["pattern"][slot], got["thumb"][slot], got["map"][slot].view(np.uint32)
    np_, nt_, nm_ = 0, 0, 0
    if want["status"] in (1, 2, 3):
        assert rec["c"].tobytes() == np.float32(want["c"]).tobytes() and (rec["Wg"], rec["Hg"]) == (want["Wg"], want["Hg"])
    if want["pattern"] is not None:
        np_ = M * M
        assert np.array_equal(pat[:np_].reshape(M, M), want["pattern"]), slot
    if want["thumb"] is not None:
        nt_ = want["Wg"] * want["Hg"]
        assert np.array_equal(th[:nt_].reshape(want["Hg"], want["Wg"]), want["thumb"]), slot
        nm_ = want["map"].size
        assert np.array_equal(mp[:nm_], want["map"].reshape(-1).view(np.uint32)), slot
    assert (pat[np_:] == -1).all() and (th[nt_:] == -1).all() and (mp[nm_:] == 0xffffffff).all(), slot
    p = want["proposals"]
    assert rec["n"] == len(p), (slot, rec["n"], p)
    for k in ("sim", "box", "pos"):
        assert rec["p"][k][:len(p)].tobytes() == p[k].tobytes(), (slot, k, rec["p"][:len(p)], p)
    assert not np.frombuffer(rec["p"][len(p):].tobytes(), np.uint8).any(), slot
