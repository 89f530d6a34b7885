"""The result overlay's specification restated for the tests (DESIGN.md section 3 "Result overlay"): the command list a
result draws, the gate, and the frame the list leaves - drawn by the EXISTING oracle.vit_ref.draw / draw_rgb.

A frame here is a packed host buffer of one of the formats below (strides equal the row bytes, planes follow each other).
Luma formats other than NV12 lend their Y plane to a packed NV12 buffer for the drawing; the permuted RGB formats go through
their RGB8 sibling (planar_formats_util.py) and keep their pad byte."""
import numpy as np

import planar_formats_util as pf

DEFAULTS = dict(flags=7, thickness=3, size=15, scale=2, luma=255, rgb=0x00FF00, min_score_pct=25)
LUMA = ("nv12", "nv21", "i420", "yv12", "nv16", "yuy2", "uyvy", "gray8")
RGB = ("rgb8", "bgr8", "rgbx", "bgrx", "xrgb", "xbgr")
DRAWABLE = LUMA + RGB


def cdiv2(v):
    """v / 2 in C: truncated towards zero"""
    return int(v / 2)


def label_n(score):
    """N of "score: N%": clamp((int)rintf(score * 100.0f), 0, 100) - one binary32 multiply, ties to even; a NaN gives 0"""
    v = np.rint(np.float32(score) * np.float32(100.0))
    if not v > 0:
        return 0
    return 100 if v >= 100 else int(v)


def draws(success, score, min_score_pct=25):
    """rule 4: success and score > (float)pct / 100.0f; a NaN fails"""
    return bool(success) and bool(np.float32(score) > np.float32(min_score_pct) / np.float32(100.0))


def commands(bbox, score, surface, flags=7, thickness=3, size=15, scale=2, luma=255, rgb=0x00FF00, **_):
    """the ordered list of one slot as oracle.vit_ref.draw / draw_rgb take it: (kind, x, y, w, h, p, value, text)"""
    x, y, w, h = (int(v) for v in bbox)
    value = luma if surface == "luma" else rgb
    out = []
    if flags & 1:
        out.append((2, x, y, w, h, thickness, value, ""))
    if flags & 2:
        out.append((3, x + cdiv2(w), y + cdiv2(h), 0, 0, size, value, ""))
    if flags & 4:
        above = y - 7 * scale - 4
        out.append((1, max(x, 0), above if above >= 0 else y + h + 4, 0, 0, scale, luma, f"score: {label_n(score)}%"))
    return out


def surface(fmt):
    return "luma" if fmt in LUMA else "rgb" if fmt in RGB else None


def frame_bytes(fmt, w, h):
    cw, ch = pf.chroma_dims(w, h)
    return {"nv12": w * h + 2 * cw * ch, "nv21": w * h + 2 * cw * ch, "i420": w * h + 2 * cw * ch, "yv12": w * h + 2 * cw * ch,
            "p010": 2 * (w * h + 2 * cw * ch), "nv16": 2 * w * h, "yuy2": 2 * w * h, "uyvy": 2 * w * h, "gray8": w * h,
            "rgb8": 3 * w * h, "bgr8": 3 * w * h, "rgbx": 4 * w * h, "bgrx": 4 * w * h, "xrgb": 4 * w * h, "xbgr": 4 * w * h}[fmt]


def luma_view(fmt, buf, w, h):
    """writable (h, w) view of the frame's luma bytes"""
    if fmt in ("yuy2", "uyvy"):
        return buf[:2 * w * h].reshape(h, w, 2)[..., 0 if fmt == "yuy2" else 1]
    return buf[:w * h].reshape(h, w)


def rgb_view(fmt, buf, w, h):
    """writable (h, w, 3) view of the frame's R, G, B bytes, in that order"""
    if fmt in ("rgb8", "bgr8"):
        v = buf[:3 * w * h].reshape(h, w, 3)
        return v if fmt == "rgb8" else v[..., ::-1]
    v = buf[:4 * w * h].reshape(h, w, 4)
    return {"rgbx": v[..., 0:3], "bgrx": v[..., 2::-1], "xrgb": v[..., 1:4], "xbgr": v[..., :0:-1]}[fmt]


def expected(oracle, fmt, buf, w, h, slots, **policy):
    """the frame after the pass: `slots` = [(success, score, bbox)] in slot order, every one of them a winner on this frame
    in a device pass; their lists are concatenated in that order. P010 and gated slots leave the bytes alone."""
    pol = dict(DEFAULTS, **policy)
    out = np.array(buf, np.uint8).reshape(-1).copy()
    surf = surface(fmt)
    if surf is None or not pol["flags"]:
        return out
    cmds = []
    for success, score, bbox in slots:
        if draws(success, score, pol["min_score_pct"]):
            cmds += commands(bbox, score, surf, **pol)
    if not cmds:
        return out
    if surf == "luma":
        y = luma_view(fmt, out, w, h)
        cw, ch = pf.chroma_dims(w, h)
        nv12 = np.concatenate([np.ascontiguousarray(y).reshape(-1), np.full(2 * cw * ch, 0x5A, np.uint8)])
        drawn = oracle.draw(nv12, w, h, cmds)
        assert np.all(drawn[w * h:] == 0x5A), "the oracle touched chroma"
        y[...] = drawn[:w * h].reshape(h, w)
    else:
        v = rgb_view(fmt, out, w, h)
        v[...] = oracle.draw_rgb(np.ascontiguousarray(v), cmds)
    return out


def stats_after(slots, flags=7, min_score_pct=25, drawable=True, **_):
    """(drawn, n_drawn, n_gated, n_unsupported, last_n or None) one launch adds for each slot of `slots` (all winners, device pass)"""
    out = []
    for success, score, _bbox in slots:
        if not flags:
            out.append((0, 0, 0, 0, None))
        elif not draws(success, score, min_score_pct):
            out.append((0, 0, 1, 0, None))
        elif not drawable:
            out.append((0, 0, 0, 1, None))
        else:
            out.append((1, 1, 0, 0, label_n(score) if flags & 4 else None))
    return out
