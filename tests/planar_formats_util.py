"""Sibling builders of the vt_pixfmt2 formats, in both directions. Every vt_pixfmt2 format is DEFINED as a byte
re-arrangement of RGB8, NV12 or YUY2 (include/vittrack_hip.h), so a frame of one is built from a frame of its sibling and
back without arithmetic:
  nv12 <-> i420 / yv12 (chroma pairs split into two planes), nv12 <-> p010 (every byte the high byte of a 16-bit word),
  yuy2 <-> nv16 (luma and chroma pairs in planes of their own), rgb8 <-> gray8 (three equal bytes), rgb8 <-> xrgb / xbgr.
Buffers are packed: strides equal the row bytes, the planes follow each other."""
import numpy as np

SIBLING = {"i420": "nv12", "yv12": "nv12", "p010": "nv12", "nv16": "yuy2", "gray8": "rgb8", "xrgb": "rgb8", "xbgr": "rgb8"}
NEW = list(SIBLING)


def chroma_dims(w, h):
    """(columns, rows) of a 4:2:0 chroma plane"""
    return (w + 1) // 2, (h + 1) // 2


def nv12_planes(buf, w, h):
    """(Y [h][w], UV [ceil(h/2)][ceil(w/2)][2]) views of a packed NV12 buffer"""
    cw, ch = chroma_dims(w, h)
    buf = np.asarray(buf, np.uint8).reshape(-1)
    return buf[:w * h].reshape(h, w), buf[w * h:w * h + 2 * cw * ch].reshape(ch, cw, 2)


def nv12_to_i420(buf, w, h, yv12=False):
    y, uv = nv12_planes(buf, w, h)
    first, second = (uv[..., 1], uv[..., 0]) if yv12 else (uv[..., 0], uv[..., 1])
    return np.concatenate([y.reshape(-1), first.reshape(-1), second.reshape(-1)])


def i420_to_nv12(buf, w, h, yv12=False):
    cw, ch = chroma_dims(w, h)
    buf = np.asarray(buf, np.uint8).reshape(-1)
    first = buf[w * h:w * h + cw * ch].reshape(ch, cw)
    second = buf[w * h + cw * ch:w * h + 2 * cw * ch].reshape(ch, cw)
    u, v = (second, first) if yv12 else (first, second)
    return np.concatenate([buf[:w * h], np.stack([u, v], axis=2).reshape(-1)])


def nv12_to_p010(buf, w, h, rng=None):
    """bytes of the P010 frame: every NV12 byte becomes the high byte of a little-endian 16-bit word whose low byte - the
    two low value bits of a 10-bit sample and the six padding bits - comes from `rng` (None: zero)"""
    cw, ch = chroma_dims(w, h)
    n = w * h + 2 * cw * ch
    hi = np.asarray(buf, np.uint8).reshape(-1)[:n]
    lo = rng.integers(0, 256, n, dtype=np.uint8) if rng is not None else np.zeros(n, np.uint8)
    return np.stack([lo, hi], axis=1).reshape(-1)


def p010_to_nv12(buf, w, h):
    return np.ascontiguousarray(np.asarray(buf, np.uint8).reshape(-1, 2)[:, 1])


def yuy2_to_nv16(buf, w, h):
    p = np.asarray(buf, np.uint8).reshape(h, w // 2, 4)
    y = np.stack([p[..., 0], p[..., 2]], axis=2).reshape(-1)
    uv = np.stack([p[..., 1], p[..., 3]], axis=2).reshape(-1)
    return np.concatenate([y, uv])


def nv16_to_yuy2(buf, w, h):
    buf = np.asarray(buf, np.uint8).reshape(-1)
    y = buf[:w * h].reshape(h, w // 2, 2)
    uv = buf[w * h:2 * w * h].reshape(h, w // 2, 2)
    return np.stack([y[..., 0], uv[..., 0], y[..., 1], uv[..., 1]], axis=2).reshape(-1)


def rgb8_to_gray8(rgb):
    """(H,W) grey plane of a grey (H,W,3) image: r = g = b in every pixel"""
    rgb = np.asarray(rgb, np.uint8)
    assert np.array_equal(rgb[..., 0], rgb[..., 1]) and np.array_equal(rgb[..., 0], rgb[..., 2]), "not a grey image"
    return np.ascontiguousarray(rgb[..., 0])


def gray8_to_rgb8(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[:, :, None], 3, axis=2))


def rgb8_to_xrgb(rgb, xbyte=0, bgr=False):
    """(H,W,4) x,R,G,B (bgr: x,B,G,R); the x byte of every pixel is `xbyte` (a number or an (H,W) array)"""
    rgb = np.asarray(rgb, np.uint8)
    x = np.broadcast_to(np.asarray(xbyte, np.uint8), rgb.shape[:2])[:, :, None]
    return np.ascontiguousarray(np.concatenate([x, rgb[..., ::-1] if bgr else rgb], axis=2))


def xrgb_to_rgb8(a, bgr=False):
    a = np.asarray(a, np.uint8)
    return np.ascontiguousarray(a[..., 3:0:-1] if bgr else a[..., 1:4])


def from_sibling(fmt, sib, w, h, rng=None, xbyte=0):
    """the new format's packed bytes from its sibling's (SIBLING[fmt]): an NV12 / YUY2 buffer or an (H,W,3) RGB array"""
    if fmt in ("i420", "yv12"):
        return nv12_to_i420(sib, w, h, yv12=fmt == "yv12")
    if fmt == "p010":
        return nv12_to_p010(sib, w, h, rng)
    if fmt == "nv16":
        return yuy2_to_nv16(sib, w, h)
    if fmt == "gray8":
        return rgb8_to_gray8(sib)
    assert fmt in ("xrgb", "xbgr")
    return rgb8_to_xrgb(sib, xbyte, bgr=fmt == "xbgr")
