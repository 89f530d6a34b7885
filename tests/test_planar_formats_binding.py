"""vt_pixfmt2 (I420, YV12, P010, NV16, GRAY8, XRGB, XBGR) across the bindings, without a GPU: the header's enum values,
the Rust constants and the Python PIX_* constants agree; vt_pixfmt, the function count and the ABI version are what they
were; the Python frame classes hand the library the right format code, strides and plane pointers; the sibling builders
of planar_formats_util.py give hand-written known answers."""
import os
import re

import numpy as np
import pytest

import planar_formats_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES2 = {"I420": 16, "YV12": 17, "P010": 18, "NV16": 19, "GRAY8": 20, "XRGB": 21, "XBGR": 22}
NAMES = ["RGB8", "NV12", "YUY2", "BGR8", "RGBX", "BGRX", "NV21", "UYVY"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vittrack_hip.h")).read(), flags=re.S)


def _enum(name, prefix):
    body = re.search(r"typedef\s+enum\s+%s\s*\{(.*?)\}" % name, _header(), flags=re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(prefix + r"(\w+)\s*=\s*(\d+)", body)}


def test_header_rust_and_python_agree_on_vt_pixfmt2(vt):
    hdr = _enum("vt_pixfmt2", "VT_PIX2_")
    assert hdr == NAMES2
    rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    rust = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const VT_PIX2_(\w+): i32 = (\d+);", rs)}
    assert rust == hdr
    assert {n: getattr(vt, "PIX_" + n) for n in NAMES2} == hdr


def test_the_frozen_surface_is_what_it_was(vt):
    assert _enum("vt_pixfmt", "VT_PIX_") == {n: i for i, n in enumerate(NAMES)}
    txt = _header()
    assert len(set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", txt))) == 91 and len(vt.EXPORTS) == 91
    assert re.search(r"#define\s+VT_ABI_VERSION\s+5\b", txt)
    # the enum of the new values sits directly below vt_pixfmt
    assert re.search(r"\}\s*vt_pixfmt;\s*typedef\s+enum\s+vt_pixfmt2\b", txt)


def test_frame_classes_map_to_format_strides_and_planes(vt):
    # an odd-sized I420 / YV12 buffer: plane1 is the first chroma plane, stride1 = ceil(w / 2)
    w, h = 11, 7
    cw, ch = 6, 4
    buf = np.arange(w * h + 2 * cw * ch, dtype=np.uint8)
    for cls, code in ((vt.I420Frame, vt.PIX_I420), (vt.YV12Frame, vt.PIX_YV12)):
        f, keep = vt.Group._host_frame(cls(buf, w, h))
        assert (f.format, f.width, f.height, f.stride0, f.stride1) == (code, w, h, w, cw)
        assert f.plane0 == keep.buf.ctypes.data and f.plane1 - f.plane0 == w * h
        assert (f.origin_x, f.origin_y, f.windowed, f.window_w, f.window_h) == (0, 0, 0, 0, 0)
    with pytest.raises(AssertionError):
        vt.I420Frame(buf[:-1], w, h)
    # P010: strides in bytes, from bytes and from 16-bit samples
    w, h = 10, 6
    s16 = (np.arange(w * h * 3 // 2, dtype=np.uint16) * 64).astype(np.uint16)
    for b in (s16, s16.astype("<u2").view(np.uint8)):
        f, keep = vt.Group._host_frame(vt.P010Frame(b, w, h))
        assert (f.format, f.stride0, f.stride1) == (vt.PIX_P010, 2 * w, 2 * w)
        assert f.plane1 - f.plane0 == 2 * w * h
        assert np.array_equal(keep.buf.view("<u2"), s16)
    f, _ = vt.Group._host_frame(vt.P010Frame(np.zeros(2 * (11 * 7 + 12 * 4), np.uint8), 11, 7))
    assert (f.stride0, f.stride1) == (22, 24)
    f, _ = vt.Group._host_frame(vt.NV16Frame(np.zeros(2 * w * h, np.uint8), w, h))
    assert (f.format, f.stride0, f.stride1, f.plane1 - f.plane0) == (vt.PIX_NV16, w, w, w * h)
    # the packed ones: GRAY8 from (H,W) and (H,W,1), XRGB / XBGR from (H,W,4); padded views in place
    g = np.arange(h * w, dtype=np.uint8).reshape(h, w)
    for a in (g, g[:, :, None]):
        f, keep = vt.Group._host_frame(vt.Gray8Frame(a))
        assert (f.format, f.stride0, f.plane1, f.plane0) == (vt.PIX_GRAY8, w, None, keep.arr.ctypes.data)
    wide = np.zeros((h, w + 5), np.uint8)
    fr = vt.Gray8Frame(wide[:, :w])
    assert fr.stride == w + 5 and fr.cframe().plane0 == wide.ctypes.data
    assert vt.Gray8Frame(g, stride=16).stride == 16
    x = np.arange(h * w * 4, dtype=np.uint8).reshape(h, w, 4)
    for cls, code in ((vt.XRGBFrame, vt.PIX_XRGB), (vt.XBGRFrame, vt.PIX_XBGR)):
        f, keep = vt.Group._host_frame(cls(x))
        assert (f.format, f.stride0, f.plane1) == (code, 4 * w, None)
        with pytest.raises(vt.VtError):
            cls(x[..., :3])
    # device helpers
    f = vt.frame_i420(4096, 8192, 11, 7)
    assert (f.format, f.plane0, f.plane1, f.stride0, f.stride1) == (vt.PIX_I420, 4096, 8192, 11, 6)
    assert (vt.frame_yv12(4096, 8192, 11, 7, 16, 8).stride0, vt.frame_yv12(4096, 8192, 11, 7, 16, 8).stride1) == (16, 8)
    assert vt.frame_yv12(4096, 8192, 11, 7).format == vt.PIX_YV12
    f = vt.frame_p010(4096, 8192, 11, 7)
    assert (f.format, f.stride0, f.stride1) == (vt.PIX_P010, 22, 24)
    f = vt.frame_nv16(4096, 8192, w, h)
    assert (f.format, f.stride0, f.stride1) == (vt.PIX_NV16, w, w)
    assert (vt.frame_gray8(4096, w, h).format, vt.frame_gray8(4096, w, h).stride0, vt.frame_gray8(4096, w, h, 64).stride0) == \
        (vt.PIX_GRAY8, w, 64)
    assert (vt.frame_xrgb(4096, w, h).format, vt.frame_xrgb(4096, w, h).stride0) == (vt.PIX_XRGB, 4 * w)
    assert (vt.frame_xbgr(4096, w, h).format, vt.frame_xbgr(4096, w, h, 48).stride0) == (vt.PIX_XBGR, 48)


def test_sibling_builders_give_the_known_answers():
    # 4 x 2 NV12: Y 0..7, one chroma row U,V,U,V = 10,20,11,21
    nv12 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 10, 20, 11, 21], np.uint8)
    i420 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 20, 21], np.uint8)
    yv12 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 20, 21, 10, 11], np.uint8)
    assert np.array_equal(U.nv12_to_i420(nv12, 4, 2), i420) and np.array_equal(U.nv12_to_i420(nv12, 4, 2, yv12=True), yv12)
    assert np.array_equal(U.i420_to_nv12(i420, 4, 2), nv12) and np.array_equal(U.i420_to_nv12(yv12, 4, 2, yv12=True), nv12)
    p010 = U.nv12_to_p010(nv12, 4, 2)
    assert p010.tolist() == [0, 0, 0, 1, 0, 2, 0, 3, 0, 4, 0, 5, 0, 6, 0, 7, 0, 10, 0, 20, 0, 11, 0, 21]
    noisy = U.nv12_to_p010(nv12, 4, 2, np.random.default_rng(1))
    assert np.array_equal(noisy[1::2], nv12) and noisy[0::2].any() and np.array_equal(U.p010_to_nv12(noisy, 4, 2), nv12)
    # 5 x 3 (odd both ways): chroma planes 3 x 2, NV12 chroma rows of 6 bytes
    y = np.arange(15, dtype=np.uint8)
    nv12 = np.concatenate([y, np.array([30, 40, 31, 41, 32, 42, 33, 43, 34, 44, 35, 45], np.uint8)])
    i420 = np.concatenate([y, np.array([30, 31, 32, 33, 34, 35, 40, 41, 42, 43, 44, 45], np.uint8)])
    yv12 = np.concatenate([y, np.array([40, 41, 42, 43, 44, 45, 30, 31, 32, 33, 34, 35], np.uint8)])
    assert U.chroma_dims(5, 3) == (3, 2)
    assert np.array_equal(U.nv12_to_i420(nv12, 5, 3), i420) and np.array_equal(U.nv12_to_i420(nv12, 5, 3, yv12=True), yv12)
    assert np.array_equal(U.i420_to_nv12(i420, 5, 3), nv12) and np.array_equal(U.i420_to_nv12(yv12, 5, 3, yv12=True), nv12)
    assert U.nv12_to_p010(nv12, 5, 3).size == 2 * 27 and np.array_equal(U.p010_to_nv12(U.nv12_to_p010(nv12, 5, 3), 5, 3), nv12)
    # 4 x 2 YUY2: Y0 U Y1 V
    yuy2 = np.array([1, 50, 2, 60, 3, 51, 4, 61, 5, 52, 6, 62, 7, 53, 8, 63], np.uint8)
    nv16 = np.array([1, 2, 3, 4, 5, 6, 7, 8, 50, 60, 51, 61, 52, 62, 53, 63], np.uint8)
    assert np.array_equal(U.yuy2_to_nv16(yuy2, 4, 2), nv16) and np.array_equal(U.nv16_to_yuy2(nv16, 4, 2), yuy2)
    # grey and pad-first RGB, 5 x 3
    g = np.arange(15, dtype=np.uint8).reshape(3, 5)
    rgb = U.gray8_to_rgb8(g)
    assert rgb.shape == (3, 5, 3) and rgb[1, 2].tolist() == [7, 7, 7] and np.array_equal(U.rgb8_to_gray8(rgb), g)
    with pytest.raises(AssertionError):
        U.rgb8_to_gray8(np.arange(45, dtype=np.uint8).reshape(3, 5, 3))
    rgb = np.arange(45, dtype=np.uint8).reshape(3, 5, 3)
    xrgb, xbgr = U.rgb8_to_xrgb(rgb, 200), U.rgb8_to_xrgb(rgb, 9, bgr=True)
    assert xrgb[0, 1].tolist() == [200, 3, 4, 5] and xbgr[0, 1].tolist() == [9, 5, 4, 3] and xrgb.shape == (3, 5, 4)
    assert np.array_equal(U.xrgb_to_rgb8(xrgb), rgb) and np.array_equal(U.xrgb_to_rgb8(xbgr, bgr=True), rgb)
    assert np.array_equal(U.from_sibling("xbgr", rgb, 5, 3, xbyte=9), xbgr)
    assert np.array_equal(U.from_sibling("yv12", nv12, 5, 3), yv12)
