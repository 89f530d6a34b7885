"""vt_pixfmt 3-7 (BGR8, RGBX, BGRX, NV21, UYVY) across the bindings, without a GPU: the header's enum values, the Rust
constants and the Python PIX_* constants agree; the Python frame classes hand the library the right format code,
stride and planes; a bare (H,W,3) array is still RGB8."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["RGB8", "NV12", "YUY2", "BGR8", "RGBX", "BGRX", "NV21", "UYVY"]


def _header_enum():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vittrack_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+enum\s+vt_pixfmt\s*\{(.*?)\}", txt, flags=re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"VT_PIX_(\w+)\s*=\s*(\d+)", body)}


def test_header_rust_and_python_agree(vt):
    hdr = _header_enum()
    assert hdr == {n: i for i, n in enumerate(NAMES)}
    rs = open(os.path.join(ROOT, "bindings", "vit_tracker", "src", "sys.rs")).read()
    rust = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const VT_PIX_(\w+): i32 = (\d+);", rs)}
    assert rust == hdr
    assert {n: getattr(vt, "PIX_" + n) for n in NAMES} == hdr
    for fn in ("vt_init_frame", "vt_update_frame"):
        assert fn in vt.EXPORTS and re.search(r"pub fn %s\(" % fn, rs)


def test_frame_classes_map_to_format_stride_and_planes(vt):
    h, w = 6, 10
    rgb = np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3)
    rgbx = np.arange(h * w * 4, dtype=np.uint8).reshape(h, w, 4)
    for cls, a, code, c in ((vt.BGR8Frame, rgb, vt.PIX_BGR8, 3), (vt.RGBXFrame, rgbx, vt.PIX_RGBX, 4),
                            (vt.BGRXFrame, rgbx, vt.PIX_BGRX, 4)):
        f, keep = vt.Group._host_frame(cls(a))
        assert (f.format, f.width, f.height, f.stride0, f.plane1) == (code, w, h, c * w, None)
        assert f.plane0 == keep.arr.ctypes.data
        # a padded buffer's view is used in place with its pitch; an explicit stride pads a copy
        wide = np.zeros((h, c * w + 7), np.uint8)
        view = wide[:, :c * w].reshape(h, w, c)
        fr = cls(view)
        assert fr.stride == c * w + 7 and fr.cframe().plane0 == wide.ctypes.data
        fr = cls(a, stride=c * w + 16)
        assert fr.stride == c * w + 16 and np.array_equal(fr.arr, a)
        with pytest.raises(vt.VtError):
            cls(a, stride=c * w - 1)
        with pytest.raises(vt.VtError):
            cls(rgbx if c == 3 else rgb)
    buf = np.arange(w * h * 3 // 2, dtype=np.uint8)
    f, _ = vt.Group._host_frame(vt.NV21Frame(buf, w, h))
    assert (f.format, f.stride0, f.stride1) == (vt.PIX_NV21, w, w)
    assert f.plane1 - f.plane0 == w * h
    f, _ = vt.Group._host_frame(vt.UYVYFrame(np.zeros(2 * w * h, np.uint8), w, h))
    assert (f.format, f.stride0, f.plane1) == (vt.PIX_UYVY, 2 * w, None)
    # device helpers
    assert (vt.frame_bgr8(4096, w, h).format, vt.frame_bgr8(4096, w, h).stride0) == (vt.PIX_BGR8, 3 * w)
    assert (vt.frame_rgbx(4096, w, h).stride0, vt.frame_bgrx(4096, w, h, 64).stride0) == (4 * w, 64)
    nv21 = vt.frame_nv21(4096, 4096 + w * h, w, h)
    assert (nv21.format, nv21.stride0, nv21.stride1) == (vt.PIX_NV21, w, w)
    assert (vt.frame_uyvy(4096, w, h).format, vt.frame_uyvy(4096, w, h).stride0) == (vt.PIX_UYVY, 2 * w)


def test_a_bare_array_is_still_rgb8(vt):
    a = np.zeros((6, 10, 3), np.uint8)
    f, _ = vt.Group._host_frame(a)
    assert (f.format, f.stride0) == (vt.PIX_RGB8, 30)
