"""The NumPy model of the frame format's colour bits (include/vittrack_hip.h: vt_color_matrix, vt_color_range).

code = matrix * 2 + range chooses a row of TABLE (YO, CY, CRV, CGU, CGV, CBU); yuv_to_rgb8 is the header's rule to the bit.
rgb8_sibling is the RGB8 frame a coloured YUV frame MEANS, pixel by pixel, with the chroma sample replicated as the kernels
read it (4:2:0 at (x >> 1, y >> 1), 4:2:2 at (x >> 1, y)): an engine fed it computes what the engine fed the YUV frame must.
The builders make every YUV format's bytes from one NV12 / YUY2 buffer through the existing sibling builders."""
import numpy as np

import planar_formats_util as U
from test_gpu_pixel_formats import _nv12_to_yuy2, _permute

TABLE = np.array([[16, 298, 409, -100, -208, 516],
                  [0, 256, 359, -88, -183, 454],
                  [16, 298, 459, -55, -136, 541],
                  [0, 256, 403, -48, -120, 475],
                  [16, 298, 430, -48, -167, 548],
                  [0, 256, 377, -42, -146, 482]], np.int32)
CODES = range(6)
NEW_CODES = range(1, 6)
KR_KB = [(0.299, 0.114), (0.2126, 0.0722), (0.2627, 0.0593)]      # BT.601, BT.709, BT.2020 (non-constant luminance)
YUV_FORMATS = ["nv12", "nv21", "yuy2", "uyvy", "i420", "yv12", "p010", "nv16"]
FAMILY = {"nv12": "420", "nv21": "420", "i420": "420", "yv12": "420", "p010": "420", "yuy2": "422", "uyvy": "422", "nv16": "422"}


def matrix_range(code):
    return code >> 1, code & 1


def exact_coefficients(code):
    """(YO, CY, CRV, CGU, CGV, CBU) in float64, before the scale by 256 and the rounding"""
    m, full = matrix_range(code)
    kr, kb = KR_KB[m]
    kg = 1.0 - kr - kb
    sy, sc = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    return (0.0 if full else 16.0, sy, 2.0 * (1.0 - kr) * sc, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc,
            2.0 * (1.0 - kb) * sc)


def unclamped(y, u, v, code):
    """the three int32 sums of the rule, before the clamp"""
    yo, cy, crv, cgu, cgv, cbu = (int(c) for c in TABLE[code])
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    yv = cy * (y - yo)
    return yv + crv * (v - 128) + 128, yv + cgu * (u - 128) + cgv * (v - 128) + 128, yv + cbu * (u - 128) + 128


def yuv_to_rgb8(y, u, v, code):
    """(..., 3) uint8: min(max(x, 0), 0xffff) >> 8 of the three sums"""
    return np.stack([np.clip(c, 0, 0xffff) >> 8 for c in unclamped(y, u, v, code)], axis=-1).astype(np.uint8)


def float_rgb8(y, u, v, code):
    """clip(rint(exact float64 conversion), 0, 255)"""
    yo, cy, crv, cgu, cgv, cbu = exact_coefficients(code)
    y, u, v = (np.asarray(a).astype(np.float64) for a in (y, u, v))
    yv, u, v = cy * (y - yo), u - 128.0, v - 128.0
    return np.clip(np.rint(np.stack([yv + crv * v, yv + cgu * u + cgv * v, yv + cbu * u], axis=-1)), 0, 255).astype(np.int32)


def yuv_planes(family, data, w, h):
    """(Y, U, V), each [h][w], of an NV12 buffer ("420") or a YUY2 buffer ("422"): chroma replicated as the kernels read it"""
    d = np.asarray(data, np.uint8).reshape(-1)
    xs = np.arange(w) >> 1
    if family == "420":
        y, uv = U.nv12_planes(d, w, h)
        rows = (np.arange(h) >> 1)[:, None]
        return y, uv[rows, xs[None, :], 0], uv[rows, xs[None, :], 1]
    p = d[:2 * w * h].reshape(h, w // 2, 4)
    y = np.stack([p[..., 0], p[..., 2]], axis=2).reshape(h, w)
    return y, p[:, xs, 1], p[:, xs, 3]


def rgb8_sibling(family, data, w, h, code):
    """the (h, w, 3) RGB8 frame that the NV12 ("420") / YUY2 ("422") bytes mean under `code`"""
    return np.ascontiguousarray(yuv_to_rgb8(*yuv_planes(family, data, w, h), code))


def random_nv12(w, h, seed):
    """a packed NV12 frame whose every Y, U and V byte is uniform in 0..255"""
    cw, ch = U.chroma_dims(w, h)
    return np.random.default_rng(seed).integers(0, 256, w * h + 2 * cw * ch, dtype=np.uint8)


def base_bytes(family, nv12, w, h):
    """the NV12 buffer itself, or the YUY2 buffer with its luma and, per row, its chroma row (w even)"""
    return nv12 if family == "420" else _nv12_to_yuy2(nv12, w, h)


def format_bytes(fmt, nv12, w, h, rng=None):
    """packed bytes of a YUV format from ONE NV12 buffer: the 4:2:0 formats hold its samples, the 4:2:2 ones its luma and
    on every row the chroma row of that row's pair"""
    if fmt == "nv12":
        return nv12
    if fmt == "nv21":
        return _permute("nv21", nv12, w, h)
    if fmt in ("i420", "yv12", "p010"):
        return U.from_sibling(fmt, nv12, w, h, rng=rng)
    yuy2 = _nv12_to_yuy2(nv12, w, h)
    if fmt == "yuy2":
        return yuy2
    if fmt == "uyvy":
        return _permute("uyvy", yuy2, w, h)
    assert fmt == "nv16"
    return U.yuy2_to_nv16(yuy2, w, h)


def sibling_of(fmt, nv12, w, h, code):
    """the RGB8 sibling of format_bytes(fmt, nv12, ...) under `code`"""
    return rgb8_sibling(FAMILY[fmt], base_bytes(FAMILY[fmt], nv12, w, h), w, h, code)


def host_frame(gpu, fmt, data, w, h, code=0):
    m, full = matrix_range(code)
    cls = {"nv12": gpu.NV12Frame, "nv21": gpu.NV21Frame, "yuy2": gpu.YUY2Frame, "uyvy": gpu.UYVYFrame, "i420": gpu.I420Frame,
           "yv12": gpu.YV12Frame, "p010": gpu.P010Frame, "nv16": gpu.NV16Frame}[fmt]
    return cls(data, w, h, matrix=m, full_range=bool(full))


def pix(gpu, fmt):
    return getattr(gpu, "PIX_" + fmt.upper())


def word(gpu, fmt, code):
    m, full = matrix_range(code)
    return gpu.frame_format(pix(gpu, fmt), m, bool(full))
