"""The colour bits of vt_frame.format on the CPU: the coefficient table, its error bound, and the host helpers.

The table of include/vittrack_hip.h (code = matrix * 2 + range) is derived here in float64 from Kr / Kb and the range
scales, row 0 is the reference's formula written out, and every row stays within 1 of the clipped, rounded float64
conversion over all 2^24 (Y, U, V) triples. No GPU."""
import ctypes

import numpy as np
import pytest

import colorimetry_util as C


@pytest.fixture(scope="module")
def random_planes():
    rng = np.random.default_rng(7)
    w, h = 64, 48
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8), w, h


def _reference_formula(y, u, v):
    """the reference's BT.601 limited-range integer formula, constants written out"""
    y, u, v = (a.astype(np.int32) for a in (y, u, v))
    yv = 298 * (y - 16)
    r = (yv + 409 * (v - 128) + 128) >> 8
    g = (yv - 100 * (u - 128) - 208 * (v - 128) + 128) >> 8
    b = (yv + 516 * (u - 128) + 128) >> 8
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def test_the_table_is_the_rounded_exact_matrix():
    for code in C.CODES:
        exact = C.exact_coefficients(code)
        assert int(exact[0]) == C.TABLE[code][0]
        want = [int(np.rint(256.0 * c)) for c in exact[1:]]
        assert want == [int(c) for c in C.TABLE[code][1:]], (code, want)


def test_row_0_is_the_references_formula(vt, random_planes):
    assert [int(c) for c in C.TABLE[0]] == [16, 298, 409, -100, -208, 516]
    rng = np.random.default_rng(1)
    y, u, v = (rng.integers(0, 256, 100000, dtype=np.uint8) for _ in range(3))
    assert np.array_equal(C.yuv_to_rgb8(y, u, v, 0), _reference_formula(y, u, v))
    yy, uv, w, h = random_planes
    nv12 = np.concatenate([yy.reshape(-1), uv.reshape(-1)])
    assert np.array_equal(vt.synth.nv12_planes_to_rgb8(yy, uv, w, h), C.rgb8_sibling("420", nv12, w, h, 0))


def test_synth_defaults_are_unchanged_and_every_code_is_the_model(vt, random_planes):
    yy, uv, w, h = random_planes
    nv12 = np.concatenate([yy.reshape(-1), uv.reshape(-1)])
    cols, rows = (np.arange(w) // 2) * 2, np.arange(h) // 2
    want = _reference_formula(yy, uv[rows][:, cols], uv[rows][:, cols + 1])         # today's function, written out
    got = vt.synth.nv12_planes_to_rgb8(yy, uv, w, h)
    assert got.tobytes() == want.tobytes() and got.flags["C_CONTIGUOUS"] and got.dtype == np.uint8 and got.shape == (h, w, 3)
    assert vt.synth.MovingSquare(64, 48, 16, seed=0).frame_rgb8(1).flags["C_CONTIGUOUS"]        # it goes to the GPU as it lies
    assert vt.synth.nv12_planes_to_rgb8(yy, uv, w, h, 0, False).tobytes() == want.tobytes()
    for code in C.CODES:
        m, full = C.matrix_range(code)
        got = vt.synth.nv12_planes_to_rgb8(yy, uv, w, h, matrix=m, full_range=bool(full))
        assert np.array_equal(got, C.rgb8_sibling("420", nv12, w, h, code)), code


@pytest.mark.parametrize("code", list(C.CODES))
def test_every_row_is_within_1_of_the_float64_conversion_over_all_triples(code):
    """all 2^24 (Y, U, V) triples, one Y at a time over the 256 x 256 (U, V) grid; the clamp to 0xffff matters (the sums
    reach 140946) and is part of what is compared"""
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    yo, cy, crv, cgu, cgv, cbu = (int(c) for c in C.TABLE[code])
    eyo, ecy, ecrv, ecgu, ecgv, ecbu = C.exact_coefficients(code)
    ci = [crv * (v - 128) + 128, cgu * (u - 128) + cgv * (v - 128) + 128, cbu * (u - 128) + 128]
    cf = [ecrv * (v - 128.0), ecgu * (u - 128.0) + ecgv * (v - 128.0), ecbu * (u - 128.0)]
    worst, peak = 0, 0
    for y in range(256):
        yi, yf = cy * (y - yo), ecy * (y - eyo)
        for k in range(3):
            s = ci[k] + yi
            peak = max(peak, int(s.max()))
            got = np.clip(s, 0, 0xffff) >> 8
            want = np.clip(np.rint(cf[k] + yf), 0, 255).astype(np.int64)
            worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, (code, worst)
    assert peak > 0xffff, "no sum of this row needs the clamp ahead of the shift"
    # the chunked loop is the model: spot-check it against yuv_to_rgb8 / float_rgb8 on random triples
    rng = np.random.default_rng(code)
    t = [rng.integers(0, 256, 50000) for _ in range(3)]
    assert np.abs(C.yuv_to_rgb8(*t, code).astype(np.int32) - C.float_rgb8(*t, code)).max() <= 1


def test_the_sums_reach_140946():
    assert max(int(np.max(c)) for code in C.CODES for c in C.unclamped(
        *np.meshgrid(np.array([0, 255]), np.array([0, 255]), np.array([0, 255]), indexing="ij"), code)) == 140946


def test_the_grey_axis():
    y = np.arange(256)
    g = np.full(256, 128)
    for code in C.CODES:
        rgb = C.yuv_to_rgb8(y, g, g, code).astype(np.int32)
        assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 0], rgb[:, 2]), code
        if code & 1:
            assert np.array_equal(rgb[:, 0], y), code
        else:
            assert rgb[16, 0] == 0 and rgb[235, 0] == 255 and rgb[:16].max() == 0 and rgb[235:].min() == 255, code


def test_every_pair_of_codes_differs_somewhere():
    rng = np.random.default_rng(3)
    y, u, v = (rng.integers(0, 256, 4096) for _ in range(3))
    out = [C.yuv_to_rgb8(y, u, v, code) for code in C.CODES]
    for a in C.CODES:
        for b in range(a + 1, 6):
            assert not np.array_equal(out[a], out[b]), (a, b)


def test_the_synthetic_clips_square_differs_under_every_code(vt):
    sc = vt.synth.MovingSquare(640, 480, 64, seed=1)
    assert (sc.sq_u, sc.sq_v) == (90, 200)
    rgb = [tuple(int(c) for c in C.yuv_to_rgb8(200, sc.sq_u, sc.sq_v, code)) for code in C.CODES]
    assert len(set(rgb)) == 6, rgb


# ---- host helpers ---------------------------------------------------------------------------------------------------------

def test_frame_format_round_trips(vt):
    assert (vt.COLOR_BT601, vt.COLOR_BT709, vt.COLOR_BT2020, vt.RANGE_LIMITED, vt.RANGE_FULL) == (0, 1, 2, 0, 1)
    pixes = [getattr(vt, n) for n in dir(vt) if n.startswith("PIX_")]
    assert len(pixes) == 15
    for p in pixes:
        assert vt.frame_format(p) == p and vt.frame_format(p, vt.COLOR_BT601, False) == p
        for m in (0, 1, 2):
            for full in (False, True):
                word = vt.frame_format(p, m, full)
                assert (word & 0xff, (word >> 8) & 15, (word >> 12) & 15, word >> 16) == (p, m, int(full), 0)


def test_every_yuv_frame_class_and_builder_carries_the_word(vt):
    w, h = 32, 16
    buf = np.zeros(4 * w * h, np.uint8)
    for fmt in C.YUV_FORMATS:
        for code in C.CODES:
            m, full = C.matrix_range(code)
            want = C.word(vt, fmt, code)
            assert C.host_frame(vt, fmt, buf, w, h, code).cframe().format == want, (fmt, code)
            builder = getattr(vt, "frame_" + fmt)
            args = (1 << 20, w, h) if fmt in ("yuy2", "uyvy") else (1 << 20, 1 << 21, w, h)
            assert builder(*args, matrix=m, full_range=bool(full)).format == want, (fmt, code)
            assert builder(*args).format == C.pix(vt, fmt)
        cls_default = C.host_frame(vt, fmt, buf, w, h).cframe()
        assert cls_default.format == C.pix(vt, fmt)


def test_the_rgb_and_grey_classes_refuse_the_keywords(vt):
    a3, a4, a1 = np.zeros((16, 16, 3), np.uint8), np.zeros((16, 16, 4), np.uint8), np.zeros((16, 16), np.uint8)
    for cls, a in ((vt.BGR8Frame, a3), (vt.RGBXFrame, a4), (vt.BGRXFrame, a4), (vt.XRGBFrame, a4), (vt.XBGRFrame, a4),
                   (vt.Gray8Frame, a1)):
        for kw in ({"matrix": 1}, {"full_range": True}):
            with pytest.raises(TypeError):
                cls(a, **kw)
    for name in ("frame_rgb8", "frame_bgr8", "frame_rgbx", "frame_bgrx", "frame_gray8", "frame_xrgb", "frame_xbgr"):
        with pytest.raises(TypeError):
            getattr(vt, name)(1 << 20, 16, 16, matrix=1)


def test_colorimetry_from_gst(vt):
    f = vt.colorimetry_from_gst
    assert f("bt601") == (vt.COLOR_BT601, False) and f("bt709") == (vt.COLOR_BT709, False)
    assert f("bt2020") == (vt.COLOR_BT2020, False) and f("bt2020-10") == (vt.COLOR_BT2020, False)
    for rng, full in ((1, True), (2, False)):
        for mat, m in ((3, vt.COLOR_BT709), (4, vt.COLOR_BT601), (6, vt.COLOR_BT2020)):
            for tail in ("1:1", "5:1", "14:7", "0:0"):
                assert f(f"{rng}:{mat}:{tail}") == (m, full)
    assert f("1:4:0:0") == (vt.COLOR_BT601, True) and f("2:3:5:1") == (vt.COLOR_BT709, False)
    for bad in ("0:3:5:1", "3:3:5:1", "2:0:5:1", "2:1:5:1", "2:2:5:1", "2:5:5:1", "2:7:5:1", "sRGB", "srgb", "smpte240m", "", "bt470",
                "2:3:5", "2:3", "a:b:c:d", "2:3:5:1:0", "-1:3:5:1", "bt709-full"):
        with pytest.raises(ValueError):
            f(bad)
