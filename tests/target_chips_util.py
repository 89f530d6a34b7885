"""Target chips ("Target chips") restated in numpy float32, for the tests: the crop's bilinear value v
with the geometry, tap order and float operation order of vto_preproc (tests/test_target_chips_abi.py ties bf16(v) to the
oracle bit for bit), the two chip kinds on top of v, the gate, and a driver that runs the oracle tracker under the gate."""
import numpy as np

from oracle import vit_ref as o
from template_refresh_util import inside, tap_rect_geo

F = np.float32
NOT_DUE, CUT, SKIPPED = 0, 1, 2
NORM_BF16, RGB8 = 0, 1


def chip_geometry(box, factor, C):
    """(x0m, y0m, scale, side) of the chip crop: vto_crop_geometry"""
    return o.crop_geometry(np.asarray(box, F), float(factor), int(C))


def bilinear(rgb, box, factor, C):
    """v [3][C][C] float32: the bilinear value of the chip crop of an (H, W, 3) RGB8 frame at `box`; taps outside the
    frame are black. One binary32 operation per source operation, in the order of k_preproc_body.inc."""
    rgb = np.asarray(rgb, np.uint8)
    h, w, _ = rgb.shape
    x0m, y0m, scale, _ = (F(v) for v in chip_geometry(box, factor, C))
    idx = np.arange(C, dtype=F)
    fx = (idx + F(0.5)) * scale + x0m
    fy = (idx + F(0.5)) * scale + y0m
    assert fx.dtype == F and fy.dtype == F
    fx0, fy0 = np.floor(fx), np.floor(fy)
    wx, wy = (fx - fx0)[None, :, None], (fy - fy0)[:, None, None]
    ix, iy = fx0.astype(np.int64), fy0.astype(np.int64)
    pad = np.zeros((h + 2, w + 2, 3), F)            # a black border: index -1 and w / h
    pad[1:-1, 1:-1] = rgb

    def tap(yy, xx):
        yc = np.where((yy < 0) | (yy >= h), -1, yy) + 1
        xc = np.where((xx < 0) | (xx >= w), -1, xx) + 1
        return pad[yc[:, None], xc[None, :]]        # [C][C][3]

    p00, p01, p10, p11 = tap(iy, ix), tap(iy, ix + 1), tap(iy + 1, ix), tap(iy + 1, ix + 1)
    top = p00 + wx * (p01 - p00)
    bot = p10 + wx * (p11 - p10)
    v = top + wy * (bot - top)
    assert v.dtype == F
    return np.ascontiguousarray(v.transpose(2, 0, 1))


def chip_bf16(v, norm_a, norm_b):
    """VT_CHIP_NORM_BF16: planar [3][C][C] bf16 bit patterns of v * a_c + b_c"""
    a, b = np.asarray(norm_a, F)[:, None, None], np.asarray(norm_b, F)[:, None, None]
    return o.f32_to_bf16_bits((v * a + b).astype(F)).reshape(v.shape)


def chip_u8(v):
    """VT_CHIP_RGB8: packed [C][C][3] of (uint8)min(max(rintf(v), 0), 255); rint is round-half-to-even, as rintf"""
    return np.ascontiguousarray(np.clip(np.rint(v), 0, 255).astype(np.uint8).transpose(1, 2, 0))


def oracle_chip_bf16(frame, box, factor, C, norm_a, norm_b):
    """the same from the oracle: vto_preproc with patch = C, kpad = 3 C^2 writes one row that IS the planar chip"""
    return o.preproc(frame, np.asarray(box, F), float(factor), C, C, 3 * C * C, norm_a, norm_b).reshape(3, C, C)


class ChipRule:
    """The gate for one stream. step() is called once per update of the stream with the state the update left: the box
    (the new one, or the last good one after a failed update), the geometry of the search crop the update sampled, and
    whether its window missed; -> NOT_DUE / CUT / SKIPPED, as vt_chip_info.status."""

    def __init__(self, C, S, factor, period=1, phase=0):
        self.C, self.S, self.factor, self.period, self.phase = int(C), int(S), float(factor), int(period), int(phase)
        self.done = 0
        self.cut, self.skipped = [], []

    def step(self, box, search_geo, window_miss=False, winner=True):
        self.done += 1
        if not self.factor > 0 or not winner:
            return None
        if self.done % self.period != self.phase or window_miss:
            return NOT_DUE
        t = tap_rect_geo(chip_geometry(box, self.factor, self.C), self.C)
        if not inside(t, tap_rect_geo(search_geo, self.S)):
            self.skipped.append(self.done)
            return SKIPPED
        self.cut.append(self.done)
        return CUT


def drive_oracle(weights, frames, box0, rules):
    """the oracle tracker (oracle.VitTrackRef on RGB8 arrays) over frames (frames[0] initialises AND is the first update's
    frame) under every rule of `rules` (a dict name -> ChipRule)
    -> per update (result, box after the update, {name: status})"""
    ref = o.VitTrackRef(weights)
    ref.init(o.Frame.rgb8(frames[0]), box0)
    out = []
    for fr in frames:
        geo = o.crop_geometry(ref.box, 4.0, ref.m.S)
        r = ref.update(o.Frame.rgb8(fr))
        out.append((r, tuple(float(v) for v in ref.box), {k: rule.step(ref.box, geo) for k, rule in rules.items()}))
    return out
