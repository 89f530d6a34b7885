"""The template-refresh rule ("Template refresh") restated in numpy float32, for the tests: the tap
rectangles from oracle.crop_geometry, the gate, and a driver that applies it to any object with init / update. The oracle
(tests/test_template_refresh_abi.py) and the HIP "host twin" - an engine with refresh off that the test re-initialises
whenever the rule fires (tests/test_gpu_template_refresh.py) - both go through it."""
import numpy as np

from oracle import vit_ref as o

F = np.float32


def tap_range(scale, x0m, size):
    """per axis: lo = floor(0.5 * scale + x0m), hi = floor((size - 0.5) * scale + x0m) + 1, every operation in binary32"""
    scale, x0m = F(scale), F(x0m)
    lo = int(np.floor(F(F(F(0) + F(0.5)) * scale) + x0m))
    hi = int(np.floor(F(F(F(size - 1) + F(0.5)) * scale) + x0m)) + 1
    return lo, hi


def tap_rect_geo(geo, size):
    """(x_lo, x_hi, y_lo, y_hi) of a crop with geometry geo = (x0m, y0m, scale, ...)"""
    return tap_range(geo[2], geo[0], size) + tap_range(geo[2], geo[1], size)


def tap_rect(box, factor, size):
    return tap_rect_geo(o.crop_geometry(np.asarray(box, F), factor, size), size)


def inside(t, s):
    return t[0] >= s[0] and t[1] <= s[1] and t[2] >= s[2] and t[3] <= s[3]


class Rule:
    """The gate for one stream. step() is called once per update of the stream, with the geometry of the search crop that
    update sampled (or the box it was cut around) and its result; it returns "fire", "skip" (due, but rule 6 failed) or
    None and keeps the stream's generation / last_frame as the device does."""

    def __init__(self, T, S, period, min_score=0.0):
        self.T, self.S, self.period, self.min_score = T, S, int(period), F(min_score)
        self.done = self.last_frame = self.generation = 0
        self.fired, self.skipped = [], []

    def step(self, result, pre_box=None, geo=None, window_miss=False, winner=True):
        self.done += 1
        bbox = result.bbox
        if self.period < 2 or not winner:
            return None
        if not result.success or not (F(result.score) >= self.min_score):      # a NaN score fails
            return None
        if self.done - self.last_frame < self.period or window_miss:
            return None
        s = tap_rect_geo(geo, self.S) if geo is not None else tap_rect(pre_box, 4.0, self.S)
        t = tap_rect(np.asarray(bbox, F), 2.0, self.T)
        if not inside(t, s):
            self.skipped.append(self.done)
            return "skip"
        self.last_frame = self.done
        self.generation += 1
        self.fired.append(self.done)
        return "fire"


def drive(trk, frames, box0, rule):
    """trk: anything with init(frame, bbox), update(frame) -> result(.success, .score, .bbox) and box() -> the box the
    next search crop is cut around. frames[0] initialises AND is the first update's frame. A refresh is
    trk.init(frame_t, result.bbox) after trk.update(frame_t). -> the results"""
    out = []
    for i, fr in enumerate(frames):
        if i == 0:
            trk.init(fr, box0)
        pre = np.array(trk.box(), F)
        r = trk.update(fr)
        if rule.step(r, pre_box=pre) == "fire":
            trk.init(fr, tuple(int(v) for v in r.bbox))
        out.append(r)
    return out


class OracleTracker:
    """oracle.VitTrackRef on RGB8 arrays"""

    def __init__(self, weights):
        self.ref = o.VitTrackRef(weights)

    def init(self, rgb, bbox):
        self.ref.init(o.Frame.rgb8(rgb), bbox)

    def update(self, rgb):
        return self.ref.update(o.Frame.rgb8(rgb))

    def box(self):
        return self.ref.box


def clip_frames(sc, n, step=1):
    """-> (clip times, RGB8 frames) of n updates, every step-th clip frame"""
    ts = list(range(0, n * step, step))
    return ts, [sc.frame_rgb8(t) for t in ts]
