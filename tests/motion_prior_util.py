"""The motion prior ("Motion prior"; include/vittrack_hip.h above the "motion_*" keys) restated in numpy
float32 for the tests: the per-stream record, place and settle - every operation a binary32 operation of its own - and
drivers that apply the rule from OUTSIDE to anything whose box can be read and set: the oracle (oracle.VitTrackRef.box) and
the "set_state_box twin", a plain HIP engine whose host moves the boxes. The tests compare a motion-enabled engine with
both."""
import numpy as np

from oracle import vit_ref as o

F = np.float32
REC_WORDS = 12      # the 48-byte record: v[2] prior[4] shift[2] | live, n_shift, n_coast, reserved


class Policy:
    def __init__(self, on=1, gain_pct=50, coast=5, max_pct=100):
        self.on, self.gain_pct, self.coast, self.max_pct = int(on), int(gain_pct), int(coast), int(max_pct)

    def tuple(self):
        return self.on, self.gain_pct, self.coast, self.max_pct


class Record:
    def __init__(self, v=(0, 0), prior=(0, 0, 0, 0), shift=(0, 0), live=0, n_shift=0, n_coast=0):
        self.v = np.array(v, F)
        self.prior = np.array(prior, F)
        self.shift = np.array(shift, F)
        self.live, self.n_shift, self.n_coast = int(live), int(n_shift), int(n_coast)

    def copy(self):
        return Record(self.v, self.prior, self.shift, self.live, self.n_shift, self.n_coast)

    def words(self):
        """the record as the device lays it out: 12 32-bit words"""
        w = np.zeros(REC_WORDS, np.uint32)
        w[0:2], w[2:6], w[6:8] = self.v.view(np.uint32), self.prior.view(np.uint32), self.shift.view(np.uint32)
        w[8:11] = np.array([self.live, self.n_shift, self.n_coast], np.int32).view(np.uint32)
        return w

    def read_out(self, on):
        """what vt_group_read_tensor "motion" returns for this record"""
        return np.array([on, self.v[0], self.v[1], self.live, self.shift[0], self.shift[1], self.n_shift, self.n_coast], F)


def place(pol, rec, box, frame_w, frame_h):
    """the first launch of a pass on one initialised stream: rec is updated in place -> the box the pass is cut around"""
    b = np.array(box, F)
    rec.prior = b.copy()
    rec.shift = np.zeros(2, F)
    if not pol.on or (rec.v[0] == 0 and rec.v[1] == 0):
        return b
    px, py = F(b[0] + rec.v[0]), F(b[1] + rec.v[1])
    cx, cy = F(px + F(F(0.5) * b[2])), F(py + F(F(0.5) * b[3]))
    if F(0) <= cx < F(frame_w) and F(0) <= cy < F(frame_h):
        rec.shift = rec.v.copy()
        rec.n_shift += 1
        return np.array([px, py, b[2], b[3]], F)
    rec.v = np.zeros(2, F)
    rec.live = 0
    return b


def settle(pol, rec, box_after, success, has_box=False):
    """the launch behind the decode (the commit) on one stream of the pass: box_after is the state box the decode left,
    success the final result's flag (a NaN score arrives here as a failure), has_box: the winning candidate slot brought
    its own box. rec is updated in place -> the final state box"""
    b = np.array(box_after, F)
    if not pol.on:
        return b
    if success and not has_box:
        g = F(F(pol.gain_pct) / F(100))
        lim = F(F(F(pol.max_pct) / F(100)) * np.sqrt(F(b[2] * b[3])))
        for k in range(2):
            c_old = F(rec.prior[k] + F(F(0.5) * rec.prior[2 + k]))
            c_new = F(b[k] + F(F(0.5) * b[2 + k]))
            d = F(c_new - c_old)
            v = F(rec.v[k] + F(g * F(d - rec.v[k])))
            # fminf(fmaxf(v, -lim), lim) as two comparisons: the sign of a zero (lim == 0) is then defined - v < -lim gives
            # -lim, v > lim gives lim, anything else stays - and it is what the kernel does
            v = F(-lim) if v < F(-lim) else v
            rec.v[k] = lim if v > lim else v
        rec.live = pol.coast
    elif success:
        rec.v = np.zeros(2, F)
        rec.live = pol.coast
    elif rec.live > 0:
        rec.live -= 1
        if rec.shift[0] != 0 or rec.shift[1] != 0:
            rec.n_coast += 1
    else:
        b = rec.prior.copy()
        rec.v = np.zeros(2, F)
    return b


# ---- drivers ------------------------------------------------------------------------------------------------------------

class OracleTracker:
    """oracle.VitTrackRef on RGB8 arrays, its box readable and settable"""

    def __init__(self, weights):
        self.ref = o.VitTrackRef(weights)

    def init(self, rgb, bbox):
        self.ref.init(o.Frame.rgb8(rgb), bbox)

    def update(self, rgb):
        return self.ref.update(o.Frame.rgb8(rgb))

    def box(self):
        return self.ref.box.copy()

    def set_box(self, b):
        self.ref.box = np.array(b, F)


def drive(trk, frames, box0, pol, frame_w, frame_h):
    """init on frames[0], one update per later frame with the rule applied from outside: the box is moved ahead of the
    update and settled behind it. pol None: the plain tracker. -> (results, records after each update, boxes after each)"""
    rec = Record()
    trk.init(frames[0], box0)
    results, recs, boxes = [], [], []
    for fr in frames[1:]:
        if pol is not None:
            trk.set_box(place(pol, rec, trk.box(), frame_w, frame_h))
        r = trk.update(fr)
        if pol is not None:
            trk.set_box(settle(pol, rec, trk.box(), bool(r.success)))
        results.append(r)
        recs.append(rec.copy())
        boxes.append(trk.box())
    return results, recs, boxes


class Twin:
    """A plain engine (never motion-enabled) driven to the twin identity: the host keeps the records and calls
    set_state_box(prior + shift) ahead of every pass in which shift != 0 and set_state_box(prior) behind a failure that
    restores. before(streams) / after(...) bracket every pass of the group `g`."""

    def __init__(self, g, pol):
        self.g, self.pol = g, pol
        self.recs = [Record() for _ in range(g.streams)]

    def reset(self, s):
        self.recs[s] = Record()

    def before(self, streams):
        for s in dict.fromkeys(streams):        # once per stream, however many slots name it
            st = self.g.read_state(s)
            nb = place(self.pol, self.recs[s], st["box"], st["frame_w"], st["frame_h"])
            if self.recs[s].shift[0] != 0 or self.recs[s].shift[1] != 0:
                self.g.set_state_box(s, nb)

    def after(self, streams, results, winners=None, has_box=None):
        for i, s in enumerate(streams):
            if winners is not None and winners[i] != i:
                continue
            b = self.g.read_state(s)["box"]
            fb = settle(self.pol, self.recs[s], b, bool(results[i].success), bool(has_box[i]) if has_box is not None else False)
            if fb.tobytes() != np.array(b, F).tobytes():
                self.g.set_state_box(s, fb)


def iou(a, b):
    x1, y1 = max(a[0], b[0]), max(a[1], b[1])
    x2, y2 = min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
    inter = max(0, x2 - x1) * max(0, y2 - y1)
    return inter / float(a[2] * a[3] + b[2] * b[3] - inter)


def clip_frames(sc, n, step=1):
    """-> (clip times, RGB8 frames) of n frames, every step-th clip frame"""
    ts = list(range(0, n * step, step))
    return ts, [sc.frame_rgb8(t) for t in ts]
