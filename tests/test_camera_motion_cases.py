"""The rule of the camera motion on its NumPy model alone (tests/camera_motion_util.py; the rule to the bit:
include/vittrack_hip_ops.h, vt_op_camera_motion): what the GPU tests hold the kernels to must itself do what the rule
says, and the mutations a slip in a kernel would be must fail these cases. No GPU."""
import numpy as np
import pytest

import camera_motion_util as cm

F = np.float32
W, H, C, R = 160, 96, 4, 4
CANVAS = cm.texture(H + 64, W + 64, seed=11)


def pair(dx_cells, dy_cells, c=C, canvas=CANVAS, w=W, h=H):
    """two views whose content moves by (dx, dy) cells from the first to the second"""
    x0, y0 = 32, 32
    return cm.view(canvas, x0, y0, w, h), cm.view(canvas, x0 - dx_cells * c, y0 - dy_cells * c, w, h)


def run(a, b, box=(60, 40, 20, 20), **kw):
    s = cm.Stream()
    kw.setdefault("cell", C)
    kw.setdefault("R", R)
    first = s.step(a, box, **{k: v for k, v in kw.items() if k not in ("sign", "tie", "s2_dist")})
    return first, s.step(b, box, **kw), s


@pytest.mark.parametrize("d", [(1, 0), (0, -2), (3, 2), (-3, 1), (-1, -3)])
def test_whole_cell_shift_is_found_exactly(d):
    first, r, s = run(*pair(*d))
    assert first["status"] == 5 and not first["shift"].any() and first["applied"] == 0
    assert (r["status"], r["dx"], r["dy"], r["S_best"]) == (1, d[0], d[1], 0)
    assert not r["off"].any() and r["shift"].tobytes() == np.array([d[0] * C, d[1] * C], F).tobytes()
    assert r["applied"] == 1 and r["box"].tobytes() == np.array([60 + d[0] * C, 40 + d[1] * C, 20, 20], F).tobytes()
    assert r["n"] == (W // C - 2 * R) * (H // C - 2 * R) and r["S0"] > 0 and r["S2"] > 0
    assert (s.evaluated, s.moved) == (1, 1)


def test_still_pair():
    _, r, s = run(*pair(0, 0))
    assert (r["status"], r["dx"], r["dy"], r["S_best"], r["S0"]) == (1, 0, 0, 0, 0)
    assert not r["shift"].any() and r["applied"] == 0 and s.moved == 0      # nothing to move by


def test_mode_1_measures_and_leaves_the_box():
    _, r, _ = run(*pair(2, 1), mode=1)
    assert r["status"] == 1 and r["shift"].tolist() == [8.0, 4.0] and r["applied"] == 0 and r["box"].tolist() == [60, 40, 20, 20]


def periodic(k_cells, c=C):
    """a picture periodic in k cells along x, textured along y"""
    col = cm.texture(H + 64, k_cells * c, seed=5, smooth=1)
    return np.tile(col, (1, (W + 64) // (k_cells * c) + 2, 1))[:, :W + 64]


def test_periodic_picture_takes_the_smaller_displacement():
    canvas = periodic(3)
    a, b = pair(2, 0, canvas=canvas)        # +2 and -1 cells are the same picture
    _, r, _ = run(a, b)
    S = r["sad"]
    assert S[R, R + 2] == 0 and S[R, R - 1] == 0 and S[R, R - 4] == 0
    assert (r["dx"], r["dy"], r["S_best"]) == (-1, 0, 0)
    # S2 lies outside the 3 x 3 neighbourhood: another period of the picture, so nothing tells them apart
    assert r["S2"] == 0 and r["status"] == 3 and not r["shift"].any()


def test_tie_rule_mutation_fails_the_periodic_case():
    canvas = periodic(3)
    a, b = pair(2, 0, canvas=canvas)
    _, r, _ = run(a, b, tie="index")
    assert (r["dx"], r["dy"]) == (-4, 0)        # the lowest index of the zeros, not the shortest


def test_tie_prefers_the_lower_index_among_equal_lengths():
    S = np.full((2 * R + 1, 2 * R + 1), 1000, np.int64)
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        S[dy + R, dx + R] = 5
    d = cm.decide(S, R, C, 800)
    assert (d["dx"], d["dy"]) == (0, -1) and d["S2"] == 5 and d["status"] == 7


def test_flat_frames():
    a = np.full((H, W, 3), 93, np.uint8)
    _, r, _ = run(a, a.copy())
    assert (r["status"], r["dx"], r["dy"], r["S_best"], r["S2"]) == (3, 0, 0, 0, 0) and not r["shift"].any() and r["applied"] == 0


@pytest.mark.parametrize("d", [(R, 0), (-R, 1), (2, R), (0, -R)])
def test_a_shift_of_the_whole_range_is_status_6(d):
    _, r, _ = run(*pair(*d))
    assert (r["status"], r["dx"], r["dy"], r["S_best"]) == (6, d[0], d[1], 0) and not r["shift"].any() and r["applied"] == 0


NOISE_SEEDS = [(1, 2), (3, 4), (21, 22)]


@pytest.mark.parametrize("seeds", NOISE_SEEDS)
def test_independent_noise_is_ambiguous(seeds):
    a, b = (cm.texture(H, W, seed=s, smooth=0) for s in seeds)
    _, r, _ = run(a, b)
    assert r["status"] in (6, 7)
    d = cm.decide(r["sad"], R, C, 800)
    assert d["S_best"] * 1000 > 800 * d["S2"]       # above the default threshold, whatever else the status order reports
    if abs(d["dx"]) != R and abs(d["dy"]) != R:
        assert r["status"] == 7


@pytest.mark.parametrize("seeds", NOISE_SEEDS)
def test_noise_pairs_used_by_the_gpu_tests_are_status_7(seeds):
    """the GPU tests take the first seed pair whose minimum is not at the border"""
    a, b = (cm.texture(H, W, seed=s, smooth=0) for s in seeds)
    _, r, _ = run(a, b)
    if seeds == NOISE_SEEDS[0]:
        assert r["status"] == 7


def test_good_frames_stay_below_the_threshold():
    for d in ((1, 0), (3, 2), (-3, 1)):
        _, r, _ = run(*pair(*d))
        assert r["S_best"] * 1000 <= 800 * r["S2"] and r["status"] == 1


def test_half_cell_shift_on_a_smooth_picture():
    canvas = cm.texture(H + 64, W + 64, seed=7, smooth=6)
    a = cm.view(canvas, 32, 32, W, H)
    b = cm.view(canvas, 32 - (C + C // 2), 32, W, H)       # 1.5 cells to the right
    _, r, _ = run(a, b)
    assert r["status"] == 1 and r["dx"] in (1, 2) and r["dy"] == 0
    assert np.all(np.abs(r["off"]) <= F(0.5))
    assert abs(float(r["shift"][0]) - 1.5 * C) <= C / 2 and abs(float(r["shift"][1])) <= C / 2


def test_sign_flip_mutation_fails():
    a, b = pair(3, 2)
    _, r, _ = run(a, b, sign=-1)
    assert (r["dx"], r["dy"]) == (-3, -2)


def test_s2_neighbourhood_mutation_fails():
    """with the neighbourhood taken at distance 0, S2 is a direct neighbour of the minimum: on a smooth picture a good
    shift then reads as ambiguous"""
    canvas = cm.texture(H + 64, W + 64, seed=7, smooth=6)
    a, b = pair(2, 1, canvas=canvas)
    _, good, _ = run(a, b, conf_pm=300)
    _, bad, _ = run(a, b, conf_pm=300, s2_dist=0)
    assert good["status"] == 1 and bad["S2"] < good["S2"]
    a, b = cm.view(canvas, 32, 32, W, H), cm.view(canvas, 30, 31, W, H)      # half a cell: the neighbour is nearly as good
    _, good, _ = run(a, b)
    _, bad, _ = run(a, b, s2_dist=0)
    assert good["status"] == 1 and bad["status"] == 7


def test_geometry_and_automatic_cell():
    assert cm.geometry(160, 96, 0, 4, 65536) == dict(status=1, c=4, Wg=40, Hg=24)
    assert cm.geometry(157, 93, 0, 4, 65536) == dict(status=1, c=4, Wg=39, Hg=23)
    assert cm.geometry(160, 96, 0, 4, 40 * 24 - 1)["c"] == 8
    assert cm.geometry(1920, 1080, 0, 8, 65536) == dict(status=1, c=8, Wg=240, Hg=135)
    assert cm.geometry(160, 96, 4, 4, 40 * 24 - 1)["status"] == 2          # a fixed cell over max_cells
    assert cm.geometry(160, 96, 0, 9, 65536)["status"] == 2                # 24 - 18 < 8
    assert cm.geometry(160, 96, 0, 8, 65536)["status"] == 1                # 24 - 16 == 8
    assert cm.geometry(1 << 17, 1 << 17, 0, 8, 4096) == dict(status=2, c=0, Wg=0, Hg=0)     # no cell up to 64 fits


def test_statuses_that_drop_the_previous_thumbnail():
    a, b = pair(1, 0)
    s = cm.Stream()
    box = (60, 40, 20, 20)
    assert s.step(a, box, cell=C, R=R)["status"] == 5
    assert s.step(b, box, cell=C, R=R, device=False)["status"] == 4 and not s.has_prev
    assert s.step(b, box, cell=C, R=R)["status"] == 5
    assert s.step(a, box, cell=C, R=R, mode=0)["status"] == 0 and not s.has_prev
    assert s.step(a, box, cell=C, R=R)["status"] == 5
    assert s.step(b, box, cell=C, R=12)["status"] == 2 and not s.has_prev
    assert s.step(a, box, cell=C, R=R)["status"] == 5
    assert s.step(b, box, cell=8, R=2)["status"] == 5      # another cell: the old thumbnail does not fit
    assert s.step(a, box, cell=8, R=2)["status"] == 1
    s.reset()
    assert s.step(b, box, cell=8, R=2)["status"] == 5


def test_apply_keeps_the_centre_inside_the_frame():
    b, applied = cm.apply_shift((150, 40, 20, 20), np.array([4, 0], F), 160, 96)
    assert applied == 0 and b.tolist() == [150, 40, 20, 20]         # the centre would be 164
    b, applied = cm.apply_shift((140, 40, 20, 20), np.array([8, -4], F), 160, 96)
    assert applied == 1 and b.tolist() == [148, 36, 20, 20]
    b, applied = cm.apply_shift((-8, 40, 20, 20), np.array([-4, 0], F), 160, 96)
    assert applied == 0
    b, applied = cm.apply_shift((0, 0, 20, 20), np.zeros(2, F), 160, 96)
    assert applied == 0


def test_sums_above_31_bits_are_exact():
    """every cell 4080 against 0 on the largest grid max_cells allows, the overflow case of the GPU tests: n * 4080 =
    4,244,832,000 lies above 2^31 (a signed 32-bit sum goes wrong) and, with n < 2^20 cells, just below 2^32"""
    cur, prev = np.full((1024, 1024), 4080, np.uint16), np.zeros((1024, 1024), np.uint16)
    S = cm.sad_table(cur, prev, 2)
    assert (S == 1020 * 1020 * 4080).all() and 1 << 31 < S[0, 0] < 1 << 32
    assert cm.thumbnail(np.full((8, 8, 3), 255, np.uint8), 4, 2, 2).tolist() == [[4080, 4080], [4080, 4080]]
