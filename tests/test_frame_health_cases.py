"""The rule of the frame health on its NumPy model alone (tests/frame_health_util.py; the rule to the bit:
include/vittrack_hip_ops.h, vt_op_frame_health): what the GPU tests hold the kernels to must itself do what the rule says,
and the mutations a slip in a kernel would be must change the outcome of a case here. No GPU."""
import numpy as np
import pytest

import frame_health_util as fh

W, H, C = 160, 100, 4           # 40 x 25 = 1000 cells
N = (W // C) * (H // C)
CANVAS = fh.texture(H, W, seed=21)


def run(frames, **kw):
    """the frames through one stream, frames_done counting from 0 -> the records"""
    s = fh.Stream()
    kw.setdefault("cell", C)
    return [s.step(f, frames_done=k, **kw) for k, f in enumerate(frames)], s


def moved(k, v_from=10, v_to=200):
    """a grey picture, and the same with exactly k cells (row-major from the top left) at another grey"""
    a = fh.grey(H, W, v_from)
    b = a.copy()
    for cell in range(k):
        j, i = divmod(cell, W // C)
        b[j * C:(j + 1) * C, i * C:(i + 1) * C] = v_to
    return a, b


def test_known_measures_of_a_grey_frame_and_of_half_planes():
    (r,), s = run([fh.grey(H, W, 100)])
    assert (r["status"], r["c"], r["Wg"], r["Hg"]) == (5, C, 40, 25)
    assert (r["S1"], r["S2"], r["G"], r["D"], r["HD"], r["still"]) == (N * 1600, N * 1600 * 1600, 0, 0, 0, 0)
    assert r["hist"][1600 >> 7] == N and r["hist"].sum() == N and r["flags"] == fh.FLAT
    (r,), _ = run([fh.halves(H, W, 10, 250)])
    assert r["S1"] == N // 2 * (160 + 4000) and r["G"] == 25 * 3840 and r["G_ref"] == r["G"]
    assert N * r["S2"] - r["S1"] ** 2 == (8 * 240) ** 2 * N * N       # the standard deviation is 8 |v1 - v2|


@pytest.mark.parametrize("v1,v2", [(100, 104), (0, 255), (30, 29)])
def test_flat_exactly_on_and_one_below_the_bound(v1, v2):
    q = 8 * abs(v1 - v2)
    pic = fh.halves(H, W, v1, v2)
    assert run([pic], flat_q=q)[0][0]["flags"] == fh.FLAT
    assert run([pic], flat_q=q - 1)[0][0]["flags"] == 0
    assert run([pic], flat_q=q, strict=True)[0][0]["flags"] == 0        # the mutation < for <=
    assert run([pic, pic], flat_q=q)[0][1]["flags"] == fh.FLAT          # status 1 flags it too


def test_flat_q_0_flags_a_constant_picture_only():
    assert run([fh.grey(H, W, 7)], flat_q=0)[0][0]["flags"] == fh.FLAT
    assert run([fh.halves(H, W, 7, 8)], flat_q=0)[0][0]["flags"] == 0


@pytest.mark.parametrize("cut_pm,k", [(500, 500), (250, 250), (1000, 1000), (1, 1)])
def test_cut_with_exactly_k_cells_in_another_bin(cut_pm, k):
    a, b = moved(k)
    r = run([a, b], cut_pm=cut_pm, flat_q=0)[0][1]
    assert (r["status"], r["HD"]) == (1, 2 * k) and 2 * k * 1000 == cut_pm * 2 * N and r["flags"] & fh.CUT
    a, b = moved(k - 1)
    r = run([a, b], cut_pm=cut_pm, flat_q=0)[0][1]
    assert r["HD"] == 2 * (k - 1) and not r["flags"] & fh.CUT


def test_cut_pm_0_never_cuts_and_status_5_never_cuts():
    a, b = moved(N)
    recs, _ = run([a, b], cut_pm=0, flat_q=0)
    assert recs[1]["HD"] == 2 * N and recs[1]["flags"] == fh.FLAT       # a constant picture is flat at any flat_q
    assert run([a, b[:, :W - C]], flat_q=0)[0][1]["status"] == 5        # another geometry: nothing to compare with


def test_bins_are_128_wide():
    """greys 1 and 5 give cells of 16 and 80: one bin of t >> 7, two bins of t >> 6"""
    a, b = moved(N, 1, 5)
    r = run([a, b], flat_q=0)[0][1]
    assert (r["HD"], r["flags"], r["D"]) == (0, fh.FLAT, N * 64)
    r = run([a, b], flat_q=0, shift=6)[0][1]
    assert r["HD"] == 2 * N and r["flags"] == fh.FLAT | fh.CUT          # the mutation >> 6
    a, b = moved(N, 7, 8)                                               # 112 and 128: two bins
    assert run([a, b], flat_q=0)[0][1]["flags"] == fh.FLAT | fh.CUT


def test_frozen_at_the_still_run_th_identical_comparison_and_reset_by_one_tap():
    pic = CANVAS
    recs, _ = run([pic] * 5, still_run=3)
    assert [r["status"] for r in recs] == [5, 1, 1, 1, 1]
    assert [r["still"] for r in recs] == [0, 1, 2, 3, 4] and [r["flags"] for r in recs] == [0, 0, 0, fh.FROZEN, fh.FROZEN]
    assert [r["flags"] for r in run([pic] * 4, still_run=3, still5=True)[0]] == [0, 0, fh.FROZEN, fh.FROZEN]     # the mutation
    one = pic.copy()
    y = x = C // 8                                                      # the first tap of cell (0, 0)
    one[y, x] = (255 - one[y, x].astype(int)).astype(np.uint8)
    recs, _ = run([pic, pic, pic, one, one], still_run=2)
    assert [r["still"] for r in recs] == [0, 1, 2, 0, 1] and [r["flags"] for r in recs] == [0, 0, fh.FROZEN, 0, 0]
    assert recs[3]["D"] == abs(int(recs[3]["thumb"][0, 0]) - int(recs[2]["thumb"][0, 0])) > 0
    off = pic.copy()
    off[0, 0] = 255 - off[0, 0]
    assert run([pic, off], cell=8)[0][1]["D"] == 0                      # cell 8: taps at 1, 3, 5, 7 - pixel (0, 0) is none


def test_still_run_1_flags_the_first_identical_comparison():
    recs, _ = run([CANVAS] * 2, still_run=1)
    assert [r["flags"] for r in recs] == [0, fh.FROZEN]


def test_g_and_g_ref():
    stripes = fh.grey(H, W, 0)
    for j in range(0, H, 2 * C):
        stripes[j:j + C] = 255                                          # rows of cells alternate 4080 / 0: only vertical differences
    (r,), _ = run([stripes])
    assert r["G"] == 24 * 40 * 4080 and r["G_ref"] == r["G"]
    assert run([stripes], vertical=False)[0][0]["G"] == 0               # the mutation: G without its vertical term
    a = fh.halves(H, W, 10, 50)
    recs, s = run([a, a, stripes, stripes], flat_q=0)
    assert [r["flags"] & fh.CUT for r in recs] == [0, 0, fh.CUT, 0]
    assert [r["G_ref"] for r in recs] == [recs[0]["G"], recs[0]["G"], recs[2]["G"], recs[2]["G"]] and recs[0]["G"] != recs[2]["G"]
    assert [r["flags"] for r in recs] == [0, 0, fh.CUT, 0] and (s.evaluated, s.flagged) == (4, 1)


def test_period_and_not_due_passes_keep_the_previous_thumbnail():
    recs, s = run([CANVAS] * 5, period=2, still_run=2)
    assert [r["status"] for r in recs] == [5, 0, 1, 0, 1] and [r.get("still") for r in recs] == [0, None, 1, None, 2]
    assert recs[4]["flags"] == fh.FROZEN and s.evaluated == 3
    assert [r["status"] for r in run([CANVAS] * 3, period=2, drop=True)[0]] == [5, 0, 5]     # the mutation
    assert [r["status"] for r in run([CANVAS] * 3, on=0)[0]] == [0, 0, 0]
    assert [r["status"] for r in run([CANVAS] * 2, initialised=False)[0]] == [0, 0]


def test_statuses_4_and_2_clear_the_previous_thumbnail_and_still():
    s = fh.Stream()
    assert s.step(CANVAS, cell=C, frames_done=0)["status"] == 5
    assert s.step(CANVAS, cell=C, frames_done=1)["still"] == 1
    r = s.step(CANVAS, cell=C, frames_done=2, device=False)
    assert (r["status"], r["S1"], r["G"], r["flags"], r["still"], r["G_ref"]) == (4, 0, 0, 0, 0, 0) and s.has_prev == 0
    assert s.step(CANVAS, cell=C, frames_done=3)["status"] == 5
    r = s.step(CANVAS, cell=C, frames_done=4, max_cells=999)
    assert (r["status"], r["c"], r["Wg"], r["Hg"], r["S1"]) == (2, C, 40, 25, 0) and s.has_prev == 0
    assert s.step(CANVAS[:28], cell=C, frames_done=5)["status"] == 2    # Hg = 7
    assert s.step(CANVAS[:32], cell=C, frames_done=6)["status"] == 5    # Hg = 8
    assert s.step(CANVAS, cell=C, frames_done=7, whole=False)["status"] == 4
    assert (s.evaluated, s.flagged) == (4, 0)


def test_automatic_cell_and_the_largest_sums():
    g = fh.geometry(260, 256, 0, 4096)
    assert (g["c"], g["Wg"], g["Hg"], g["status"]) == (8, 32, 32, 1)
    assert fh.geometry(260, 256, 4, 4096)["status"] == 2 and fh.geometry(256, 256, 4, 4096)["status"] == 1
    n = 262144
    S1, S2 = n * 4080, n * 4080 * 4080                                  # a white-out at max_cells
    assert S2 > 1 << 32 and n * S2 < 1 << 61 and S1 * S1 < 1 << 61 and 4080 * 4080 * n * n < 1 << 61
    assert fh.is_flat(n, S1, S2, 0)
    S1, S2 = n // 2 * 4080, n // 2 * 4080 * 4080                        # half black, half white: the deviation is 2040
    assert fh.is_flat(n, S1, S2, 2040) and not fh.is_flat(n, S1, S2, 2039)
