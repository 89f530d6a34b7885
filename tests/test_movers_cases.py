"""Moving regions on the CPU: the NumPy model of tests/movers_util.py against hand-built masks whose records are written
out here by hand, six mutations of the rule that must each break at least one of these cases, the key table in a stand-alone
program under host sanitizers, and what the change adds to the boundary (one operator hook in the ops library; no product
function, no new ABI version). No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import movers_util as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gstreamer-vit-tracker_amd", "csrc")
HG, WG, C = 12, 16, 4
G = dict(status=1, c=C, Wg=WG, Hg=HG)
BASE, STEP = 1000, 500          # thumbnail values: the background, and what a painted cell adds (16 * 500 > 16 * 96)


def run(mask, mut=None, box=(0, 0, 0, 0), model=None, **pol):
    """a fresh stream: the background from a flat thumbnail, then the thumbnail with `mask` painted. min_nb 1 unless stated:
    the kept cells are the mask's"""
    m = model or mv.Stream()
    p = dict(dict(min_nb=1, min_area=1), **pol)
    if model is None:
        first = m.step_thumb(np.full((HG, WG), BASE), G, (WG * C, HG * C), box, **p, **(mut or {}))
        assert first["status"] == 5 and first["n"] == 0 and np.array_equal(first["bg"], np.full((HG, WG), 16 * BASE))
    return m.step_thumb(BASE + STEP * np.asarray(mask, np.int64), G, (WG * C, HG * C), box, frames_done=1, **p, **(mut or {}))


def boxes(rec):
    return [(b["box"], b["area"], b["label"]) for b in rec["boxes"]]


def counts(rec):
    return tuple(rec[k] for k in ("status", "n", "moving", "kept", "components"))


# ---- the cases: each takes the mutation (None: the rule) and asserts the record written out by hand -----------------------

def case_empty(mut):
    r = run(np.zeros((HG, WG), bool), mut)
    assert counts(r) == (1, 0, 0, 0, 0) and boxes(r) == [] and (r["labels"] == -1).all()


def case_one_cell(mut):
    r = run(mv.place(mv.parse(["#"]), HG, WG, 3, 5), mut)
    assert counts(r) == (1, 1, 1, 1, 1) and boxes(r) == [((20, 12, 4, 4), 1, 53)]


def case_diagonal_touch(mut):
    m = mv.place(mv.parse(["##", "##"]), HG, WG, 2, 2) | mv.place(mv.parse(["##", "##"]), HG, WG, 4, 4)
    r = run(m, mut)
    assert counts(r) == (1, 1, 8, 8, 1) and boxes(r) == [((8, 8, 16, 16), 8, 34)]


def case_u(mut):
    r = run(mv.place(mv.U_SHAPE, HG, WG, 1, 2), mut)
    assert counts(r) == (1, 1, 11, 11, 1) and boxes(r) == [((8, 4, 20, 16), 11, 18)]


def case_spiral(mut):
    assert int(mv.SPIRAL.sum()) == 49
    r = run(mv.place(mv.SPIRAL, HG, WG, 1, 1), mut, global_pm=1000)
    assert counts(r) == (1, 1, 49, 49, 1) and boxes(r) == [((4, 4, 36, 36), 49, 17)]
    assert set(np.unique(r["labels"])) == {-1, 17}


def case_comb(mut):
    r = run(mv.place(mv.COMB, HG, WG, 2, 2), mut)
    assert counts(r) == (1, 1, 29, 29, 1) and boxes(r) == [((8, 8, 44, 16), 29, 34)]


def case_four_borders(mut):
    m = np.zeros((HG, WG), bool)
    m[6, :] = True
    m[:, 8] = True
    r = run(m, mut)
    assert counts(r) == (1, 1, 27, 27, 1) and boxes(r) == [((0, 0, 64, 48), 27, 8)]


def case_one_more_than_max_with_a_tie_at_the_cut(mut):
    m = mv.place(mv.parse(["###"]), HG, WG, 9, 1) | mv.place(mv.parse(["##"]), HG, WG, 2, 8) | mv.place(mv.parse(["#", "#"]), HG, WG, 5, 3)
    r = run(m, mut, max_n=2)
    # areas 3 (label 145), 2 (label 40), 2 (label 83): the tie goes to the smaller label, the third is cut
    assert counts(r) == (1, 2, 7, 7, 3) and boxes(r) == [((4, 36, 12, 4), 3, 145), ((32, 8, 8, 4), 2, 40)]
    r = run(m, mut, max_n=3)
    assert boxes(r)[2] == ((12, 20, 4, 8), 2, 83)


def case_min_area(mut):
    m = mv.place(mv.parse(["##", "##"]), HG, WG, 5, 5)
    for min_area, n in ((3, 1), (4, 1), (5, 0)):
        r = run(m, mut, min_area=min_area)
        assert counts(r) == (1, n, 4, 4, 1) and boxes(r) == [((20, 20, 8, 8), 4, 85)][:n]


def case_global_change(mut):
    # 192 cells at 250 per mille: moving * 1000 > 48000, i.e. 49 cells and more
    for cells, status in ((47, 1), (48, 1), (49, 6)):
        m = np.zeros(HG * WG, bool)
        m[:cells] = True
        r = run(m.reshape(HG, WG), mut, global_pm=250)
        assert counts(r) == (status, 1 if status == 1 else 0, cells, cells, 1 if status == 1 else 0)
        # an empty own box has no kept cell while others are kept: still counts at status 1 and is cleared at status 6
        assert r["still"] == (1 if status == 1 else 0) and (boxes(r) == [] if status == 6 else boxes(r)[0][1:] == (cells, 0))
    r = run(np.ones((HG, WG), bool), mut, global_pm=1000)      # never
    assert counts(r) == (1, 1, 192, 192, 1) and boxes(r) == [((0, 0, 64, 48), 192, 0)]


def case_threshold(mut):
    """a difference of exactly 16 thr does not move; 16 more does. With learn 4 the updated background is 1/16 nearer: a mask
    taken from it would lose the cell that is only just over"""
    for delta, moving in ((96, 0), (97, 1), (-96, 0), (-97, 1), (100, 1)):
        m = mv.Stream()
        m.step_thumb(np.full((HG, WG), BASE), G, (64, 48), min_nb=1, min_area=1, **(mut or {}))
        t = np.full((HG, WG), BASE)
        t[4, 4] += delta
        r = m.step_thumb(t, G, (64, 48), frames_done=1, min_nb=1, min_area=1, thr=96, learn=4, **(mut or {}))
        assert r["moving"] == moving and r["n"] == moving, delta
        assert int(r["bg"][4, 4]) == 16 * BASE + ((16 * delta) >> 4) and int(r["bg"][0, 0]) == 16 * BASE


def case_learn_and_the_floor_rule(mut):
    """learn 8 and a small negative d: the arithmetic shift moves the background by -1, a division that truncates by 0"""
    for learn, delta, bg in ((8, -1, 15999), (8, 1, 16000), (8, -16, 15999), (8, -17, 15998), (8, 16, 16001), (0, -1, 15984), (0, 3, 16048),
                             (4, -1, 15999), (4, 1, 16001)):
        m = mv.Stream()
        m.step_thumb(np.full((HG, WG), BASE), G, (64, 48), **(mut or {}))
        r = m.step_thumb(np.full((HG, WG), BASE + delta), G, (64, 48), frames_done=1, learn=learn, **(mut or {}))
        assert r["status"] == 1 and r["moving"] == 0 and (r["bg"] == bg).all(), (learn, delta, int(r["bg"][0, 0]))
    # three passes: the second's background is the first's output
    m = mv.Stream()
    m.step_thumb(np.full((HG, WG), BASE), G, (64, 48), **(mut or {}))
    t = np.full((HG, WG), BASE)
    t[2:5, 2:5] += STEP
    a = m.step_thumb(t, G, (64, 48), frames_done=1, learn=4, **(mut or {}))
    b = m.step_thumb(t, G, (64, 48), frames_done=2, learn=4, **(mut or {}))
    assert int(a["bg"][3, 3]) == 16500 and int(b["bg"][3, 3]) == 16968 and (a["kept"], b["kept"]) == (9, 9)
    assert (m.evaluated, m.listed) == (2, 2)


def case_the_ends_of_the_range(mut):
    """t = 0 and t = 4080: d = +-65,280, the background reaches 65,280 and 0, thr 4079 moves and thr 4080 cannot"""
    for first, second in ((0, 4080), (4080, 0)):
        for thr, moving in ((4079, 192), (4080, 0)):
            m = mv.Stream()
            a = m.step_thumb(np.full((HG, WG), first), G, (64, 48), **(mut or {}))
            r = m.step_thumb(np.full((HG, WG), second), G, (64, 48), frames_done=1, thr=thr, learn=0, global_pm=1000, min_nb=1, **(mut or {}))
            assert (a["bg"] == 16 * first).all() and (r["bg"] == 16 * second).all() and r["moving"] == moving, (first, thr)


def case_clean_up(mut):
    """a 2 x 2 block keeps its four cells at min_nb 4, a lone cell goes; three cells in the corner have three moving
    neighbours each at most: none is kept at min_nb 4 - unless the cells beyond the border counted"""
    m = mv.place(mv.parse(["##", "##"]), HG, WG, 5, 5) | mv.place(mv.parse(["#"]), HG, WG, 9, 12)
    r = run(m, mut, min_nb=4)
    assert counts(r) == (1, 1, 5, 4, 1) and boxes(r) == [((20, 20, 8, 8), 4, 85)]
    assert r["mask"][9, 12] == 1 and r["mask"][5, 5] == 2 and r["mask"][0, 0] == 0
    r = run(mv.place(mv.parse(["##", "#."]), HG, WG, 0, 0), mut, min_nb=4)
    assert counts(r) == (1, 0, 3, 0, 0)
    r = run(mv.place(mv.parse([".#", "##"]), HG, WG, HG - 2, WG - 2), mut, min_nb=3)       # the opposite corner, one less asked
    assert counts(r) == (1, 1, 3, 3, 1) and boxes(r) == [((56, 40, 8, 8), 3, 175)]
    line = run(mv.place(mv.parse(["#####"]), HG, WG, 3, 3), mut, min_nb=3)      # the ends of a line have two
    assert counts(line) == (1, 1, 5, 3, 1) and boxes(line) == [((16, 12, 12, 4), 3, 52)]
    assert run(np.ones((HG, WG), bool), mut, min_nb=9, global_pm=1000)["kept"] == (HG - 2) * (WG - 2)


def case_own_box_and_still(mut):
    blob = mv.place(mv.parse(["##", "##"]), HG, WG, 5, 5)        # pixels 20..28 both ways
    m = mv.Stream()
    r = run(blob, mut, box=(21.5, 22.0, 5.0, 9.5))                # cells 5..6 x 5..7: floor(5.375), ceil(6.625); floor(5.5), ceil(7.875)
    assert (r["own_cells"], r["own_kept"], r["still"]) == (6, 4, 0)
    m = mv.Stream()
    m.step_thumb(np.full((HG, WG), BASE), G, (64, 48), (40.0, 0.0, 8.0, 8.0), **(mut or {}))
    stills = []
    for k, mask in enumerate((blob, blob, np.zeros((HG, WG), bool), blob)):
        r = run(mask, mut, box=(40.0, 0.0, 8.0, 8.0), model=m, learn=8)
        stills.append((r["own_cells"], r["own_kept"], r["still"]))
    assert stills == [(4, 0, 1), (4, 0, 2), (4, 0, 0), (4, 0, 1)]
    r = run(blob, mut, box=(-30.0, -4.0, 20.0, 10.0))            # left of the frame: clipped to nothing in x
    assert (r["own_cells"], r["own_kept"]) == (0, 0)
    r = run(blob, mut, box=(0.0, 0.0, 1000.0, 1000.0))
    assert (r["own_cells"], r["own_kept"], r["still"]) == (192, 4, 0)


CASES = [case_empty, case_one_cell, case_diagonal_touch, case_u, case_spiral, case_comb, case_four_borders,
         case_one_more_than_max_with_a_tie_at_the_cut, case_min_area, case_global_change, case_threshold,
         case_learn_and_the_floor_rule, case_the_ends_of_the_range, case_clean_up, case_own_box_and_still]
MUTATIONS = [dict(conn=4), dict(ge=True), dict(label="max"), dict(ties="reverse"), dict(outside=True), dict(update_first=True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_the_model_gives_the_hand_written_records(case):
    case(None)


@pytest.mark.parametrize("mut", MUTATIONS, ids=lambda m: "-".join(f"{k}={v}" for k, v in m.items()))
def test_every_mutation_breaks_a_case(mut):
    broken = []
    for case in CASES:
        try:
            case(mut)
        except AssertionError:
            broken.append(case.__name__)
    assert broken, mut


def test_statuses_and_bookkeeping():
    m = mv.Stream()
    t = np.full((HG, WG), BASE)
    assert m.step_thumb(t, G, (64, 48), on=0) == dict(status=0) and m.step_thumb(t, G, (64, 48), initialised=False) == dict(status=0)
    assert m.step_thumb(t, G, (64, 48), period=3, frames_done=4) == dict(status=0) and m.rec is None
    assert [m.step_thumb(t, G, (64, 48), frames_done=k)["status"] for k in range(2)] == [5, 1]
    r = m.step_thumb(None, dict(status=4, c=0, Wg=0, Hg=0), (64, 48))
    assert r["status"] == 4 and m.has_bg == 0 and r["has_bg"] == 0
    assert [m.step_thumb(t, G, (64, 48))["status"] for _ in range(2)] == [5, 1]
    assert m.step_thumb(t, G, (128, 48))["status"] == 5                 # another W
    assert m.step_thumb(t, dict(G, c=8), (128, 48))["status"] == 5      # another c
    assert m.step_thumb(None, dict(status=2, c=4, Wg=7, Hg=12), (28, 48))["status"] == 2 and m.has_bg == 0
    m.reset()
    assert m.step_thumb(t, G, (64, 48))["status"] == 5 and (m.evaluated, m.listed) == (2, 0)


def test_a_serpentine_is_one_component_and_paint_lands_on_the_values():
    s = mv.serpentine(HG, WG)
    lab = mv.components(s)
    assert set(np.unique(lab)) == {-1, 0} and int((lab == 0).sum()) == int(s.sum()) == 6 * WG + 5
    assert len(np.unique(mv.components(s, conn=4))) == 2
    pic = mv.paint(s, C, base=60, value=200)
    assert pic.shape == (HG * C, WG * C, 3)
    assert np.array_equal(mv.thumbnail(pic, C, WG, HG), np.where(s, 3200, 960))


def test_own_rect_is_floor_and_ceil_clipped():
    assert mv.own_rect((21.5, 22.0, 5.0, 9.5), 4, 16, 12) == (5, 5, 7, 8)
    assert mv.own_rect((20.0, 20.0, 8.0, 8.0), 4, 16, 12) == (5, 5, 7, 7)       # on the cell lines: nothing added
    assert mv.own_rect((-5.0, 47.9, 5.1, 10.0), 4, 16, 12) == (0, 11, 1, 12)
    assert mv.own_rect((70.0, 60.0, 5.0, 5.0), 4, 16, 12) == (16, 12, 16, 12)


# ---- the key table under host sanitizers ------------------------------------------------------------------------------------

def test_movers_key_table_under_sanitizers(tmp_path):
    exe = tmp_path / "movers_keys_main"
    # the runtimes linked statically: the program then starts whatever else the environment preloads into processes
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "movers_keys_main.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 checks failed"), r.stdout[-4000:] + r.stderr[-4000:]


# ---- the boundary -----------------------------------------------------------------------------------------------------------

KEYS = ("movers", "movers_period", "movers_cell", "movers_learn", "movers_thr", "movers_min_nb", "movers_min_area", "movers_global_pm",
        "movers_max", "movers_max_cells")


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("vt_")}


def test_the_hook_is_in_the_ops_library_only_and_the_product_still_exports_91(vt):
    txt = re.sub(r"/\*.*?\*/", "", _header("vittrack_hip.h"), flags=re.S)
    names = set(re.findall(r"\b(vt_[a-z0-9_]+)\s*\(", txt))
    assert len(names) == 91 and set(vt.EXPORTS) == names and _exports(vt.LIB_PATH) == names
    assert "#define VT_ABI_VERSION 5" in _header("vittrack_hip.h").replace("  ", " ")
    ops = re.sub(r"/\*.*?\*/", "", _header("vittrack_hip_ops.h"), flags=re.S)
    assert re.search(r"\bint\s+vt_op_movers\s*\(", ops)
    assert "vt_op_movers" in vt.OPS_EXPORTS and "vt_op_movers" not in vt.EXPORTS
    assert "vt_op_movers" in _exports(vt.OPS_LIB_PATH) and "vt_op_movers" not in _exports(vt.LIB_PATH)


def test_keys_records_and_the_python_binding(vt):
    keys = open(os.path.join(CSRC, "vt_feature_keys.hpp")).read()
    for k in KEYS:
        assert keys.count(f'{{"{k}", ') == 1, k
        assert f'"{k}"' in _header("vittrack_hip_ops.h"), k
    assert "constexpr int kMaxWords = 8;" in keys and "MV_WORDS = 8" in keys
    assert vt.MOVERS_REC_DTYPE.itemsize == 256 and vt.MOVERS_REC_DTYPE.fields["box"][1] == 64 and vt.MOVERS_BOX_DTYPE.itemsize == 24
    hpp = open(os.path.join(CSRC, "k_movers.hpp")).read()
    assert "sizeof(MoverRec) == 256" in hpp and "offsetof(MoverRec, box) == 64" in hpp
    src = open(os.path.join(CSRC, "k_movers.hip")).read()
    assert '#include "k_thumb_dev.hpp"' in src and "thumb_cell<ANY>(" in src and "double" not in src
    assert callable(vt.op_movers) and vt.movers_shape(4, 3, 4) == 4 | 3 << 4 | 4 << 8
