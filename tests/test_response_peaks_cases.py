"""Response peaks, the reference side (no GPU): the case sets of tests/peaks_util.py satisfy the conditions that keep device
expf out of every comparison, the specification treats a -inf score logit as response 0, the float32 specification and its
float64 restatement list the same cells, and a few answers are known by hand."""
import numpy as np
import pytest

import decode_util as du
import peaks_util as pu


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_case_sets_keep_rounding_out_of_every_decision(grid, C, capsys):
    lines = []
    for s in pu.all_sets(grid, C):
        lines.append(s.report())
        assert s.same_cells, f"{s.name} R {s.R}: the float32 specification and the float64 restatement list different cells"
        if not s.exact:
            assert s.lead.min() >= pu.MARGIN, f"{s.name} R {s.R}: a listed peak leads by {s.lead.min():.2e}"
            assert s.thr.min() >= pu.MARGIN, f"{s.name} R {s.R}: a response lies {s.thr.min():.2e} from min_resp"
            if not getattr(s, "allow_nonfinite", False):
                assert s.finite.all(), f"{s.name} R {s.R}: {int((~s.finite).sum())} cases have no finite float64 box"
        # the set's own float32 - float64 distance against the shape's bar (4 x the decode sweep's distance)
        assert s.dist <= 0.25 * s.tol, f"{s.name} R {s.R}: |f32 - f64| {s.dist:.3e} against a bar of {s.tol:.3e}"
    with capsys.disabled():
        print("\n" + "\n".join(lines))


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_the_sets_exercise_what_they_are_for(grid, C):
    for R in (1, 2, 3, 4):
        p = pu.planted(grid, C, R)
        assert p.ora["n"].min() >= 1 and p.ora["n"].max() <= 5
        if 2 * (2 * R + 1) <= grid:         # room for squares side by side: most cases list several peaks, some many
            assert (p.ora["n"] >= 2).mean() > 0.5 and p.ora["n"].max() >= 3, (R, p.ora["n"])
        assert np.all(p.ora["resp"][p.ora["cell"] >= 0] >= 0.42)
        b = pu.border(grid, C, R)
        assert np.array_equal(b.ora["cell"][:, 0], np.arange(grid * grid)), "every cell is some case's peak 0"
        two = b.ora["n"] == 2
        assert np.array_equal(b.ora["cell"][two, 1], b.second[two]) and (b.ora["n"] <= 2).all()
        xs, ys = np.arange(grid * grid) % grid, np.arange(grid * grid) // grid
        inside = (np.abs(b.second % grid - xs) <= R) & (np.abs(b.second // grid - ys) <= R)
        assert np.array_equal(two, ~inside), "a second maximum outside the square is listed, one inside is not"
        if R + 1 < grid:
            a = pu.apart(grid, C, R)
            assert a.ora["n"].tolist() == [1, 2, 2]
            assert np.all(np.isfinite(a.ora["fbox"][1, 1])) and a.ora["fbox"][2, 1, 0] == 0.0 and a.ora["fbox"][2, 1, 2] == 10.0
            assert a.ora["fbox"][2, 1, 3] == a.ora["fbox"][1, 1, 3], "only x is touched by the NaN x-offset"
    # corners and edges: second windows of 4 and 6 cells occur
    b = pu.border(grid, C, 1)
    sx, sy = b.second % grid, b.second // grid
    listed = b.ora["n"] == 2
    edge = (sx == 0) | (sx == grid - 1) | (sy == 0) | (sy == grid - 1)
    corner = ((sx == 0) | (sx == grid - 1)) & ((sy == 0) | (sy == grid - 1))
    assert (listed & corner).any() and (listed & edge & ~corner).any()


def test_a_minus_inf_score_logit_is_response_zero(oracle):
    """bit test: the suppressed cell contributes weight +0 and the map with everything suppressed decodes cell 0, score 0,
    box (0, 0, 10, 10)"""
    grid = 8
    ns = grid * grid
    lg = np.zeros((1, ns, 5), np.float32)
    lg[0, :, 0] = -np.inf
    hann = du.lifted_hann(grid).reshape(-1)
    st = du._plain_states(1, 1)
    o = du.decode_oracle(lg, hann, grid, st["geo"], st["frame_w"], st["frame_h"])
    assert o["idx"][0] == 0 and o["score"].view(np.uint32)[0] == 0 and o["fbox"][0].tolist() == [0.0, 0.0, 10.0, 10.0]
    # one live cell beside suppressed neighbours: the box is that cell's alone (the neighbours' weights are exactly 0)
    lg[0, 27, 0] = 2.0
    rng = np.random.default_rng(5)
    lg[0, :, 1:] = rng.standard_normal((ns, 4)).astype(np.float32)
    alone = du.decode_oracle(lg, hann, grid, st["geo"], st["frame_w"], st["frame_h"])
    lg2 = lg.copy()
    lg2[0, :, 1:] = 0.0
    lg2[0, 27, 1:] = lg[0, 27, 1:]
    other = du.decode_oracle(lg2, hann, grid, st["geo"], st["frame_w"], st["frame_h"])
    assert alone["idx"][0] == 27 and np.array_equal(alone["fbox"].view(np.uint32), other["fbox"].view(np.uint32))


@pytest.mark.parametrize("grid,C", du.SHAPES)
def test_known_answers(grid, C):
    for R in (1, 2, 4):
        f = pu.flat(grid, C, R)
        want = pu.flat_expected(grid, R)
        assert f.ora["n"][0] == len(want) and f.ora["cell"][0, :len(want)].tolist() == want, (grid, R)
        assert f.f64["cell"][0, :len(want)].tolist() == want
        assert want[:2] == [0, R + 1] and np.all(f.ora["resp"][0, :len(want)] == np.float32(0.5))
    if grid == 8:
        f = pu.flat(8, C, 4)
        assert f.ora["n"][0] == 4 and f.ora["cell"][0, :4].tolist() == [0, 5, 40, 45]
    t = pu.tie_order(grid, C)
    names = list(du.tie_sets(grid))
    i = names.index("first and last")
    assert t.ora["cell"][i, :2].tolist() == [0, grid * grid - 1] and t.ora["n"][i] == 2
    i = names.index("two in one stride")
    assert t.ora["n"][i] == 1 and t.ora["cell"][i, 0] == grid + 1, "the second tying cell lies inside the first one's square"
    i = names.index("all")
    assert t.ora["cell"][i, :t.ora["n"][i]].tolist() == pu.flat_expected(grid, 2)
    m = pu.at_min_resp(grid, C, 0.5)
    assert m.ora["n"].tolist() == [2, 2] and np.all(m.ora["resp"][:, 1] == np.float32(0.5))
    assert pu.at_min_resp(grid, C, pu.THR_ABOVE_HALF).ora["n"].tolist() == [1, 1]
    nf = pu.nonfinite(grid, C)
    k = nf.names.index("all nan")
    assert nf.ora["n"][k] == 1 and nf.ora["cell"][k, 0] == 0 and np.isnan(nf.ora["score"][k, 0])
    assert nf.ora["fbox"][k, 0].tolist() == [0.0, 0.0, 10.0, 10.0]
    k = nf.names.index("all -inf")
    assert nf.ora["n"][k] == 1 and nf.ora["cell"][k, 0] == 0 and nf.ora["score"][k, 0] == 0.0


def test_prefixes_are_the_lists_of_smaller_k():
    grid, C = 8, 64
    p = pu.planted(grid, C, 1)
    st = p.states
    for K in (1, 3):
        o = pu.iterate_oracle(p.logits, p.hann, grid, st["geo"], st["frame_w"], st["frame_h"], K, 1, p.min_resp)
        pre = p.prefix(K)
        assert np.array_equal(o["n"], pre["n"]) and np.array_equal(o["cell"], pre["cell"][:, :K])
