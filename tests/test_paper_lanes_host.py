"""
The cases of tests/paper_lane_cases.py on the CPU (no GPU): they are what they claim (lane width, degree-1 and degree-0
checks, level counts, the class the codewords-per-wave rule puts each geometry in), the two yardsticks of
tests/test_gpu_paper_lanes.py -- oracle.rcq_layered(paper=True) and the restatement of tests/test_gpu_layered_weighted.py --
agree at unit beta on every one of them (neither had run on a graph with a degree-0 check under this schedule), and no case
is degenerate: under each early-stop reference some rows stop before T, some never do, they stop at different iterations,
and a wave of the LDS kernel holds a stopped codeword beside an open one.
"""
import numpy as np
import pytest

import paper_lane_cases as pc
from test_gpu_layered_weighted import restate

NAMES = [c.name for c in pc.CASES]


def test_case_list():
    kinds = [c.kind for c in pc.CASES]
    assert (kinds.count("lane"), kinds.count("quant"), kinds.count("geom")) == (7, 8, 8)
    assert [c.lw for c in pc.CASES if c.kind == "lane"] == [1, 2, 4, 8, 16, 32, 64]
    assert sorted({c.lw for c in pc.CASES if c.kind == "geom"}) == [1, 2, 4, 8, 16, 32, 64]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_what_it_claims(name):
    c, code = pc.BY_NAME[name], pc.code_of(name)
    g = code.tanner_graph()
    dc = np.diff(g.check_ptr)
    assert pc.lane_width(int(dc.max())) == c.lw
    if c.kind == "geom":
        n, m, dmax = c.code
        assert (g.n, g.m) == (n, m) and dc.max() == dmax and dc.min() >= 1
    else:
        assert dc.max() == c.lw                                  # the widest check fills the row
        assert (dc == 1).any() and (dc == 0).any() and g.n % 2 == 1 and g.m % 2 == 1
    plain, weighted, beta_e = pc.decoders(name)
    for dec in (plain, weighted):
        assert dec.max_iterations == pc.T and dec.layered == "paper"
        assert [len(q.thresholds) for q in dec.quantizers] == [pc.n_levels(c)] * 3
    assert pc.n_levels(c) == {3: 4, 4: 8, 5: 16}[c.bc]
    zero0 = [q.thresholds[0] == 0.0 for q in plain.quantizers]
    assert zero0 == ([False, True, False] if name.endswith("gamma0") else [True] * 3)
    # randomise_betas: zeros and negatives among the weights the code's edges use, and no two iterations alike
    assert beta_e.shape == (pc.T, g.E) and (beta_e == 0).any() and (beta_e < 0).any() and (np.abs(beta_e) < 1).all()
    assert all((beta_e[t] != beta_e[0]).any() for t in range(1, pc.T))
    llr = pc.inputs(name)
    assert llr.shape == (pc.POOL, g.n) and llr.dtype == np.float32
    assert (llr[0, :3] == 0).all() and (llr[1] == np.round(llr[1])).all() and (llr[2] >= 4).all()


# the table of the rule as written: (n, m, max dc) -> (codewords per wave, workgroups per CU)
TABLE = {(500, 250, 6): (8, 5), (100, 25, 12): (4, 48), (100, 25, 24): (2, 63), (1300, 325, 3): (5, 5),
         (500, 250, 2): (13, 5), (1100, 275, 1): (7, 5), (300, 75, 12): (1, 67), (1200, 600, 40): (0, 0)}


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.kind == "geom"])
def test_geometry_class_under_the_restated_rule(name):
    c = pc.BY_NAME[name]
    n, m, _ = c.code
    cw, per_cu = pc.plan_of(n, m, c.lw)
    assert (cw, per_cu) == TABLE[c.code]
    assert pc.class_of(cw, c.lw) == c.klass
    if c.klass == pc.STREAM:                                     # one codeword fits, three workgroups per CU do
        assert pc.row_bytes(n, m, c.lw) <= pc.LDS_BYTES and pc.LDS_BYTES // pc.row_bytes(n, m, c.lw) == 3
    if c.klass == pc.SINGLE:
        assert 64 // c.lw == 4                                   # three shadow groups


def test_classes_of_a_count():
    assert pc.class_of(8, 8) == pc.FULL and pc.class_of(1, 64) == pc.FULL and pc.class_of(64, 1) == pc.FULL
    assert pc.class_of(5, 4) == pc.NPOT and pc.class_of(13, 2) == pc.NPOT and pc.class_of(7, 1) == pc.NPOT
    assert pc.class_of(1, 16) == pc.SINGLE and pc.class_of(0, 64) == pc.STREAM
    assert pc.class_of(2, 8) is None and pc.class_of(4, 2) is None


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_oracle_at_unit_beta(name, oracle_mod):
    """bits, posteriors, iterations and success of the whole pool, bit for bit"""
    c, code = pc.BY_NAME[name], pc.code_of(name)
    ones = np.ones((pc.T, code.tanner_graph().E), dtype=np.float32)
    got = restate(code, pc.inputs(name), c.bc, c.qp, pc.T, ones)
    want = pc.reference(oracle_mod, name, weighted=False)
    for a, b, what in zip(got, want, ("bits", "posterior", "iterations", "success")):
        np.testing.assert_array_equal(a, b, err_msg=f"{name} {what}")


@pytest.mark.parametrize("name", [c.name for c in pc.CASES if c.kind == "quant"])
def test_quantiser_cases_hold_every_level(name):
    """the codes the edges hold when their codeword's decode ends (the ones a next iteration reads back): every level with a
    positive sign under both decoders -- each leaf of the kernel's select trees, and the table entries past the eight
    registers at sixteen levels -- and with a negative sign under the weighted one; with gamma = 0, level 0 under both signs
    (it reconstructs to +-C, not to 0) and the top level"""
    c, code = pc.BY_NAME[name], pc.code_of(name)
    L = pc.n_levels(c)
    for weighted in (False, True):
        beta_e = pc.decoders(name)[2] if weighted else np.ones((pc.T, code.tanner_graph().E), dtype=np.float32)
        held = restate(code, pc.inputs(name), c.bc, c.qp, pc.T, beta_e, want_messages=True)[4]
        held = held[held != 255]
        pos, neg = set(held[held < L].tolist()), set((held[held >= L] - L).tolist())
        if name.endswith("gamma0"):
            assert {0, L - 1} <= pos and {0, L - 1} <= neg, (name, weighted, pos, neg)
        else:
            assert pos == set(range(L)), (name, weighted, pos)
            assert not weighted or neg == set(range(L)), (name, neg)


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("name", NAMES)
def test_no_case_is_degenerate(name, weighted, oracle_mod):
    c, g = pc.BY_NAME[name], pc.code_of(name).tanner_graph()
    cw, _ = pc.plan_of(g.n, g.m, c.lw)
    _, _, iters, succ = pc.reference(oracle_mod, name, weighted)
    if not weighted:                                             # the |llr| + 4 row stops at once (a negative beta may push it off)
        assert iters[2] == 1 and succ[2]
    assert (iters[~succ] == pc.T).all()
    assert pc.degeneracy(name, iters, succ, cw or None) == [], (name, c.snr, iters.tolist())


def test_static_codes_are_the_lane_width_one_codes():
    assert [n for n in NAMES if pc.static_decode(n)] == ["lw1", "g1100x275-dc1"]
    for name in ("lw1", "g1100x275-dc1"):
        assert (np.abs(pc.decoders(name)[2]) < 1).all()
