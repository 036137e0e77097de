"""
Host side (no GPU) of tests/test_gpu_quantiser_widths.py: conditions its inputs must meet on the CPU oracle alone, so that an
exact comparison with the oracle says something about the widths under test.

For every flooding case (the classes at bc 2, 6, 7, 8; engines built directly at 1, 9, 62, 63, 127 and 128 levels):
  * the decoded share of the batch lies in [0.1, 0.9]: early stop latches some codewords and runs others to T;
  * both signs of the top level L - 1 occur among the codes of the last executed iteration -- the saturated code, at L = 128
    the byte 255, is compared and not merely possible;
  * at least 95 % of the 2L code values occur there.
The layered cases have no code trace in their references; their decoded share is held to the same range, and for bc = 8 the
restatement of the weighted paper schedule must hold a code with level 127 and a negative sign when a decode ends.
"""
import numpy as np
import pytest

import quantiser_width_cases as qw


@pytest.mark.parametrize("case", qw.flood_cases() + qw.level_cases(), ids=qw.case_id)
def test_inputs_decode_in_part_and_reach_every_code(case, oracle_mod):
    L = qw.n_levels(case)
    for early in (True, False):
        want = qw.expected(oracle_mod, case, early)
        share, seen, neg_top, pos_top = qw.figures(case, want)
        print(f"{qw.case_id(case)} early_stop={early} at {qw.snr_of(case)} dB: decoded {share:.2f}, {seen} of {2 * L} code "
              f"values, top level {pos_top} times positive and {neg_top} times negative")
    want = qw.expected(oracle_mod, case, True)
    share, seen, neg_top, pos_top = qw.figures(case, want)
    assert 0.1 <= share <= 0.9
    assert neg_top > 0 and pos_top > 0
    assert seen >= 0.95 * 2 * L
    assert len(np.unique(want[2])) >= 2                       # early stop was exercised


def test_case_list_covers_the_widths_and_the_gates():
    flood, level = qw.flood_cases(), qw.level_cases()
    assert len(set(flood)) == len(flood) and len(set(level)) == len(level)
    small = [c for c in flood if c.code == "small"]
    assert {(c.dec, c.bc, c.chunk) for c in small} == {(d, bc, ch) for d in ("rcq", "w1", "w2") for bc in (2, 6, 7, 8) for ch in (300, 40)}
    assert all(c.chunk <= 64 or c.chunk == c.B for c in flood + level)
    assert {(c.bc, c.code) for c in flood if c.code == "odd"} == {(6, "odd"), (8, "odd")}
    assert {c.L for c in level} == {1, 9, 62, 63, 127, 128} and {c.tau0 for c in level if c.L == 1} == {0.0, 1.5}
    # the code-pair gate as the header states it: 32 levels through the classes, 62 directly; 63, 64, 128 and per-edge beta refused
    assert qw.pair_admitted(qw.Flood("w2", 6, 40, "small", 40)) and qw.pair_admitted(qw.Flood("rcq", 2, 40, "small", 40))
    assert not qw.pair_admitted(qw.Flood("w2", 7, 40, "small", 40)) and not qw.pair_admitted(qw.Flood("w1", 6, 40, "small", 40))
    assert qw.pair_admitted(qw.Level(62, 0.0, 40, 40)) and not qw.pair_admitted(qw.Level(63, 0.0, 40, 40))


def test_special_rows_and_channel_formula():
    x = qw.llrs(640, 40, 96, (1.0, 4.0))
    assert np.array_equal(x[0], np.round(x[0])) and np.all(x[1, ::3] == 0.0)
    assert np.all(np.isposinf(x[2, ::5])) and np.all(np.isneginf(x[3, 1::4]))
    rng = np.random.default_rng(640)
    z = [rng.standard_normal(96) for _ in range(6)]
    for r in (4, 5):
        s2 = 10.0 ** (-(1.0, 4.0)[r % 2] / 10.0)
        np.testing.assert_array_equal(x[r], (2.0 * (1.0 + np.sqrt(s2) * z[r]) / s2).astype(np.float32))


def test_per_check_beta_tables_have_a_negative_and_a_zero_slot(oracle_mod):
    for c in (qw.Flood("w2", 8, 300, "small", 300), qw.Flood("w1", 8, 320, "small", 40), qw.Flood("w2", 6, 300, "odd", 300)):
        _, wkw, _ = qw.build_flood(c)
        vals = list(wkw["beta"].values())
        assert min(vals) < 0 and 0.0 in vals
    _, _, kw = qw.level_tables(oracle_mod, qw.Level(62, 0.0, 320, 40))
    assert kw["beta"].min() < 0 and (kw["beta"] == 0).any() and kw["thresholds"].shape == (3, 62)
    code, _ = qw.make_code(qw.Level(62, 0.0, 320, 40))
    cp = code.tanner_graph().check_ptr
    assert all(len(set(kw["beta_slot"][cp[i]:cp[i + 1]].tolist())) <= 1 for i in range(len(cp) - 1))    # one beta per check


@pytest.mark.parametrize("case", qw.layered_cases(), ids=qw.case_id)
def test_layered_inputs_decode_in_part(case, oracle_mod):
    llr, bits, post, iters, succ, fixed, neg_top = qw.layered_expected(oracle_mod, case)
    print(f"{qw.case_id(case)}: decoded {succ.mean():.2f}, negative top-level code held: {neg_top}")
    assert 0.1 <= succ.mean() <= 0.9
    assert len(np.unique(iters)) >= 2
    if case.dec == "wpaper" and case.bc == 8:
        assert neg_top
