"""
CPU side of tests/test_gpu_fp64_weighted.py and tests/test_gpu_sum_order.py: the conditions on their inputs
(tests/fp64_cases.py), checked with the oracle alone, so that no GPU assertion can pass vacuously.

* every decoding case: the oracle decodes at least 20 % and leaves open at least 20 % of the 37 codewords and reports three
  distinct iteration counts -- the syndrome answers both ways and rows latch at different iterations inside one tile;
* every weighted case: the tables are not float32 values, replacing alpha by ones changes the posterior of at least half of
  the codewords, and the float32 oracle's posterior differs from the float64 one on every codeword -- a kernel that skips
  alpha or narrows an operand cannot equal the expectation;
* both sum-order graphs: exactly the listed degrees, outside the resident engine, and at T = 1 the posterior of every
  variable of degree >= 7 differs between the numpy and the torch order on some codeword while no bit does -- only the
  value comparison of the posterior can see the order.
"""
import numpy as np
import pytest

import fp64_cases as fc

ids = fc.case_id


@pytest.mark.parametrize("case", fc.DECODE_CASES, ids=ids)
def test_oracle_decodes_some_codewords_and_not_others(case, oracle_mod):
    e = fc.expected(oracle_mod, case)
    assert e.success.shape == (fc.B,)
    ok = int(e.success.sum())
    assert ok >= 0.2 * fc.B and fc.B - ok >= 0.2 * fc.B, f"{ok} of {fc.B} decoded"
    assert len(set(e.iterations.tolist())) >= 3, sorted(set(e.iterations.tolist()))
    assert np.isfinite(e.posterior).all()
    fixed = fc.expected(oracle_mod, case, early_stop=False)
    assert (fixed.iterations == fc.T_of(case.code)).all()


@pytest.mark.parametrize("case", fc.TILE_CASES, ids=ids)
def test_tile_edge_batches_hold_latched_and_open_rows(case, oracle_mod):
    """from one full tile on, every batch of the tile-edge list mixes rows that stop with rows that stay open"""
    assert fc.TILE_BATCHES == (1, 64, 65, 128, 129, 130)
    for batch in fc.TILE_BATCHES:
        e = fc.expected(oracle_mod, case, batch=batch)
        assert e.bits.shape == (batch, 96)
        if batch >= 64:
            ok = int(e.success.sum())
            assert ok >= 0.2 * batch and batch - ok >= 0.2 * batch, (batch, ok)
            assert len(set(e.iterations.tolist())) >= 3
    # the codewords of the batches past a tile edge (row 64 of 65, rows 128 and 129 of 130) differ from row 0
    assert not np.array_equal(fc.llrs("small", 65)[64], fc.llrs("small", 65)[0])


def test_capped_decodes_cut_rows_at_every_cap(oracle_mod):
    """the caps 1 and 2 leave rows open that the full decode stops, 2 and T - 1 stop some rows and not others"""
    case = fc.CAP_CASE
    assert fc.caps(case) == (1, 2, 9)
    full = fc.expected(oracle_mod, case)
    for cap in fc.caps(case):
        e = fc.expected(oracle_mod, case, cap=cap)
        assert e.iterations.max() == cap
        if cap <= 2:
            assert int(e.success.sum()) < int(full.success.sum())
        if cap > 1:
            assert e.success.any() and not e.success.all()
        fixed = fc.expected(oracle_mod, case, early_stop=False, cap=cap)
        assert (fixed.iterations == cap).all()
    # the posterior of a capped fixed decode is that iteration's: it differs from the next iteration's on every row
    last = fc.expected(oracle_mod, case, early_stop=False).posterior
    a, b, c = (fc.expected(oracle_mod, case, early_stop=False, cap=c).posterior for c in fc.caps(case))
    assert (a != b).any(axis=1).all() and (c != last).any(axis=1).all()


@pytest.mark.parametrize("case", fc.WEIGHTED, ids=ids)
def test_tables_are_double_and_every_table_matters(case, oracle_mod):
    t = fc.tables(oracle_mod, case)
    T = fc.T_of(case.code)
    lo_hi = {"beta": fc.RANGES[case.form][0], "alpha": fc.RANGES[case.form][1], "oms_alpha": (0.0, 0.3)}
    for name in ("beta", "alpha", "oms_alpha"):
        tab = getattr(t, name)
        if tab is None:
            assert case.form == "nms" and name == "oms_alpha"
            continue
        assert tab.dtype == np.float64 and tab.shape[0] == T
        assert (tab.astype(np.float32).astype(np.float64) != tab).all(), f"{name} holds float32 values"
        assert (tab >= lo_hi[name][0]).all() and (tab <= lo_hi[name][1]).all()
        assert len(np.unique(tab)) == tab.size                          # every row and slot its own value
    assert (t.alpha != 1.0).all()
    # slot structure of the sharing type: what decides between the resident and the streaming engine
    per_check = all(len(set(t.beta_slot[a:b].tolist())) <= 1 for a, b in
                    zip(fc.load_code(case.code).tanner_graph().check_ptr[:-1], fc.load_code(case.code).tanner_graph().check_ptr[1:]))
    assert per_check == (case.wtype != 1)
    assert (t.beta.shape[1] > 1) == (case.wtype in (1, 2, 3)) and (t.alpha.shape[1] > 1) == (case.wtype in (2, 4))
    if t.beta.shape[1] > 1:
        assert set(t.beta_slot.tolist()) == set(range(t.beta.shape[1]))
    if t.alpha.shape[1] > 1:
        assert set(t.alpha_slot.tolist()) == set(range(t.alpha.shape[1]))
    if case.form == "oms":
        assert np.array_equal(t.oms_alpha_slot, t.beta_slot) and t.oms_alpha.shape == t.beta.shape

    og = fc.oracle_graph(oracle_mod, fc.load_code(case.code).tanner_graph())
    llr = fc.llrs(case.code)
    want = fc.expected(oracle_mod, case)
    # alpha: replaced by ones, the posterior of at least half of the codewords changes
    ones = fc.oracle_decode(oracle_mod, og, llr, case.form, fc.unit_alpha(t), T)
    rows = int((ones[1] != want.posterior).any(axis=1).sum())
    assert rows >= fc.B / 2, f"alpha changes {rows} of {fc.B} codewords"
    # the other draw of the weight-update test changes them too
    if case in fc.SET_WEIGHTS_CASES:
        other = fc.expected(oracle_mod, case, variant=1)
        assert (other.posterior != want.posterior).any(axis=1).sum() >= fc.B / 2
        unit = fc.expected(oracle_mod, case, unit=True)
        assert np.array_equal(unit.posterior, ones[1])
    # float: the same decode in float32 differs on every codeword
    f32 = fc.oracle_decode(oracle_mod, og, llr.astype(np.float32), case.form, t, T)
    assert f32[1].dtype == np.float32
    assert (f32[1].astype(np.float64) != want.posterior).any(axis=1).all()


@pytest.mark.parametrize("case", fc.BASIC, ids=ids)
def test_basic_case_is_the_decoder_classes_arithmetic(case, oracle_mod):
    og = fc.oracle_graph(oracle_mod, fc.load_code(case.code).tanner_graph())
    for early in (True, False):
        e = fc.expected(oracle_mod, case, early_stop=early)
        ob, op, oi, os_ = oracle_mod.basic_minsum(og, fc.llrs(case.code), 0.7, fc.T_of(case.code), early_stop=early)
        assert np.array_equal(e.bits, ob) and np.array_equal(e.posterior, op) and np.array_equal(e.iterations, oi)
        assert np.array_equal(e.success, os_)


# ---- sum-order graphs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.SUM_GRAPHS))
def test_sum_graphs_have_exactly_the_listed_degrees(name):
    dtype, m, _, degrees = fc.SUM_GRAPHS[name]
    g = fc.sum_graph(name)
    assert (g.m, g.n) == (m, len(degrees) + fc.FILLER) and fc.FILLER == 40
    assert g.dv[:len(degrees)].tolist() == list(degrees) and (g.dv[len(degrees):] == 3).all()
    assert len(set(degrees)) == len(degrees)
    assert g.dc.min() >= 1
    # the engine's limits are the largest degrees; dv > 8 keeps the graph off the resident, gather and pair forms
    # (choose_resident_plan and decoder_create_impl test max_dv <= 8 first)
    assert g.max_dv == (128 if dtype is fc.F64 else 575) == m
    assert g.max_dv > 8
    # both sides of every block edge, as operand counts N = dv (posterior) and N = dv - 1 (leave-one-out)
    counts = set(degrees) | {d - 1 for d in degrees}
    edges = (8, 16, 24, 32, 64) if dtype is fc.F64 else (8, 32, 40, 64, 256)
    for e in edges:
        assert {e - 1, e, e + 1} <= counts, e
    assert ({119, 120, 127, 128} if dtype is fc.F64 else {511, 512, 574, 575}) <= counts
    assert fc.refused_graph(129).max_dv == 129 and fc.refused_graph(576).max_dv == 576


def test_sum_graph_lists_are_the_documented_ones():
    assert fc.SUM_GRAPHS["f64"][3] == (1, 2, 7, 8, 9, 10, 15, 16, 17, 18, 24, 25, 32, 33, 64, 65, 120, 127, 128)
    assert fc.SUM_GRAPHS["f32"][3] == (7, 8, 9, 12, 13, 31, 32, 33, 39, 40, 41, 63, 64, 65, 255, 256, 257, 511, 512, 574, 575)
    assert fc.SUM_BATCH == 16 and fc.SUM_WIDE_BATCH == {"f64": 130, "f32": 300} and fc.SUM_T == (1, 3)
    assert fc.SUM_DECODERS == {"f64": ("nms1", "nms2", "oms2"), "f32": ("nms1", "nms2")}


@pytest.mark.parametrize("name,decoder", [(n, d) for n in sorted(fc.SUM_GRAPHS) for d in fc.SUM_DECODERS[n]])
def test_the_order_shows_in_every_high_degree_posterior_and_in_no_bit(name, decoder, oracle_mod):
    dtype, _, _, degrees = fc.SUM_GRAPHS[name]
    o = oracle_mod
    own, other = (o.SUM_NUMPY, o.SUM_TORCH) if dtype is fc.F64 else (o.SUM_TORCH, o.SUM_NUMPY)
    t = fc.sum_tables(oracle_mod, name, decoder, 1)
    assert t.beta.shape[1] == t.alpha.shape[1] == 1 if decoder.endswith("1") else t.beta.shape[1] > 8 and t.alpha.shape[1] > 8
    assert (t.alpha != 1.0).all() and (t.beta != 1.0).all()
    a = fc.sum_expected(oracle_mod, name, decoder, 1)
    b = fc.sum_expected(oracle_mod, name, decoder, 1, sum_order=other)
    assert a.posterior.dtype == dtype and a.posterior.shape == (fc.SUM_BATCH, len(degrees) + fc.FILLER)
    assert np.isfinite(a.posterior).all()
    assert np.array_equal(a.posterior, fc.sum_expected(oracle_mod, name, decoder, 1, sum_order=own).posterior)
    assert np.array_equal(a.bits, b.bits)
    differ = (a.posterior != b.posterior).any(axis=0)
    for j, d in enumerate(degrees):
        if d >= 7:
            assert differ[j], f"degree {d}: both orders give the same posterior on all {fc.SUM_BATCH} codewords"
    assert fc.differing_degrees(name, a.posterior, b.posterior) == sorted(d for d in degrees if d >= 7)
    # how far apart the orders are: the room a relaxed comparison would have to stay below
    rel = np.abs(a.posterior.astype(np.float64) - b.posterior) / np.maximum(1.0, np.abs(b.posterior))
    assert rel.max() < (1e-13 if dtype is fc.F64 else 1e-4)
    # T = 3 and the wide batches are inputs of the same kind: finite, fixed T
    for T, batch in ((3, fc.SUM_BATCH), (1, fc.SUM_WIDE_BATCH[name])):
        e = fc.sum_expected(oracle_mod, name, decoder, T, batch=batch)
        assert np.isfinite(e.posterior).all() and (e.iterations == T).all() and e.posterior.shape[0] == batch
