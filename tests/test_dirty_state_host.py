"""
What tests/test_gpu_dirty_state.py relies on, established on the CPU from the restatements alone (tests/dirty_state_cases.py):
every batch of 64 rows or more is decoded in part -- between 20 % and 80 % of its rows within T --, so every tile holds rows that
latch early beside rows that stay open; one row stops at iteration 1; under the cap of 2 some rows have stopped and some have not.
"""
import numpy as np
import pytest

import dirty_state_cases as ds


@pytest.mark.parametrize("case", ds.DECODE_CASES, ids=ds.case_id)
def test_the_oracle_decodes_part_of_every_batch(case, oracle_mod):
    want = ds.expected(oracle_mod, case)
    T = ds.T_OF[case.code]
    assert want.rows is None and want.bits.shape == (case.B, ds.load_code(case.code).n)
    assert np.all((want.iterations >= 1) & (want.iterations <= T)) and np.all(want.iterations[~want.success] == T)
    if case.B > 3:
        assert want.success[3] and want.iterations[3] == 1                 # the strongly sent codeword
    if case.B >= 64:
        frac = want.success.mean()
        assert 0.2 <= frac <= 0.8, f"the oracle decodes {frac:.0%} of the rows"
        fam = ds.FAMILIES[case.family]
        W = 64 if fam.kind.startswith("lay") or case.B <= 64 else 128 if fam.dtype is ds.F64 else 256
        for t0 in range(0, case.B, W):                                      # every tile that is not a lone row or two: both kinds
            tile = want.success[t0:t0 + W]
            assert len(tile) <= 2 or (tile.any() and not tile.all()), (t0, tile)
        capped = ds.expected(oracle_mod, case, True, ds.CAP)
        stopped = capped.success if capped.rows is None else capped.rows
        assert stopped.any() and not stopped.all()                          # the cap of 2 cuts some rows off
        assert np.all(capped.iterations[~stopped] == ds.CAP)


def test_the_case_list_covers_what_it_claims():
    fams = ds.FAMILIES
    assert {f.mode for f in fams.values() if f.kind == "rcq"} == {"pair", "gather", "sweeps"}
    assert {f.where for f in fams.values() if f.kind.startswith("lay")} == {"layered_rcq<ref>", "layered_rcq<paper>", "layered_minsum"}
    assert {c.B for c in ds.DECODE_CASES if fams[c.family].dtype is ds.F32} == {1, 64, 65, 257}
    assert {c.B for c in ds.DECODE_CASES if fams[c.family].dtype is ds.F64} == {129}
    assert {c.family for c in ds.DECODE_CASES if c.code == "wide"} == {"basic32", "rcq-sweeps"}
    small, ira = ds.load_code("small").tanner_graph(), ds.load_code("ira").tanner_graph()
    assert small.m == 48 and ira.m == 486 and (ira.n * 4) % 16 == 8        # one-block syndrome / chunked latch; 8-byte rows
    assert ds.load_code("wide").tanner_graph().dc.max() == 129
    x = ds.saturated_llrs("small", ds.F32)
    assert x.shape == (300, 96) and np.all(np.abs(x) == np.float32(1e30)) and 0.4 < (x < 0).mean() < 0.6
