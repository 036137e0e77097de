"""
What tests/test_gpu_row_alignment.py relies on, established on the CPU from the restatements and the case list alone
(tests/row_alignment_cases.py): the three codes give the three residues of the row length; every batch of 64 rows or more is
decoded in part, over several stop iterations, in every tile; the placement list holds every placement the alignment rule
distinguishes, and the restated rule reaches every width of every family.  ldpc_debug_boundary_kernels rejects a NULL
decoder without touching a device.
"""
import numpy as np
import pytest

import row_alignment_cases as ra
from row_alignment_cases import ds


@pytest.mark.parametrize("family,code", ra.FAMILY_CODES)
def test_the_oracle_decodes_part_of_every_batch_over_several_iterations(family, code, oracle_mod):
    for case in ra.cases(family, code):
        want = ra.expected(oracle_mod, case)
        assert want.rows is None and want.bits.shape == (case.B, ds.load_code(code).n)
        assert np.all((want.iterations >= 1) & (want.iterations <= ra.T)) and np.all(want.iterations[~want.success] == ra.T)
        if case.B > 3:
            assert want.success[3] and want.iterations[3] == 1             # the strongly sent codeword
        if case.B < 64:
            continue
        frac = want.success.mean()
        stops = np.unique(want.iterations[want.success])
        print(f"{ds.case_id(case)}: the oracle decodes {frac:.0%}, stop iterations {stops.tolist()}")
        assert 0.2 <= frac <= 0.8, f"the oracle decodes {frac:.0%} of the rows"
        assert len(stops) >= 3, stops
        W = ra.tile_rows(family, case.B)
        for t0 in range(0, case.B, W):                                      # every tile of more than two rows: both kinds
            tile = want.success[t0:t0 + W]
            assert len(tile) <= 2 or (tile.any() and not tile.all()), (t0, tile)
        capped = ra.expected(oracle_mod, case, True, ds.CAP)
        assert capped.rows is None
        assert capped.success.any() and not capped.success.all()            # the cap of 2 cuts some rows off
        assert np.all(capped.iterations[~capped.success] == ds.CAP)


def test_the_codes_give_the_three_row_lengths():
    n = {c: ds.load_code(c).n for c in ra.CODES}
    assert n == {"small96": 96, "g134": 134, "g131": 131}
    assert [(4 * n[c]) % 16 for c in ra.CODES] == [0, 8, 12] and n[ra.ODD] % 2 == 1 and n[ra.ODD] % 64 == 3
    assert [(8 * n[c]) % 16 for c in ra.CODES] == [0, 0, 8]                 # fp64: only the odd code has 8-byte rows
    for c in ("g134", "g131"):
        code = ds.load_code(c)
        g = code.tanner_graph()
        H = np.asarray(code.H)
        assert (H.sum(axis=0) == 3).all() and H.sum(axis=1).max() - H.sum(axis=1).min() <= 1
        assert g.dv.max() <= 8 and g.dc.max() <= 32
        assert gf2_rank(H) == g.m                                           # k = n - m
    g = ds.load_code("small96").tanner_graph()
    assert g.dv.max() <= 8 and g.dc.max() <= 32


def gf2_rank(H):
    A = (np.array(H) % 2).astype(np.uint8)
    r = 0
    for c in range(A.shape[1]):
        piv = np.flatnonzero(A[r:, c])
        if not len(piv):
            continue
        A[[r, r + piv[0]]] = A[[r + piv[0], r]]
        rows = np.flatnonzero(A[:, c])
        rows = rows[rows != r]
        A[rows] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def test_the_placement_list_holds_every_named_placement():
    P = ra.Placement
    f32 = {(p.llr, p.posterior, p.bits) for p in ra.PLACEMENTS[ra.F32]}
    want = {(0, 0, 0), (4, 0, 0), (8, 0, 0), (12, 0, 0), (0, 4, 4), (0, 8, 8), (0, 12, 12), (0, 0, 4), (0, 4, 0), (0, 8, 4),
            (4, 12, 8), (0, None, 4), (0, 4, None), (0, None, None)}
    assert f32 == want and len(ra.PLACEMENTS[ra.F32]) == len(want)
    f64 = {(p.llr, p.posterior, p.bits) for p in ra.PLACEMENTS[ra.F64]}
    assert f64 == {(0, 0, 0), (8, 8, 4), (8, 8, 8), (8, 8, 12)}
    for dt, elem in ((ra.F32, 4), (ra.F64, 8)):
        names = [p.name for p in ra.PLACEMENTS[dt]]
        assert len(set(names)) == len(names) and ra.PLACEMENTS[dt][0] == P("aligned", 0, 0, 0)
        for p in ra.PLACEMENTS[dt]:                                         # every pointer keeps its element's alignment
            assert p.llr % elem == 0 and (p.posterior or 0) % elem == 0 and (p.bits or 0) % 4 == 0
            assert max(p.llr, p.posterior or 0, p.bits or 0) < ra.MAX_OFFSET
    assert set(ra.BATCHES[ra.F32]) == {1, 64, 65, 257} and set(ra.BATCHES[ra.F64]) == {1, 64, 129}
    assert ra.STOPS == ((True, None), (False, None), (True, 2))


@pytest.mark.parametrize("family", ra.FAMILIES)
def test_the_restated_rule_reaches_every_width_of_every_family(family):
    """the rule as tests/row_alignment_cases.py restates it; the GPU file asserts the launcher's own answer equals it"""
    seen = {ra.kernels(family, ds.load_code(c).n, B, pl)
            for c in ra.CODES for B in ra.BATCHES[ra.dtype_of(family)] for pl in ra.placements(family)}
    ins, outs = ra.reachable(family)
    assert {(k.vec, k.in_bytes) for k in seen} == ins
    assert {(k.vec, k.out_path, k.out_bytes) for k in seen} == outs
    fused = {(k.vec, k.in_bytes) for k in seen if k.fused_in}
    assert fused == ({(4, 16)} if family in ra.PAIR_Q4 else set())
    assert not any(k.vec == 4 and k.in_bytes == 16 and not k.fused_in for k in seen if family in ra.PAIR_Q4)


def test_boundary_kernels_hook_rejects_bad_arguments():
    import _native
    lib = _native.load()
    out = np.zeros(5, np.int32)
    assert "ldpc_debug_boundary_kernels" in _native.EXPORTS
    assert lib.ldpc_debug_boundary_kernels(None, 65, 0, 0, None, None, None, _native.ptr(out)) == -1     # LDPC_ERR_ARG
    assert lib.ldpc_debug_boundary_kernels(None, 65, 0, 1, None, None, None, None) == -1
    assert not out.any()
    # with a live decoder (NULL output, a decoder on a resident engine): tests/test_gpu_row_alignment.py
