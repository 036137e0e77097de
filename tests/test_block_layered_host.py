"""
Host side of the block-parallel layered decode (CPU): layers on the graph (``TannerGraph.layer_ptr`` / ``with_layers``,
``tanner_graph.disjoint_runs``), quasi-cyclic codes (``codes.quasi_cyclic`` / ``generate_qc_code``, the committed
``qc_1944_972``), the layer order of any code (``codes.layered_order``), the npz round trip, the input sets of
tests/block_layered_cases.py, the C header, and the legality claim the GPU kernel rests on: the checks of a layer share
no variable, so the restatement of the graph whose rows are REVERSED inside every layer returns the same bits,
posteriors, iterations and success as the restatement of the graph itself.
"""
import io
import os
import re

import numpy as np
import pytest

import block_layered_cases as bc
from conftest import ROOT


# ---- quasi_cyclic --------------------------------------------------------------------------------------------------------------
def test_quasi_cyclic_equals_a_dense_construction():
    import codes
    rng = np.random.default_rng(3)
    for mb, nb, Z in ((2, 3, 1), (3, 5, 4), (2, 4, 7), (1, 2, 9)):
        S = rng.integers(-1, Z + 2, size=(mb, nb))            # -1: zero block; values >= Z wrap
        S[S == Z + 1] = -3                                    # every value < 0 is the zero block
        H = np.zeros((mb * Z, nb * Z), dtype=np.int8)
        for r in range(mb):
            for c in range(nb):
                if S[r, c] >= 0:
                    for z in range(Z):
                        H[r * Z + z, c * Z + (z + S[r, c]) % Z] = 1
        g = codes.quasi_cyclic(S, Z)
        assert (g.n, g.m) == (nb * Z, mb * Z)
        np.testing.assert_array_equal(g.to_dense(), H)
        np.testing.assert_array_equal(g.layer_ptr, np.arange(mb + 1) * Z)
        assert g.layer_ptr.dtype == np.int32
    with pytest.raises(ValueError):
        codes.quasi_cyclic(np.zeros((2, 2)), 4)               # not an integer array
    with pytest.raises(ValueError):
        codes.quasi_cyclic(np.zeros((2, 2), dtype=np.int64), 0)


# ---- with_layers -----------------------------------------------------------------------------------------------------------------
def test_with_layers_validates_pointer_and_disjointness():
    import codes
    g = codes.load_graph("small_96_48")
    assert g.layer_ptr is None and g.n_layers == 0
    ok = g.with_layers(np.arange(g.m + 1))
    assert ok is not g and g.layer_ptr is None and ok.n_layers == g.m and ok.layer_ptr.dtype == np.int32
    np.testing.assert_array_equal(ok.var_idx, g.var_idx)
    for bad in ([1, g.m], [0, g.m - 1], [0, 5, 5, g.m], [0, 7, 3, g.m], [[0, g.m]], np.array([0.0, g.m])):
        with pytest.raises(ValueError, match="layer_ptr"):
            g.with_layers(bad)
    # checks 0 and 1 share a staircase variable: the first offending layer and the variable are named
    shared = sorted(set(g.var_idx[g.check_ptr[0]:g.check_ptr[1]]) & set(g.var_idx[g.check_ptr[1]:g.check_ptr[2]]))
    assert shared
    with pytest.raises(ValueError, match=rf"layer 0 .*variable {shared[0]}\b"):
        g.with_layers([0, 2] + list(range(3, g.m + 1)))
    with pytest.raises(ValueError, match="layer 1 "):
        g.with_layers([0, 1, 3] + list(range(4, g.m + 1)))


def test_a_code_from_a_graph_carries_its_layers_and_a_dense_one_has_none():
    from ldpc_decoder import LDPCCode
    g = bc.graph("qc_3_6_5")
    code = LDPCCode.from_graph(g, k=g.n - g.m)
    assert code.tanner_graph() is g and code.tanner_graph().n_layers == 3
    assert LDPCCode(n=g.n, k=g.n - g.m, H=g.to_dense()).tanner_graph().layer_ptr is None


# ---- disjoint_runs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,runs", [("small_96_48", 48), ("ira_1998_1512", 486), ("dvbs2_like_16200_7200", 9000)])
def test_disjoint_runs_on_the_committed_codes(name, runs):
    """the IRA staircase makes every check collide with its neighbour: every run has length 1"""
    import codes
    import tanner_graph
    g = codes.load_graph(name)
    lp = tanner_graph.disjoint_runs(g)
    assert lp.dtype == np.int32 and len(lp) - 1 == runs
    np.testing.assert_array_equal(lp, tanner_graph.disjoint_runs(g))
    g.with_layers(lp)                                             # valid by construction


def test_disjoint_runs_are_maximal():
    import tanner_graph
    for name in ("qc_4_8_65", "ragged", "ira_lo"):
        g = bc.graph(name)
        lp = tanner_graph.disjoint_runs(g)
        g.with_layers(lp)
        for l in range(1, len(lp) - 1):                           # the first check of a run collides with the run before it
            prev = set(g.var_idx[g.check_ptr[lp[l - 1]]:g.check_ptr[lp[l]]].tolist())
            assert prev & set(g.var_idx[g.check_ptr[lp[l]]:g.check_ptr[lp[l] + 1]].tolist()), (name, l)
    assert len(tanner_graph.disjoint_runs(bc.graph("qc_4_8_65"))) - 1 == 4


# ---- layered_order ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layers,smallest,largest", [("small_96_48", 10, 2, 7), ("ira_1998_1512", 20, 1, 40)])
def test_layered_order(name, layers, smallest, largest):
    import codes
    g = codes.load_graph(name)
    g2, perm = codes.layered_order(g)
    again, perm_again = codes.layered_order(g)
    np.testing.assert_array_equal(perm, perm_again)
    np.testing.assert_array_equal(g2.var_idx, again.var_idx)
    np.testing.assert_array_equal(g2.layer_ptr, again.layer_ptr)
    sizes = np.diff(g2.layer_ptr)
    assert (g2.n_layers, sizes.min(), sizes.max()) == (layers, smallest, largest)
    np.testing.assert_array_equal(np.sort(perm), np.arange(g.m))
    for i in range(g.m):                                          # row i of graph2 is row perm[i] of graph
        np.testing.assert_array_equal(g2.var_idx[g2.check_ptr[i]:g2.check_ptr[i + 1]],
                                      g.var_idx[g.check_ptr[perm[i]]:g.check_ptr[perm[i] + 1]])
    for l in range(g2.n_layers):                                  # ascending inside a layer, disjoint (with_layers checked it too)
        rows = perm[g2.layer_ptr[l]:g2.layer_ptr[l + 1]]
        assert (np.diff(rows) > 0).all()
        vs = g2.var_idx[g2.check_ptr[g2.layer_ptr[l]]:g2.check_ptr[g2.layer_ptr[l + 1]]]
        assert len(set(vs.tolist())) == len(vs)
    for cap in (1, 3, 16):
        g3, perm3 = codes.layered_order(g, max_layer=cap)
        assert np.diff(g3.layer_ptr).max() <= cap and np.array_equal(np.sort(perm3), np.arange(g.m))
    assert codes.layered_order(g, max_layer=1)[0].n_layers == g.m
    with pytest.raises(ValueError):
        codes.layered_order(g, max_layer=0)
    # the same code: codewords of the original's encoder have zero syndrome on the reordered graph
    enc = codes.Encoder.from_graph(g)
    cw = enc.encode(np.random.default_rng(5).integers(0, 2, size=(7, enc.k)))
    assert cw.any() and not g.syndrome(cw).any() and not g2.syndrome(cw).any()


# ---- npz round trip --------------------------------------------------------------------------------------------------------------
def test_npz_round_trip_with_and_without_layers(tmp_path):
    import codes
    g = bc.graph("ragged")
    p = str(tmp_path / "layered.npz")
    codes.save_graph(p, g)
    back = codes.load_graph(p)
    np.testing.assert_array_equal(back.layer_ptr, g.layer_ptr)
    np.testing.assert_array_equal(back.check_ptr, g.check_ptr)
    np.testing.assert_array_equal(back.var_idx, g.var_idx)
    # without layers: byte for byte what save_graph wrote before layers existed
    plain = codes.load_graph("small_96_48")
    q = str(tmp_path / "plain.npz")
    codes.save_graph(q, plain)
    want = io.BytesIO()
    np.savez_compressed(want, n=np.int32(plain.n), m=np.int32(plain.m), check_ptr=plain.check_ptr,
                        var_idx=plain.var_idx.astype(np.uint16))
    with open(q, "rb") as f:
        assert f.read() == want.getvalue()
    with np.load(q) as z:
        assert "layer_ptr" not in z.files
    assert codes.load_graph(q).layer_ptr is None


# ---- the committed QC code -------------------------------------------------------------------------------------------------------
def gf2_rank(H):
    A = np.array(H, dtype=np.uint8)
    r = 0
    for c in range(A.shape[1]):
        hit = np.flatnonzero(A[r:, c])
        if hit.size == 0:
            continue
        p = r + int(hit[0])
        if p != r:
            A[[r, p]] = A[[p, r]]
        rows = np.flatnonzero(A[:, c])
        rows = rows[rows != r]
        A[rows] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def test_committed_qc_1944_972():
    """the named code is generated from its seed; its recorded edge list (tests/golden/qc_1944_972.npz, written by
    ``codes.save_graph``) pins the generator"""
    import codes
    g = codes.load_graph("qc_1944_972")
    assert codes.load_graph("qc_1944_972") is g                    # once per process: engines share the device copy
    assert "qc_1944_972" in codes.code_names()
    assert (g.n, g.m, g.n_layers) == (1944, 972, 12)
    np.testing.assert_array_equal(g.layer_ptr, np.arange(13) * 81)
    assert set(g.dc.tolist()) == {7, 8}
    regen = codes.load_graph(os.path.join(ROOT, "tests", "golden", "qc_1944_972.npz"))
    np.testing.assert_array_equal(regen.check_ptr, g.check_ptr)
    np.testing.assert_array_equal(regen.var_idx, g.var_idx)
    np.testing.assert_array_equal(regen.layer_ptr, g.layer_ptr)
    assert g.four_cycles() == 0
    assert gf2_rank(g.to_dense()) == 972
    # dual diagonal: parity block column i in block rows i and i + 1 at shift 0
    H = g.to_dense()
    for i in range(12):
        blk = H[:, (12 + i) * 81:(13 + i) * 81]
        rows = [r for r in range(12) if blk[r * 81:(r + 1) * 81].any()]
        assert rows == ([i, i + 1] if i < 11 else [11])
        for r in rows:
            np.testing.assert_array_equal(blk[r * 81:(r + 1) * 81], np.eye(81, dtype=np.int8))


def test_generate_qc_code_is_seeded_and_checks_its_arguments():
    import codes
    a, b = codes.generate_qc_code(3, 6, 5, {2: 2, 3: 1}, 1), codes.generate_qc_code(3, 6, 5, {2: 2, 3: 1}, 1)
    np.testing.assert_array_equal(a.var_idx, b.var_idx)
    assert not np.array_equal(a.var_idx, codes.generate_qc_code(3, 6, 5, {2: 2, 3: 1}, 2).var_idx)
    for name in bc.QC_SHAPES:
        g = bc.graph(name)
        mb, nb, Z = bc.QC_SHAPES[name][:3]
        assert g.four_cycles() == 0 and gf2_rank(g.to_dense()) == g.m and (g.n, g.m, g.n_layers) == (nb * Z, mb * Z, mb)
    with pytest.raises(ValueError):
        codes.generate_qc_code(3, 6, 5, {2: 2}, 1)                # profile does not cover nb - mb columns
    with pytest.raises(ValueError):
        codes.generate_qc_code(3, 6, 5, {4: 3}, 1)                # degree above mb


# ---- the case graphs and their inputs -----------------------------------------------------------------------------------------
def test_case_graphs_are_what_the_cases_say():
    g = bc.graph("ragged")
    assert g.n % 2 == 1 and g.m % 2 == 1
    assert {0, 1, 33, bc.MAX_DEG} <= set(g.dc.tolist()) and g.dc.max() == bc.MAX_DEG
    sizes = np.diff(g.layer_ptr)
    assert sizes.min() == 1 and sizes.max() > 8
    r = bc.graph("runs_small")
    assert r.n_layers == r.m == 48
    assert [int(np.diff(bc.graph(n).layer_ptr).max()) for n in bc.QC_SHAPES] == [5, 64, 65, 130]
    assert bc.graph("ira_lo").n_layers == 20 and bc.graph("qc_1944").n_layers == 12
    assert bc.input_llr("ira_lo").shape == (128, 1998) and bc.input_llr("qc_1944").shape == (64, 1944)
    assert np.unique(bc.rcq_edge_betas(bc.make_rcq("unit_l4", "qc_3_6_5"), bc.T)).tolist() == [1.0]


@pytest.mark.parametrize("name", bc.GRAPHS)
def test_input_sets_leave_frozen_rows_beside_live_ones(name):
    """the restatement decodes between 20 % and 80 % of the rows and shows at least two distinct stop iterations"""
    llr = bc.input_llr(name)
    assert (llr[0, :3] == 0).all() and np.array_equal(llr[1], np.round(llr[1]))
    _, _, iters, succ = bc.reference_minsum(name, "basic")
    assert 0.2 <= succ.mean() <= 0.8, succ.mean()
    assert len(set(iters[succ].tolist())) >= 2, sorted(set(iters.tolist()))


# ---- the legality claim ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.GRAPHS)
def test_the_order_inside_a_layer_does_not_change_a_bit(name):
    big = name in ("ira_lo", "qc_1944")
    rows = 16 if big else None
    runs = [("ms", "basic"), ("rcq", "t2_l8")] if big else \
        [("ms", f) for f in bc.FAMILIES] + [("rcq", f) for f in ("t1_l4", "t2_l16", "t1_g0", "unit_l4")]
    g2, idx = bc.reversed_inside_layers(name)
    if name != "runs_small":
        assert not np.array_equal(idx, np.arange(len(idx)))            # it IS another walk
    for kind, form in runs:
        ref = bc.reference_minsum if kind == "ms" else bc.reference_rcq
        for es in (True, False):
            a = ref(name, form, early_stop=es, rows=rows)
            b = ref(name, form, early_stop=es, rows=rows, reversed_layers=True)
            for x, y, what in zip(a, b, ("bits", "posterior", "iterations", "success")):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} {form} es={es} {what}")


def test_a_reordering_across_layers_is_another_decoder():
    """layered_order gives the same code but a different layered decode (its docstring says so)"""
    import codes
    import layered_minsum_reference as ref
    g = codes.load_graph("small_96_48")
    g2, _ = codes.layered_order(g)
    llr = bc.input_llr("runs_small")
    beta = np.full((10, g.E), 0.7, dtype=np.float32)
    a, b = ref.restate(g, llr, 10, ref.NMS, beta), ref.restate(g2, llr, 10, ref.NMS, beta)
    assert not np.array_equal(a[1], b[1])


# ---- header and binding ------------------------------------------------------------------------------------------------------------
def test_header_and_binding_declare_the_new_functions_and_mode():
    import _native as nat
    with open(os.path.join(ROOT, "include", "ldpc_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define LDPC_HIP_ABI_VERSION 1\b", header)
    assert re.search(r"LDPC_MODE_BLOCK = 6\b", header) and nat.MODE_BLOCK == 6
    proto = re.sub(r"\s+", " ", header)
    assert ("int ldpc_graph_create_layered(ldpc_graph **out, int32_t n, int32_t m, int32_t n_edges, const int32_t *check_ptr, "
            "const int32_t *var_idx, int32_t n_layers, const int32_t *layer_ptr);") in proto
    assert "int ldpc_graph_layers(const ldpc_graph *g, int32_t *n_layers, int32_t *layer_ptr_out);" in proto
    for name in ("ldpc_graph_create_layered", "ldpc_graph_layers"):
        assert name in nat.PRODUCT_EXPORTS
    assert {"ldpc_layered_block.hip", "ldpc_layer_plan.h"} <= set(nat.SOURCES)
    if os.path.exists(nat.LIB_PATH):                                # where the library is built: it exports them
        lib = nat._dlopen(nat.LIB_PATH) if not nat.is_stale(nat.LIB_PATH) else None
        if lib is not None:
            for name in ("ldpc_graph_create_layered", "ldpc_graph_layers"):
                assert hasattr(lib, name)
            assert lib.ldpc_abi_version() == 1
