"""
What tests/test_gpu_tile_geometry.py relies on, established on the CPU from the graphs, the restatements and the
arrangements alone (tests/tile_geometry_cases.py): the two generated graphs have the degrees, the size and the five blocks of
256 checks they were made for; every family's restatement decodes part of its pool, over several stop iterations, stops the
strongly sent rows at iteration 1 and never stops the rows made for that; every batch arrangement holds a tile that is done
after one iteration, a tile that never is, and a mixed one, at the ragged sizes the list names.  These are conditions on the
inputs, met by the restatements alone -- no engine result is part of them.  ldpc_debug_launch_geometry rejects bad arguments
without touching a device.
"""
import numpy as np
import pytest

import tile_geometry_cases as tg
from tile_geometry_cases import ds


def test_the_generated_graphs_have_the_degrees_they_were_made_for():
    g, hi = (ds.load_code(c).tanner_graph() for c in tg.GENERATED)
    assert (g.n, g.m, g.E) == (1400, 1100, tg.EDGES)
    assert set(g.dc.tolist()) == set(range(3, 9)) and set(g.dv.tolist()) == set(range(1, 9))
    assert (hi.n, hi.m, hi.E) == (1403, 1101, tg.EDGES + 9 + 12 + 20 + 40)
    assert set(hi.dc.tolist()) == set(range(3, 9)) | {40} and set(hi.dv.tolist()) == set(range(1, 9)) | {9, 12, 20}
    assert hi.dv[1400:].tolist() == [9, 12, 20] and hi.dc[1100] == 40 and (hi.dc == 40).sum() == 1
    for graph in (g, hi):
        assert 4 * graph.n + 2 * graph.E <= 16384                # the rows one 256-codeword tile touches: at most 4 MiB
        assert -(-graph.m // 256) == 5
        assert graph.E < 8 * graph.m                             # two checks per wave in cn_sweep and cn_gather
        pairs = set(zip(graph.check_of_edge.tolist(), graph.var_idx.tolist()))
        assert len(pairs) == graph.E                             # no doubled edge
    # m1100_hi IS m1100 plus the new nodes: dropping them gives the old edge list
    old = (hi.check_of_edge < 1100) & (hi.var_idx < 1400)
    assert set(zip(hi.check_of_edge[old].tolist(), hi.var_idx[old].tolist())) == set(zip(g.check_of_edge.tolist(), g.var_idx.tolist()))
    small = ds.load_code("tg-small96").tanner_graph()
    assert (small.n, small.m) == (96, 48)
    for code in tg.CODES:
        assert len(tg.stuck_variables(ds.load_code(code).tanner_graph())) >= 1


def test_the_pool_holds_every_class_of_row():
    for code in tg.CODES:
        x64, x32 = tg.pool(code, tg.F64), tg.pool(code, tg.F32)
        assert x64.shape == (tg.POOL, ds.load_code(code).n) and x32.dtype == np.float32 and not x32.flags.writeable
        np.testing.assert_array_equal(x32, x64.astype(np.float32))
        assert [int((tg.CLASS == c).sum()) for c in range(5)] == [128, 256, 128, 128, 384]
        assert (x32[tg.rows_of(tg.STRONG)] >= 3).all()
        never = x32[tg.rows_of(tg.NEVER)]
        assert ((never < -1000).sum(axis=1) >= 1).all() and ((never < 0).sum(axis=1) <= tg.WRONG).all()
        r = x32[tg.rows_of(tg.ROUNDED)]
        assert np.array_equal(r * 4, np.round(r * 4)) and (r != 0).all()
        ties = [len(np.unique(np.abs(row))) for row in r]
        assert max(ties) < r.shape[1]                            # equal magnitudes inside every rounded row
        assert ((x32[tg.rows_of(tg.ZEROS)] == 0).sum(axis=1) == 3).all()
        assert not (x32[tg.CLASS != tg.ZEROS] == 0).any()
        assert len(np.unique(np.round(x32[tg.rows_of(tg.MIXED)].mean(axis=1)))) >= 2     # more than one SNR


@pytest.mark.parametrize("family,code", [(f, c) for f, c in tg.FAMILY_CODES if tg.FAMILIES[f].mode not in ("gather", "sweeps")])
def test_the_restatement_decodes_part_of_the_pool_over_several_iterations(family, code, oracle_mod):
    """the three W-RCQ modes share one decoder and one restatement: the pair family stands for them"""
    for early_stop in tg.STOPS:
        want = tg.expected(oracle_mod, family, code, early_stop)
        assert want.bits.shape == (tg.POOL, ds.load_code(code).n) and want.iterations.shape == (tg.POOL,)
        if not early_stop:
            assert (want.iterations == tg.T).all()
            continue
        frac = want.success.mean()
        stops = np.unique(want.iterations)
        print(f"{family} on {code}: the restatement decodes {frac:.1%}, stop iterations {np.bincount(want.iterations, minlength=tg.T + 1).tolist()}")
        assert 0.2 <= frac <= 0.8
        assert len(stops) >= 3
        assert np.all(want.iterations[~want.success] == tg.T) and np.all(want.iterations >= 1)
        strong, never = tg.rows_of(tg.STRONG), tg.rows_of(tg.NEVER)
        assert want.success[strong].all() and (want.iterations[strong] == 1).all()
        assert not want.success[never].any()
        if want.keep is not None:                                # sum-product: the frames the tolerance rule cannot decide
            print(f"  non-decisive frames: {int((~want.keep).sum())} of {tg.POOL}")
            assert (~want.keep).sum() <= 0.01 * tg.POOL
            assert want.keep[strong].all()
            fixed = tg.expected(oracle_mod, family, code, False)
            assert (~fixed.keep).sum() <= 0.01 * tg.POOL


@pytest.mark.parametrize("W", [256, 128])
def test_every_arrangement_holds_the_three_kinds_of_tile(W, oracle_mod):
    family = "nms32" if W == 256 else "nms64"
    assert tg.width(family) == W
    want_ragged = dict(zip(tg.TILES, [0, 1, W - 1] * 4))
    singles = 0
    for code in tg.CODES:
        # a row stops at iteration 1 / never stops under EVERY family that decodes the code
        first = np.ones(tg.POOL, bool)
        never = np.ones(tg.POOL, bool)
        for f, c in tg.FAMILY_CODES:
            if c == code and tg.FAMILIES[f].mode not in ("gather", "sweeps"):
                e = tg.expected(oracle_mod, f, code, True)
                first &= e.success & (e.iterations == 1)
                never &= ~e.success
        for a in tg.arrangements(family, tg.TILES):
            assert a.W == W and a.B == a.tiles * W - want_ragged[a.tiles] and a.index.shape == (a.B,)
            assert -(-a.B // W) == a.tiles and a.index.min() >= 0 and a.index.max() < tg.POOL
            assert len({a.strong_tile, a.never_tile, a.mixed_tile}) == 3 and max(a.strong_tile, a.never_tile, a.mixed_tile) < a.tiles - 1
            tile = lambda t: a.index[t * W:(t + 1) * W]
            assert first[tile(a.strong_tile)].all()              # done after iteration 1: draws no ticket from then on
            assert never[tile(a.never_tile)].all()
            m = tile(a.mixed_tile)
            assert first[m].any() and never[m].any() and (~first[m] & ~never[m]).any()
            if a.B % W == 1:                                     # the last tile holds one frame, and it stops at once
                assert first[a.index[-1]]
                singles += code == tg.CODES[0]
        largest = tg.arrangement(max(tg.TILES), W)
        assert set(largest.index.tolist()) == set(range(tg.POOL))
    assert singles >= 1
    assert sorted(tg.RUN_ORDER) == sorted(tg.TILES) and tg.RUN_ORDER[:4] == (65, 5, 64, 17)
    assert set(tg.NEIGHBOURS) <= set(tg.TILES)


def test_launch_geometry_hook_rejects_bad_arguments():
    import _native
    lib = _native.load()
    out = np.full(8, -7, np.int64)
    assert "ldpc_debug_launch_geometry" in _native.DEBUG_EXPORTS
    assert lib.ldpc_debug_launch_geometry(None, 65, _native.ptr(out)) == -1                 # LDPC_ERR_ARG
    assert (out == -7).all()
    # with a live decoder (NULL output, batch 0, a decoder on a resident engine): tests/test_gpu_tile_geometry.py
