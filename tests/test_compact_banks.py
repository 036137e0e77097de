"""
Host-only tests of the compact fixed-T plan's slot placement (csrc/ldpc_plan.h: cpt_place_banks) through
ldpc_debug_compact_banks (include/ldpc_hip_debug.h), which touches no device.  Check position p runs one check and its
edges sit in the slots row * stride + p; the planner chooses the position of a check among the checks of its degree, the
row of every edge and the variables' lanes so that the variable phase's gathers and scatters meet few LDS bank conflicts.
Checked on the (1998,1512) code and on the random codes of test_compact_layout: every edge in one slot of its own below
Sc, the rows of a check a permutation of 0 .. dc-1, the check positions a permutation that keeps every position's degree,
two calls identical, the model cost never above that of the placement the search starts from, and on the flagship the
passes per lane group under the bounds of the design.
"""
import numpy as np
import pytest

from test_compact_layout import CENSUSES, flagship, random_code

FLAGSHIP_SCATTER = 1.25      # LDS cycles per 16-lane group of a ds_write_b64 (1 = conflict-free; CSR rows at stride 496: 1.96)
FLAGSHIP_GATHER = 1.85       # LDS cycles per 32-lane group of a ds_read_b64 (CSR rows at stride 496: 2.06)


def banks(check_ptr, var_idx, n):
    import _native
    lib = _native.load()
    cp = np.ascontiguousarray(check_ptr, dtype=np.int32)
    vi = np.ascontiguousarray(var_idx, dtype=np.int32)
    m, E = len(cp) - 1, len(vi)
    out = {"slots": np.full(E, -7, np.int32), "pos": np.full(m, -7, np.int32), "model": np.zeros(4, np.int32),
           "base_slots": np.full(E, -7, np.int32), "base_pos": np.full(m, -7, np.int32),
           "base_model": np.zeros(4, np.int32), "geometry": np.zeros(2, np.int32)}
    rc = lib.ldpc_debug_compact_banks(None, n, m, E, _native.ptr(cp), _native.ptr(vi), *[_native.ptr(v) for v in out.values()])
    return rc, out


def check_placement(check_ptr, slots, pos, stride, Sc):
    cp = np.asarray(check_ptr)
    m, E = len(cp) - 1, int(cp[-1])
    dc = np.diff(cp)
    # every edge owns exactly one slot below Sc
    assert slots.min() >= 0 and slots.max() < Sc
    assert len(np.unique(slots)) == E
    # check positions: a permutation of 0 .. m-1 under which every position keeps the degree of the descending order
    assert sorted(pos.tolist()) == list(range(m))
    deg_at = np.empty(m, np.int64)
    deg_at[pos] = dc
    np.testing.assert_array_equal(deg_at, np.sort(dc)[::-1])
    # the slots of a check: its own position as the column, the rows a permutation of 0 .. dc-1
    for c in range(m):
        s = slots[cp[c]: cp[c + 1]]
        np.testing.assert_array_equal(s % stride, np.full(dc[c], pos[c]))
        assert sorted((s // stride).tolist()) == list(range(dc[c])), c


def check_graph(check_ptr, var_idx, n):
    rc, a = banks(check_ptr, var_idx, n)
    assert rc == 0
    stride, Sc = int(a["geometry"][0]), int(a["geometry"][1])
    assert stride % 2 == 1 and stride >= len(check_ptr) - 1
    check_placement(check_ptr, a["slots"], a["pos"], stride, Sc)
    check_placement(check_ptr, a["base_slots"], a["base_pos"], stride, Sc)
    # the starting placement: stable degree order, rows in CSR order
    cp, dc = np.asarray(check_ptr), np.diff(check_ptr)
    np.testing.assert_array_equal(a["base_pos"][np.argsort(-dc, kind="stable")], np.arange(len(dc)))
    for c in range(len(dc)):
        np.testing.assert_array_equal(a["base_slots"][cp[c]: cp[c + 1]] // stride, np.arange(dc[c]))
    # one group per lane group and edge index that holds an edge: the same under both placements, each costs >= 1
    g_cost, g_groups, s_cost, s_groups = (int(x) for x in a["model"])
    bg_cost, bg_groups, bs_cost, bs_groups = (int(x) for x in a["base_model"])
    assert (g_groups, s_groups) == (bg_groups, bs_groups)
    assert g_cost >= g_groups and s_cost >= s_groups
    assert g_cost + s_cost <= bg_cost + bs_cost
    _, b = banks(check_ptr, var_idx, n)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    return a


def test_flagship_placement():
    cp, vi, n = flagship()
    a = check_graph(cp, vi, n)
    g_cost, g_groups, s_cost, s_groups = (int(x) for x in a["model"])
    print("flagship model:", a["model"], "start:", a["base_model"], "geometry:", a["geometry"])
    assert a["geometry"][0] == 495 and a["geometry"][1] == 13 * 495 + 269     # 269 checks of the largest degree, 14
    assert s_cost / s_groups <= FLAGSHIP_SCATTER
    assert g_cost / g_groups <= FLAGSHIP_GATHER


@pytest.mark.parametrize("k", range(len(CENSUSES)))
def test_random_code_placements(k):
    n, m, census = CENSUSES[k]
    rng = np.random.default_rng(70 + k)
    dv_seq = rng.permutation(np.repeat(list(census), list(census.values())))
    _, cp, vi = random_code(rng, n, m, dv_seq)
    check_graph(cp, vi, n)


def test_random_degree_mixes():
    """random censuses (the generator of test_compact_layout): the invariants hold whenever the graph qualifies"""
    rng = np.random.default_rng(9)
    seen = 0
    for _ in range(12):
        n = int(rng.integers(64, 2049))
        m = int(rng.integers(max(8, n // 6), min(496, n)))
        w = rng.dirichlet(np.ones(9) * 0.5)
        dv_seq = rng.choice(9, size=n, p=w)
        dv_seq[dv_seq > 4] = np.where(np.arange((dv_seq > 4).sum()) < 512, dv_seq[dv_seq > 4], 3)
        dv_seq = np.minimum(dv_seq, m)
        _, cp, vi = random_code(rng, n, m, dv_seq)
        if banks(cp, vi, n)[0] != 0:
            continue
        check_graph(cp, vi, n)
        seen += 1
    assert seen >= 3


def test_graph_that_does_not_qualify_is_refused():
    rng = np.random.default_rng(3)
    _, cp, vi = random_code(rng, 900, 600, np.full(900, 3))      # m = 600 > 495
    assert banks(cp, vi, 900)[0] != 0
