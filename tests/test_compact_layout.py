"""
Host-only tests of the compact fixed-T plan's variable grid (csrc/ldpc_plan.h: cpt_assign / cpt_layout) through
ldpc_debug_compact_layout (include/ldpc_hip_debug.h), which touches no device.  The compact kernel runs the variable at
q = r*512 + w*64 + lane in round r of wave w; the cell table tells each wave what its four rounds hold.  Checked on the
(1998,1512) code and on random codes: every variable at exactly one position, degree > 4 variables in round 0, the
table equal to the degrees placed, the model costs as stated, and the flagship's worst wave at the documented bound.
"""

import numpy as np
import pytest

WAVES, ROUNDS, LANES = 8, 4, 64
EMPTY, HOLES, MIXED = 0x00, 0x40, 0xFF
FLAGSHIP_WORST = 118         # largest per-wave cost of the (1998,1512) code's grid; parent order: 134


def body_cost(dv):
    return dv * (dv - 1) + 2 * dv + 4


def layout(check_ptr, var_idx, n):
    import _native
    lib = _native.load()
    cp = np.ascontiguousarray(check_ptr, dtype=np.int32)
    vi = np.ascontiguousarray(var_idx, dtype=np.int32)
    pos = np.full(n, -7, dtype=np.int32)
    cells = np.zeros(WAVES * ROUNDS, dtype=np.uint8)
    stats = np.zeros(4, dtype=np.int32)
    rc = lib.ldpc_debug_compact_layout(None, n, len(cp) - 1, len(vi), _native.ptr(cp), _native.ptr(vi),
                                       _native.ptr(pos), _native.ptr(cells), _native.ptr(stats))
    return rc, pos, cells, stats


def degrees(check_ptr, var_idx, n):
    return np.bincount(np.asarray(var_idx), minlength=n)


def check_grid(check_ptr, var_idx, n):
    rc, pos, cells, stats = layout(check_ptr, var_idx, n)
    assert rc == 0
    dv = degrees(check_ptr, var_idx, n)
    # every variable at exactly one position, inside the grid
    assert pos.min() >= 0 and pos.max() < ROUNDS * WAVES * LANES
    assert len(np.unique(pos)) == n
    n_pos = int(stats[0])
    assert n_pos == pos.max() + 1
    # degree > 4 only in round 0 (the only round with the upper offset half)
    assert np.all(pos[dv > 4] < WAVES * LANES)
    # the table describes the degrees placed; the model costs follow from it
    grid = np.full(ROUNDS * WAVES * LANES, -1, dtype=np.int64)
    grid[pos] = dv
    worst = total = mixed = 0
    for w in range(WAVES):
        wave = 0
        for r in range(ROUNDS):
            lane_dv = grid[r * 512 + w * 64: r * 512 + w * 64 + 64]
            used = lane_dv[lane_dv >= 0]
            kinds = sorted(set(used.tolist()))
            if len(used) == 0:
                want = EMPTY
            elif len(kinds) == 1 and kinds[0] > 0:
                want = kinds[0] | (HOLES if len(used) < LANES else 0)
            else:
                want = MIXED
            assert cells[w * ROUNDS + r] == want, (w, r, kinds, len(used))
            mixed += want == MIXED
            wave += sum(body_cost(d) for d in kinds)
        worst = max(worst, wave)
        total += wave
    assert (int(stats[1]), int(stats[2]), int(stats[3])) == (worst, total, mixed)
    return pos, cells, stats, dv


def flagship():
    import codes
    g = codes.load_code("ira_1998_1512").tanner_graph()
    return g.check_ptr, g.var_idx, g.n


def test_flagship_grid_is_balanced():
    cp, vi, n = flagship()
    pos, cells, stats, dv = check_grid(cp, vi, n)
    assert sorted(np.bincount(dv).tolist()) == sorted([0, 1, 485, 1296, 0, 0, 0, 0, 216])   # the issue's census
    assert stats[1] <= FLAGSHIP_WORST
    assert stats[3] <= 2                     # 34 cells of one degree would not fit 32: at most this many mixed
    # waves w and w + 4 (one SIMD, assumed) carry about the same work
    grid = np.full(2048, -1)
    grid[pos] = dv
    wave = [sum(sum(body_cost(d) for d in set(grid[r * 512 + w * 64: r * 512 + w * 64 + 64].tolist()) if d >= 0)
                for r in range(ROUNDS)) for w in range(WAVES)]
    pair = [wave[w] + wave[w + 4] for w in range(4)]
    assert max(pair) - min(pair) <= 32, (wave, pair)


def test_flagship_grid_is_deterministic():
    cp, vi, n = flagship()
    a = layout(cp, vi, n)
    b = layout(cp, vi, n)
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


def random_code(rng, n, m, dv_seq):
    """variables of the given degrees, each on the dv checks of lowest current degree (random tie break)"""
    H = np.zeros((m, n), dtype=np.int64)
    deg = np.zeros(m, dtype=np.int64)
    for j, d in enumerate(dv_seq):
        cand = rng.permutation(m)
        pick = cand[np.argsort(deg[cand], kind="stable")[:d]]
        H[pick, j] = 1
        deg[pick] += 1
    check_ptr = np.concatenate([[0], np.cumsum(H.sum(axis=1))])
    var_idx = np.concatenate([np.nonzero(H[i])[0] for i in range(m)])
    return H, check_ptr, var_idx


CENSUSES = [
    # (n, m, {degree: count}): many degrees (mixed cells), partial cells (holes), dv 1, dv 5-8 over several waves
    (1200, 400, {7: 150, 5: 100, 6: 80, 8: 20, 3: 500, 2: 300, 1: 49, 4: 1}),
    (2000, 490, {8: 100, 6: 412, 3: 300, 2: 1100, 1: 88}),
    (1900, 490, {5: 500, 4: 300, 3: 600, 2: 499, 1: 1}),
    (700, 300, {8: 70, 7: 70, 6: 70, 5: 70, 4: 70, 3: 70, 2: 70, 1: 70, 0: 140}),
    (90, 40, {3: 60, 2: 30}),
]


@pytest.mark.parametrize("k", range(len(CENSUSES)))
def test_random_code_grids(k):
    n, m, census = CENSUSES[k]
    rng = np.random.default_rng(70 + k)
    dv_seq = rng.permutation(np.repeat(list(census), list(census.values())))
    assert len(dv_seq) == n
    _, cp, vi = random_code(rng, n, m, dv_seq)
    pos, cells, stats, dv = check_grid(cp, vi, n)
    hi_waves = {int(p) // 64 for p in pos[dv > 4]}
    if (dv > 4).sum() > 64:
        assert len(hi_waves) >= 2


def test_random_degree_mixes():
    """random censuses: the invariants hold whenever the graph qualifies"""
    rng = np.random.default_rng(9)
    for _ in range(12):
        n = int(rng.integers(64, 2049))
        m = int(rng.integers(max(8, n // 6), min(496, n)))
        w = rng.dirichlet(np.ones(9) * 0.5)
        dv_seq = rng.choice(9, size=n, p=w)
        dv_seq[dv_seq > 4] = np.where(np.arange((dv_seq > 4).sum()) < 512, dv_seq[dv_seq > 4], 3)
        dv_seq = np.minimum(dv_seq, m)
        _, cp, vi = random_code(rng, n, m, dv_seq)
        rc = layout(cp, vi, n)[0]
        if rc != 0:                      # e.g. a check wider than 32 or a staging area below n
            continue
        check_grid(cp, vi, n)


def test_graph_that_does_not_qualify_is_refused():
    rng = np.random.default_rng(3)
    _, cp, vi = random_code(rng, 900, 600, np.full(900, 3))      # m = 600 > 496
    assert layout(cp, vi, 900)[0] != 0
