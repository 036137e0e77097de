"""
Host-only tests of the compact fixed-T plan's check table (csrc/ldpc_plan.h: cpt_check_words) through
ldpc_debug_compact_checks (include/ldpc_hip_debug.h), which touches no device.  The plan sorts checks by descending
degree and wave w of the compact kernel runs the checks at positions 64w .. 64w+63; its word tells the wave the smallest
degree d_lo among them (that many edges run on a scalar trip count), the spread d_hi - d_lo (edges left to a lane mask),
how many lanes hold a check, and whether the wave keeps the per-lane form (d_lo < 4).  Checked on the (1998,1512) code
against the figures of DESIGN.md 3c and on the random codes of test_compact_layout.py against degrees recomputed here.
"""

import numpy as np
import pytest

from test_compact_layout import CENSUSES, flagship, random_code

WAVES, LANES = 8, 64
PER_LANE = 1 << 31


def check_words(check_ptr, var_idx, n):
    import _native
    lib = _native.load()
    cp = np.ascontiguousarray(check_ptr, dtype=np.int32)
    vi = np.ascontiguousarray(var_idx, dtype=np.int32)
    words = np.full(WAVES, 0xDEADBEEF, dtype=np.uint32)
    rc = lib.ldpc_debug_compact_checks(None, n, len(cp) - 1, len(vi), _native.ptr(cp), _native.ptr(vi),
                                       _native.ptr(words))
    return rc, words


def fields(word):
    word = int(word)
    return word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF, bool(word & PER_LANE)


def expected_words(check_ptr):
    dc = np.sort(np.diff(np.asarray(check_ptr)))[::-1]          # the plan's order: descending degree
    out = []
    for w in range(WAVES):
        wave = dc[w * LANES:(w + 1) * LANES]
        if len(wave) == 0:
            out.append(0)
            continue
        lo, hi = int(wave.min()), int(wave.max())
        out.append(lo | (hi - lo) << 8 | len(wave) << 16 | (PER_LANE if lo < 4 else 0))
    return np.array(out, dtype=np.uint32)


def test_flagship_check_table():
    cp, vi, n = flagship()
    rc, words = check_words(cp, vi, n)
    assert rc == 0
    dc = np.diff(cp)
    assert (int((dc == 14).sum()), int((dc == 13).sum()), len(dc)) == (269, 217, 486)
    got = [fields(w) for w in words]
    for w in range(4):
        assert got[w] == (14, 0, 64, False)
    assert got[4] == (13, 1, 64, False)              # 269 = 4 * 64 + 13 checks of degree 14: the boundary wave
    for w in (5, 6):
        assert got[w] == (13, 0, 64, False)
    assert got[7] == (13, 0, 38, False)              # 486 - 7 * 64
    np.testing.assert_array_equal(words, expected_words(cp))


@pytest.mark.parametrize("k", range(len(CENSUSES)))
def test_random_code_check_tables(k):
    n, m, census = CENSUSES[k]
    rng = np.random.default_rng(70 + k)
    dv_seq = rng.permutation(np.repeat(list(census), list(census.values())))
    _, cp, vi = random_code(rng, n, m, dv_seq)
    rc, words = check_words(cp, vi, n)
    assert rc == 0
    np.testing.assert_array_equal(words, expected_words(cp))
    lanes = sum(fields(w)[2] for w in words)
    assert lanes == m


def test_low_degree_waves_keep_the_per_lane_form():
    """checks of degree 1..3 at the end of the order: their waves carry the marker, the waves above them do not"""
    rng = np.random.default_rng(5)
    n, m = 600, 200
    H = np.zeros((m, n), dtype=np.int64)
    want = np.concatenate([np.full(100, 9), np.full(40, 6), np.full(30, 3), np.full(20, 2), np.full(10, 1)])
    for i, d in enumerate(want):
        H[i, rng.choice(n, size=d, replace=False)] = 1
    for j in np.nonzero(H.sum(axis=0) == 0)[0]:              # every variable on some degree-9 check (dv <= 8 holds)
        H[rng.integers(0, 100), j] = 1
    assert H.sum(axis=0).max() <= 8
    cp = np.concatenate([[0], np.cumsum(H.sum(axis=1))])
    vi = np.concatenate([np.nonzero(H[i])[0] for i in range(m)])
    rc, words = check_words(cp, vi, n)
    assert rc == 0
    np.testing.assert_array_equal(words, expected_words(cp))
    marks = [fields(w)[3] for w in words]
    assert marks[:2] == [False, False] and marks[2:4] == [True, True] and not any(marks[4:])
    assert all(int(w) == 0 for w in words[4:])               # empty waves: the whole word is zero
    assert fields(words[3])[2] == m - 3 * LANES


def test_graph_that_does_not_qualify_is_refused():
    rng = np.random.default_rng(3)
    _, cp, vi = random_code(rng, 900, 600, np.full(900, 3))      # m = 600 > 496
    assert check_words(cp, vi, 900)[0] != 0
