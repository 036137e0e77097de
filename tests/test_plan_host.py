"""
Host test of the resident-plan builder on its own (csrc/ldpc_plan.h).  tests/plan_host_shim.cpp and the planner header
are compiled with g++ and the address / undefined-behaviour sanitizers into a stand-alone program (its own process, so the
sanitizer runtime comes first and no GPU is ever opened); the program reads a graph and the planner's inputs from a file
and writes every table of the general plan and of the compact plan.

Compact plan: grid, cells, stats, check words, slots, check positions, both bank models and the geometry equal what
ldpc_debug_compact_layout / _checks / _banks of the hipcc-built library return for the bare graph (d = NULL) -- two
compilers, one result -- on the (1998,1512) code and the random codes of test_compact_layout.
General plan: its invariants, from the graph alone, on the (1998,1512) code, small_96_48 and a code with split checks,
each with a per-edge and a per-check beta table.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_compact_layout import CENSUSES, random_code

F32, NMS = 0, 0
HOLE = 0xFFFFFFFF
GXX_FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed: the planner's host program cannot be built")
    exe = str(tmp_path_factory.mktemp("plan_host") / "plan_host_shim")
    cmd = [gxx] + GXX_FLAGS + ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "plan_host_shim.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return exe


def run_planner(exe, tmp_path, cp, vi, n, beta_slot, alpha_slot, n_beta, n_alpha, T=10):
    cp, vi = np.asarray(cp, dtype=np.int64), np.asarray(vi, dtype=np.int64)
    m, E = len(cp) - 1, len(vi)
    per_check = all(len(set(beta_slot[cp[i]:cp[i + 1]].tolist())) <= 1 for i in range(m))
    src, dst = str(tmp_path / "plan.in"), str(tmp_path / "plan.out")
    with open(src, "w") as f:
        for row in ([n, m, E], cp, vi, [F32, NMS, T, n_beta, n_alpha, 0, int(per_check), 0, 0], beta_slot, alpha_slot):
            f.write(" ".join(str(int(x)) for x in row) + "\n")
    res = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    with open(dst) as f:
        for line in f:
            name, count, *vals = line.split()
            out[name] = np.array(vals, dtype=np.int64)
            assert len(vals) == int(count), name
    return out


# ---- compact plan: the g++ program against the hipcc library's host hooks ---------------------------------------------
def hooks(cp, vi, n):
    import _native
    lib = _native.load()
    cp, vi = np.ascontiguousarray(cp, dtype=np.int32), np.ascontiguousarray(vi, dtype=np.int32)
    m, E = len(cp) - 1, len(vi)
    graph = (None, n, m, E, _native.ptr(cp), _native.ptr(vi))
    pos, cells, stats = np.full(n, -7, dtype=np.int32), np.zeros(32, dtype=np.uint8), np.zeros(4, dtype=np.int32)
    assert lib.ldpc_debug_compact_layout(*graph, _native.ptr(pos), _native.ptr(cells), _native.ptr(stats)) == 0
    words = np.zeros(8, dtype=np.uint32)
    assert lib.ldpc_debug_compact_checks(*graph, _native.ptr(words)) == 0
    slots, base_slots = np.zeros(E, dtype=np.int32), np.zeros(E, dtype=np.int32)
    cpos, base_cpos = np.full(m, -7, dtype=np.int32), np.full(m, -7, dtype=np.int32)
    model, base_model, geometry = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32), np.zeros(2, dtype=np.int32)
    assert lib.ldpc_debug_compact_banks(*graph, _native.ptr(slots), _native.ptr(cpos), _native.ptr(model), _native.ptr(base_slots),
                                        _native.ptr(base_cpos), _native.ptr(base_model), _native.ptr(geometry)) == 0
    return dict(pos=pos, cells=cells, stats=stats, words=words, slots=slots, cpos=cpos, model=model, base_slots=base_slots,
                base_cpos=base_cpos, base_model=base_model, geometry=geometry)


def compact_cases():
    import codes
    g = codes.load_code("ira_1998_1512").tanner_graph()
    yield "ira_1998_1512", g.check_ptr, g.var_idx, g.n
    for k, (n, m, census) in enumerate(CENSUSES):
        rng = np.random.default_rng(70 + k)                      # test_compact_layout.test_random_code_grids' codes
        dv_seq = rng.permutation(np.repeat(list(census), list(census.values())))
        _, cp, vi = random_code(rng, n, m, dv_seq)
        yield "census%d" % k, cp, vi, n


@pytest.mark.parametrize("k", range(1 + len(CENSUSES)))
def test_compact_plan_equals_the_engine_librarys(shim, tmp_path, k):
    name, cp, vi, n = list(compact_cases())[k]
    m, E = len(cp) - 1, len(vi)
    got = run_planner(shim, tmp_path, cp, vi, n, np.zeros(E, dtype=np.int64), np.zeros(n, dtype=np.int64), 1, 1)
    want = hooks(cp, vi, n)
    assert "cpt.var_at" in got, name

    def inverse(at, size):
        inv = np.full(size, -1, dtype=np.int64)
        inv[at[at >= 0]] = np.nonzero(at >= 0)[0]
        return inv
    np.testing.assert_array_equal(inverse(got["cpt.var_at"], n), want["pos"])
    cells = np.array([(got["cpt.cell"][c // 4] >> (8 * (c % 4))) & 0xFF for c in range(32)])
    np.testing.assert_array_equal(cells, want["cells"])
    np.testing.assert_array_equal(got["cpt.stats"], want["stats"])
    np.testing.assert_array_equal(got["cpt.words"], want["words"])
    np.testing.assert_array_equal(got["cpt.slot_of_edge"], want["slots"])
    np.testing.assert_array_equal(inverse(got["cpt.check_of_pos"], m), want["cpos"])
    np.testing.assert_array_equal(got["cpt.banks"], want["model"])
    np.testing.assert_array_equal(got["cpt.base_slot_of_edge"], want["base_slots"])
    np.testing.assert_array_equal(inverse(got["cpt.base_check_of_pos"], m), want["base_cpos"])
    np.testing.assert_array_equal(got["cpt.base_banks"], want["base_model"])
    np.testing.assert_array_equal(got["cpt.geometry"], want["geometry"])
    if got["choice"][1]:                                        # the decoder's compact plan sits on that very placement
        sc = dict(zip("n m S max_dc max_dv mstride E any_split par_words par_shift n_hi n_pos".split(), got["resc.scalars"]))
        assert (sc["mstride"], sc["S"]) == tuple(want["geometry"]) and sc["n_pos"] == want["stats"][0]
        eos = got["resc.edge_of_slot"]
        np.testing.assert_array_equal(np.nonzero(eos != HOLE)[0][np.argsort(eos[eos != HOLE], kind="stable")], want["slots"])
        np.testing.assert_array_equal(got["resc.inv_perm_v"], want["pos"])
        np.testing.assert_array_equal(got["resc.ccell"], want["words"])   # NMS, one beta per check: the select form


# ---- general plan: invariants from the graph alone ---------------------------------------------------------------------
def split_check_code():
    """300 variables of degree <= 8 on 40 checks; check 0 has degree 70 (8 sub-checks), check 1 degree 40 (4 sub-checks)"""
    rng = np.random.default_rng(11)
    H, _, _ = random_code(rng, 300, 38, rng.permutation(np.repeat([2, 3, 6], [150, 100, 50])))
    wide = np.zeros((2, 300), dtype=np.int64)
    wide[0, rng.choice(300, 70, replace=False)] = 1
    wide[1, rng.choice(300, 40, replace=False)] = 1
    H = np.vstack([wide, H])
    assert H.sum(axis=0).max() <= 8 and H.sum(axis=1).max() == 70 and sorted(H.sum(axis=1))[-2] > 32
    check_ptr = np.concatenate([[0], np.cumsum(H.sum(axis=1))])
    var_idx = np.concatenate([np.nonzero(H[i])[0] for i in range(H.shape[0])])
    return check_ptr, var_idx, 300


def general_graph(name):
    if name == "split":
        return split_check_code()
    import codes
    g = codes.load_code(name).tanner_graph()
    return g.check_ptr, g.var_idx, g.n


@pytest.mark.parametrize("beta", ["per_check", "per_edge"])
@pytest.mark.parametrize("name", ["ira_1998_1512", "small_96_48", "split"])
def test_general_plan_invariants(shim, tmp_path, name, beta):
    cp, vi, n = general_graph(name)
    cp, vi = np.asarray(cp, dtype=np.int64), np.asarray(vi, dtype=np.int64)
    m, E = len(cp) - 1, len(vi)
    dc, dv = np.diff(cp), np.bincount(vi, minlength=n)
    check_of_edge = np.repeat(np.arange(m), dc)
    n_beta, n_alpha = 5, 7
    beta_slot = check_of_edge % n_beta if beta == "per_check" else (np.arange(E) * 3) % n_beta
    alpha_slot = np.arange(n) % n_alpha
    got = run_planner(shim, tmp_path, cp, vi, n, beta_slot, alpha_slot, n_beta, n_alpha)
    res_ok, _, G, NT = got["choice"][:4]
    assert res_ok and G in (1, 2) and NT in (512, 1024)
    sc = dict(zip("n m S max_dc max_dv mstride E any_split par_words par_shift n_hi n_pos per_check has_oaslot".split(),
                  got["res.scalars"]))
    S, mstride, mv = sc["S"], sc["mstride"], sc["m"]
    assert (sc["n"], sc["E"], sc["n_pos"], sc["max_dv"]) == (n, E, n, dv.max())
    assert sc["any_split"] == int(dc.max() > 32) == int(name == "split") and (mv == m) == (not sc["any_split"])
    assert S == sc["max_dc"] * mstride and mstride >= mv and S * G * 4 <= 65535      # 16-bit byte offsets

    # every edge in exactly one slot below S; edge_of_slot is the inverse map, 0xffffffff elsewhere
    eos = got["res.edge_of_slot"]
    assert len(eos) == S
    used = np.nonzero(eos != HOLE)[0]
    np.testing.assert_array_equal(np.sort(eos[used]), np.arange(E))
    slot_of_edge = np.empty(E, dtype=np.int64)
    slot_of_edge[eos[used]] = used
    # cvar: the position of the edge's variable under inv_perm_v; bslot: the edge's beta column
    inv = got["res.inv_perm_v"]
    np.testing.assert_array_equal(np.sort(inv), np.arange(n))
    np.testing.assert_array_equal(got["res.cvar"][slot_of_edge], inv[vi])
    np.testing.assert_array_equal(got["res.bslot"][slot_of_edge], beta_slot)
    # vslot offsets = slot * G * 4 in CSC order (a variable's edges by ascending check = ascending edge id); vmeta
    lo, hi = got["res.vslot_lo"].reshape(-1, 2), got["res.vslot_hi"].reshape(-1, 2)
    assert len(lo) == n and len(hi) == max(sc["n_hi"], 1) and len(got["res.vmeta"]) == n
    csc = np.argsort(vi, kind="stable")
    var_ptr = np.concatenate([[0], np.cumsum(dv)])
    for j in range(n):
        q = inv[j]
        words = list(lo[q]) + (list(hi[q]) if q < len(hi) else [0, 0])
        offs = [(words[k // 2] >> (16 * (k % 2))) & 0xFFFF for k in range(8)]
        want = (slot_of_edge[csc[var_ptr[j]:var_ptr[j + 1]]] * G * 4).tolist()
        assert offs[:dv[j]] == want and not any(offs[dv[j]:]), j
        assert got["res.vmeta"][q] == dv[j] | (alpha_slot[j] << 8)
    # the degree > 4 variables are exactly the first n_hi positions
    np.testing.assert_array_equal(np.sort(inv[dv > 4]), np.arange(sc["n_hi"]))
    assert sc["n_hi"] == (dv > 4).sum()

    # positions: slot = row * mstride + position; a position holds edges of ONE check in rows 0 .. dc_s - 1
    pos_of_edge, row_of_edge = slot_of_edge % mstride, slot_of_edge // mstride
    assert pos_of_edge.max() < mv
    dc_s = got["res.dc_s"]
    assert len(dc_s) == mv
    check_at = np.full(mv, -1, dtype=np.int64)
    for p in range(mv):
        at = np.nonzero(pos_of_edge == p)[0]
        assert len(at) == dc_s[p] and sorted(row_of_edge[at]) == list(range(dc_s[p])), p
        assert len(set(check_of_edge[at].tolist())) == 1, p
        check_at[p] = check_of_edge[at[0]]
    np.testing.assert_array_equal(np.bincount(check_at, weights=dc_s, minlength=m), dc)
    # sub-checks of one split check are adjacent and each group starts at a multiple of its size
    assert ("res.gsz" in got) == bool(sc["any_split"])
    gsz = got["res.gsz"] if sc["any_split"] else np.ones(mv, dtype=np.int64)
    for i in range(m):
        at = np.nonzero(check_at == i)[0]
        k = len(at)
        assert k == (1 if dc[i] <= 32 else 1 << int(np.ceil(np.log2(dc[i] / 16)))), i
        assert np.all(gsz[at] == k) and np.array_equal(at, at[0] + np.arange(k)) and at[0] % k == 0, i
        assert dc_s[at].max() <= (32 if k == 1 else 16)
    # bslot_c is present exactly when every check has one beta slot
    assert ("res.bslot_c" in got) == bool(sc["per_check"]) == (beta == "per_check")
    if beta == "per_check":
        np.testing.assert_array_equal(got["res.bslot_c"], check_at % n_beta)
    assert "res.oaslot" not in got and not sc["has_oaslot"]
