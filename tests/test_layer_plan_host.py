"""
Host test of the block-parallel layered decode's planner on its own (csrc/ldpc_layer_plan.h).  tests/layer_plan_shim.cpp
and the planner header are compiled with g++ and the address / undefined-behaviour sanitizers into a stand-alone program
(its own process, so the sanitizer runtime comes first and no GPU is ever opened); the program reads a graph and a layer
partition from a file and writes every table of the plan.

Invariants, from the graph alone, on every case graph of tests/block_layered_cases.py and for both record kinds: every
edge appears once, offsets lie inside the codeword's row, the lanes of one layer step never share a posterior word,
chunks of lpc checks cover the layer, and G rows fit LDS.  Where the hipcc-built library exists its host-only hook
ldpc_debug_layer_plan returns the same geometry -- two compilers, one result; tests/test_gpu_block_layered.py compares
that hook with ldpc_decoder_info on the device.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import block_layered_cases as bc
from conftest import PKG, ROOT

MINSUM, RCQ = 0, 1
HOLE = 0xFFFFFFFF
GXX_FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
SCALARS = ("n m L kind W G lpc threads max_layer entries row_words rec_off lds_bytes flag_words lds_limit max_threads "
           "max_deg").split()


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not installed: the planner's host program cannot be built")
    exe = str(tmp_path_factory.mktemp("layer_plan") / "layer_plan_shim")
    cmd = [gxx] + GXX_FLAGS + ["-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "layer_plan_shim.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return exe


def run_planner(exe, tmp_path, n, cp, vi, lp, kind):
    src, dst = str(tmp_path / "plan.in"), str(tmp_path / "plan.out")
    with open(src, "w") as f:
        for row in ([n, len(cp) - 1, len(vi), len(lp) - 1, kind], cp, vi, lp):
            f.write(" ".join(str(int(x)) for x in row) + "\n")
    res = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    with open(dst) as f:
        for line in f:
            name, rest = line.split(" ", 1)
            if name in ("partition_error", "why"):
                out[name] = rest.strip()
                continue
            count, *vals = rest.split()
            out[name] = np.array(vals, dtype=np.int64)
            assert len(vals) == int(count), name
    return out


@pytest.mark.parametrize("kind", [MINSUM, RCQ])
@pytest.mark.parametrize("name", bc.GRAPHS)
def test_plan_invariants(shim, tmp_path, name, kind):
    g = bc.graph(name)
    got = run_planner(shim, tmp_path, g.n, g.check_ptr, g.var_idx, g.layer_ptr, kind)
    assert got["ok"][0] == 1, got.get("why")
    sc = dict(zip(SCALARS, got["scalars"].tolist()))
    lp, base, deg, off, eoe = (got[k] for k in ("layer_ptr", "entry_base", "deg", "off", "edge_of_entry"))
    assert (sc["n"], sc["m"], sc["L"], sc["kind"]) == (g.n, g.m, g.n_layers, kind)
    np.testing.assert_array_equal(lp, g.layer_ptr)
    np.testing.assert_array_equal(deg, g.dc)
    sizes = np.diff(lp)
    assert sc["max_layer"] == sizes.max() and sc["W"] == (2 if g.dc.max() > 32 else 1) and g.dc.max() <= sc["max_deg"]
    # entries: layer l holds S_l x D_l of them, edge k of its check j at base + k * S_l + j; every edge appears once
    assert len(off) == len(eoe) == sc["entries"] == base[-1] and base[0] == 0
    used = eoe >= 0
    np.testing.assert_array_equal(np.sort(eoe[used]), np.arange(g.E))
    assert (off[~used] == HOLE).all()
    for l in range(g.n_layers):
        c0, S = int(lp[l]), int(sizes[l])
        D = int(g.dc[c0:c0 + S].max())
        assert base[l + 1] - base[l] == S * D
        for j in range(S):
            e0, dc = int(g.check_ptr[c0 + j]), int(g.dc[c0 + j])
            at = base[l] + np.arange(D) * S + j
            np.testing.assert_array_equal(eoe[at[:dc]], e0 + np.arange(dc))
            assert (eoe[at[dc:]] == -1).all()
        # the lanes of one layer step never share a posterior word
        words = off[base[l]:base[l + 1]][used[base[l]:base[l + 1]]]
        assert len(set(words.tolist())) == len(words), l
    # offsets are the variables' words inside the posterior part of the row
    np.testing.assert_array_equal(off[used], 4 * g.var_idx[eoe[used]])
    assert off[used].max() < 4 * sc["rec_off"] and sc["rec_off"] == g.n
    # the row: posteriors, then records (min-sum) or one code byte per entry (RCQ); an odd number of dwords
    tail = (2 + 2 * sc["W"]) * g.m if kind == MINSUM else -(-sc["entries"] // 4)
    assert sc["row_words"] % 2 == 1 and g.n + tail <= sc["row_words"] <= g.n + tail + 1
    # geometry: G rows and the bookkeeping words fit LDS; lanes: G x lpc within a workgroup of whole waves
    G, lpc, threads = sc["G"], sc["lpc"], sc["threads"]
    assert G >= 1 and sc["flag_words"] == 3 * G + 1
    assert sc["lds_bytes"] == 4 * (G * sc["row_words"] + sc["flag_words"]) <= sc["lds_limit"] == 160 * 1024
    assert 1 <= lpc <= sc["max_layer"] and G * lpc <= threads <= sc["max_threads"] and threads % 64 == 0 and threads - G * lpc < 64
    # chunks j, j + lpc, ... of the lpc lanes cover every layer exactly once
    for S in sizes.tolist():
        seen = np.concatenate([np.arange(j, S, lpc) for j in range(lpc)])
        np.testing.assert_array_equal(np.sort(seen), np.arange(S))


def test_what_the_planner_refuses(shim, tmp_path):
    g = bc.graph("qc_3_6_5")
    lp = g.layer_ptr.copy()
    # a layer with a shared variable: checks 0 .. 5 span two block rows
    got = run_planner(shim, tmp_path, g.n, g.check_ptr, g.var_idx, [0, 6, 10, 15], MINSUM)
    assert "layer 0 " in got["partition_error"] and "variable" in got["partition_error"]
    for bad in ([1, 5, 10, 15], [0, 5, 10, 14], [0, 5, 5, 15]):
        assert "layer_ptr" in run_planner(shim, tmp_path, g.n, g.check_ptr, g.var_idx, bad, MINSUM)["partition_error"]
    # a check wider than the record format
    n = 70
    got = run_planner(shim, tmp_path, n, [0, 65, 66], list(range(65)) + [69], [0, 2], MINSUM)
    assert got["ok"][0] == 0 and "65" in got["why"] and "64" in got["why"]
    # one codeword's state beyond LDS: the (16200,7200) code under any partition
    import codes
    import tanner_graph
    big = codes.load_graph("dvbs2_like_16200_7200")
    got = run_planner(shim, tmp_path, big.n, big.check_ptr, big.var_idx, tanner_graph.disjoint_runs(big), MINSUM)
    assert got["ok"][0] == 0 and "LDS" in got["why"]
    np.testing.assert_array_equal(lp, g.layer_ptr)


@pytest.mark.parametrize("name", bc.GRAPHS)
def test_geometry_equals_the_engine_librarys(shim, tmp_path, name):
    """the g++ program against the host-only hook of the hipcc-built library (no device is opened)"""
    import _native
    lib = _native.load()
    g = bc.graph(name)
    cp, vi, lp = (np.ascontiguousarray(a, dtype=np.int32) for a in (g.check_ptr, g.var_idx, g.layer_ptr))
    for kind in (MINSUM, RCQ):
        sc = dict(zip(SCALARS, run_planner(shim, tmp_path, g.n, cp, vi, lp, kind)["scalars"].tolist()))
        out = np.zeros(8, dtype=np.int64)
        assert lib.ldpc_debug_layer_plan(g.n, g.m, g.E, _native.ptr(cp), _native.ptr(vi), len(lp) - 1, _native.ptr(lp), kind,
                                         _native.ptr(out)) == 0
        assert out.tolist() == [1, sc["G"], sc["lpc"], sc["threads"], sc["lds_bytes"], sc["row_words"], sc["entries"], sc["W"]]
