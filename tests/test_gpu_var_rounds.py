"""
GPU tests (-m gpu) of the compact kernels' variable phase (res_var_phase_cpt): per round a uniform cell branches on its
scalar degree, a cell with holes masks its empty lanes, a mixed cell runs the per-lane switch, an empty cell is skipped;
the slot offsets are extracted from the packed plan words where they are used, and vmeta (a mixed cell's degrees, the
alpha columns) is read through an address formed at its use.  Small codes whose grids together show every cell kind in
every place -- asserted from ldpc_debug_compact_layout, so that a planner change cannot empty the test -- and the
(1998,1512) code once are decoded by Basic, RCQ (bc 3) and Neural-2D type 1 (one alpha column per variable: the vmeta
path) at T = 0, 1, 2, 10, batches of 1, 2 and 5 codewords (a padded last block and full blocks), with and without the
posterior: every output equals the streaming engine's bit for bit, bits / iterations / success equal the CPU oracle's,
the posterior is within test_gpu_compact_grid's POST_TOL (1e-5) of the oracle's.
"""
import numpy as np
import pytest
import torch

from test_gpu_compact_grid import HOLES, MIXED, QP, assert_post, grid_of, llrs, oracle_graph, random_code

pytestmark = pytest.mark.gpu

CODES = {
    # two waves with a single non-empty round (degree 3 and 2, both with holes), everything else empty
    "small": (13, 90, 40, {3: 60, 2: 30}),
    # mixed cells in round 0 (degrees 8 and 6) and in round 1 (2, 1 and empty lanes), odd counts so that in both the degree
    # changes inside a lane pair; round 0 of degree 6 and 8, uniform rounds of degree 1, 2, 3, a holed round 1
    "odd_round0": (12, 2000, 490, {8: 101, 6: 411, 3: 300, 2: 1099, 1: 89}),
    # round 0 of degree 5 (one cell with holes), uniform rounds of degree 4, 3, 2, holed rounds of degree 4, 3, 2, 1
    "five_four": (14, 1900, 490, {5: 500, 4: 300, 3: 600, 2: 499, 1: 1}),
    # round 0 of degree <= 4 in every wave, rounds 1-2 uniform, holed and empty, round 3 empty
    "low": (16, 1100, 300, {4: 200, 3: 300, 2: 300, 1: 300}),
}
T_ALL = (0, 1, 2, 10)
BATCHES = (1, 2, 5)


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def assert_compact(eng):
    """the fixed-T decode of this engine is the compact kernel (a small code may fit more than three workgroups per CU)"""
    info = eng.info()
    assert info["engine"] == "resident" and info["threads_per_workgroup"] == 512
    assert info["resident_kernel"]["fixed_T"]["plan"] == "compact"
    return grid_of(eng)


_codes = {}


def make_code(name, T):
    """one graph per name (built once); the iteration count is the decoder's"""
    from ldpc_decoder import LDPCCode
    if name not in _codes:
        if name == "ira":
            import codes
            _codes[name] = codes.load_code("ira_1998_1512", max_iterations=10)
        else:
            seed, n, m, census = CODES[name]
            _codes[name] = random_code(seed, n, m, census, 10)
    c = _codes[name]
    return LDPCCode(n=c.n, k=c.k, H=c.H, max_iterations=T)


def make_decoder(kind, code, T, dev):
    """(engine, oracle call) of a decoder kind; the oracle call returns (bits, posterior, iterations, success)"""
    if kind == "basic":
        from ldpc_decoder import BasicMinSumDecoder
        eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, dev)
        return eng, lambda om, og, x: om.basic_minsum(og, x, 0.7, T, early_stop=False, dtype=np.float32)
    if kind == "rcq":
        from rcq_decoder import RCQMinSumDecoder
        eng = RCQMinSumDecoder(code, 3, 8, QP, T)._get_engine(dev)
        return eng, lambda om, og, x: om.rcq(og, x, 3, QP, T, early_stop=False)
    from neural_2d_decoder import Neural2DMinSumDecoder
    rng = np.random.default_rng(50 + T)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=1, max_iterations=T)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    eng = dec._get_engine(dev)

    return eng, lambda om, og, x: om.neural2d(og, x, 1, T, beta, alpha, early_stop=False)


FIELDS = ("bits", "posterior", "iterations", "success", "packed_bits")


def same(a, b):
    for f in FIELDS:
        u, v = getattr(a, f), getattr(b, f)
        assert (u is None) == (v is None), f
        if u is not None:
            assert torch.equal(u, v), f


def decode_both(eng, x, want_posterior):
    """compact kernel and streaming engine, every output bit for bit"""
    eng.set_mode("auto")
    a = eng.decode(x, early_stop=False, want_posterior=want_posterior, want_packed=True)
    eng.set_mode("stream")
    b = eng.decode(x, early_stop=False, want_posterior=want_posterior, want_packed=True)
    eng.set_mode("auto")
    same(a, b)
    return a


def check_decoder(kind, name, T, dev, oracle_mod, batches=BATCHES):
    code = make_code(name, T)
    eng, oracle_call = make_decoder(kind, code, T, dev)
    assert_compact(eng)
    og = oracle_graph(oracle_mod, code)
    full = llrs(60 + T, max(batches), code.n)
    ob, op, oi, os_ = oracle_call(oracle_mod, og, full)          # one reference per case, its leading rows per batch
    for B in batches:
        x = torch.from_numpy(full[:B]).to(dev)
        for want_posterior in (True, False):
            res = decode_both(eng, x, want_posterior)
            np.testing.assert_array_equal(res.bits.cpu().numpy(), ob[:B])
            np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi[:B])
            np.testing.assert_array_equal(res.success.cpu().numpy(), os_[:B])
            assert (res.posterior is not None) == want_posterior
            if want_posterior:
                assert_post(res.posterior.cpu().numpy(), op[:B])


def split_pairs(code, cells):
    """rounds with a mixed cell in which two lanes 2k, 2k + 1 hold variables of different degrees (the host's placement)"""
    import _native
    g = code.tanner_graph()
    cp = np.ascontiguousarray(g.check_ptr, dtype=np.int32)
    vi = np.ascontiguousarray(g.var_idx, dtype=np.int32)
    pos = np.full(g.n, -1, dtype=np.int32)
    host_cells, stats = np.zeros(32, dtype=np.uint8), np.zeros(4, dtype=np.int32)
    rc = _native.load().ldpc_debug_compact_layout(None, g.n, len(cp) - 1, len(vi), _native.ptr(cp), _native.ptr(vi),
                                                  _native.ptr(pos), _native.ptr(host_cells), _native.ptr(stats))
    assert rc == 0 and np.array_equal(host_cells, cells)
    lane_dv = np.full(4 * 512, -1, dtype=np.int64)
    lane_dv[pos] = np.bincount(vi, minlength=g.n)
    rounds = set()
    for w, r in zip(*np.nonzero(cells.reshape(8, 4) == MIXED)):
        d = lane_dv[r * 512 + w * 64: r * 512 + w * 64 + 64].reshape(32, 2)
        if np.any((d[:, 0] != d[:, 1]) & (d.min(axis=1) >= 0)):
            rounds.add(int(r))
    return rounds


def test_the_codes_show_every_cell_kind(gpu_device):
    """what the decode tests below rely on, from the grids the engines report"""
    from ldpc_decoder import BasicMinSumDecoder
    round0, later_uniform, later_kinds, single_round_wave, split = set(), set(), set(), False, set()
    for name in CODES:
        code = make_code(name, 10)
        cells, _ = assert_compact(BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device))
        split |= split_pairs(code, cells)
        grid = cells.reshape(8, 4)
        for w in range(8):
            c0 = int(grid[w, 0])
            if c0 not in (0, MIXED):
                round0.add("low" if (c0 & 0xF) <= 4 else "high")
            for r in (1, 2, 3):
                c = int(grid[w, r])
                if c == 0:
                    later_kinds.add("empty")
                elif c == MIXED:
                    later_kinds.add("mixed")
                elif c & HOLES:
                    later_kinds.add("holes")
                else:
                    later_uniform.add(c)
            single_round_wave |= int(np.count_nonzero(grid[w])) == 1
        if MIXED in grid[:, 0]:
            round0.add("mixed")
    assert round0 == {"low", "high", "mixed"}
    assert later_uniform == {1, 2, 3, 4}
    assert later_kinds == {"empty", "mixed", "holes"}
    assert single_round_wave
    # a mixed cell of round 0 and one of a later round whose degree boundary lies inside a lane pair: a degree read from
    # the neighbouring lane changes a result on these codes, not only on the (1998,1512) code
    assert 0 in split and split & {1, 2, 3}


@pytest.mark.parametrize("T", T_ALL)
@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("kind", ["basic", "rcq", "neural2d"])
def test_decoders_vs_stream_and_oracle(kind, name, T, gpu_device, oracle_mod):
    check_decoder(kind, name, T, gpu_device, oracle_mod)


@pytest.mark.parametrize("kind", ["basic", "rcq", "neural2d"])
def test_flagship_once(kind, gpu_device, oracle_mod):
    check_decoder(kind, "ira", 10, gpu_device, oracle_mod, batches=(5,))


@pytest.mark.parametrize("kind", ["basic", "neural2d"])
def test_two_decodes_in_a_row(kind, gpu_device):
    """nothing of a decode is left in the engine: the second of two decodes with different LLRs equals a fresh engine's"""
    T = 10
    xs = [torch.from_numpy(llrs(70 + k, 5, CODES["odd_round0"][1])).to(gpu_device) for k in range(2)]
    eng, _ = make_decoder(kind, make_code("odd_round0", T), T, gpu_device)
    got = [eng.decode(x, early_stop=False, want_packed=True) for x in xs]
    for x, g in zip(xs, got):
        fresh, _ = make_decoder(kind, make_code("odd_round0", T), T, gpu_device)
        assert fresh is not eng
        same(g, fresh.decode(x, early_stop=False, want_packed=True))
