"""
GPU tests (-m gpu) of the compact fixed-T kernel (resident_decode<..., CPT>) on its balanced variable grid: the host
places variables at q = r*512 + w*64 + lane so that most (wave, round) cells hold one degree, and each wave branches on
its cells' degrees (ldpc_debug_compact_layout reports the grid).  Codes built to force mixed cells, cells with empty
lanes, a degree-1 variable and degree 5-8 variables over several waves, next to the (1998,1512) code, are decoded by
Basic, RCQ and Neural-2D (posterior; per-variable alpha columns) at T = 0, 1 and 10, odd batches and capped decodes:
bits, iterations and success equal the CPU oracle, and every output equals the streaming engine's bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
POST_TOL = 1e-5
LDS_THIRD = 160 * 1024 // 3
MIXED, HOLES = 0xFF, 0x40


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def random_code(seed, n, m, census, T):
    """variables of the census' degrees, each on the dv checks of lowest current degree (random tie break)"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(seed)
    dv_seq = rng.permutation(np.repeat(list(census), list(census.values())))
    assert len(dv_seq) == n
    H = np.zeros((m, n), dtype=np.int64)
    deg = np.zeros(m, dtype=np.int64)
    for j, d in enumerate(dv_seq):
        cand = rng.permutation(m)
        pick = cand[np.argsort(deg[cand], kind="stable")[:d]]
        H[pick, j] = 1
        deg[pick] += 1
    return LDPCCode(n=n, k=n - m, H=H, max_iterations=T)


CODES = {
    # dv 5-8 over four waves, partial cells of every degree, a lone dv 4 and 49 dv 1 (mixed cells)
    "spread": (11, 1200, 400, {7: 150, 5: 100, 6: 80, 8: 20, 3: 500, 2: 300, 1: 49, 4: 1}),
    # 512 degree > 4 variables: all eight round-0 cells, two degrees in one of them
    "full_round0": (12, 2000, 490, {8: 100, 6: 412, 3: 300, 2: 1100, 1: 88}),
}


def make_code(name, T=10):
    if name == "ira":
        import codes
        return codes.load_code("ira_1998_1512", max_iterations=T)
    seed, n, m, census = CODES[name]
    return random_code(seed, n, m, census, T)


def oracle_graph(oracle_mod, code):
    g = code.tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


def llrs(seed, B, n):
    rng = np.random.default_rng(seed)
    out = []
    for snr in (1.0, 3.0):
        s2 = 10.0 ** (-snr / 10.0)
        out.append((2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32))
    x = np.concatenate([out[0][: B - B // 2], out[1][: B // 2]])
    return x[rng.permutation(B)]


def grid_of(eng):
    import _native
    cells = np.zeros(32, dtype=np.uint8)
    stats = np.zeros(4, dtype=np.int32)
    rc = eng._lib.ldpc_debug_compact_layout(eng.handle, 0, 0, 0, None, None, None, _native.ptr(cells),
                                            _native.ptr(stats))
    assert rc == 0, "the engine has no compact plan"
    return cells, stats


def assert_compact(eng):
    info = eng.info()
    assert info["engine"] == "resident" and info["threads_per_workgroup"] == 512
    assert info["lds_bytes"] <= LDS_THIRD and info["workgroups_per_cu"] == 3
    return grid_of(eng)


def assert_same_as_stream(eng, x, **kw):
    """the compact fixed-T decode against the streaming engine, every output bit for bit"""
    eng.set_mode("auto")
    a = eng.decode(x, early_stop=False, want_packed=True, **kw)
    eng.set_mode("stream")
    b = eng.decode(x, early_stop=False, want_packed=True, **kw)
    eng.set_mode("auto")
    for f in ("bits", "posterior", "iterations", "success", "packed_bits"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    return a


def assert_post(a, b):
    err = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    assert np.all(err <= POST_TOL * np.maximum(1.0, np.abs(b))), f"posterior max err {err.max()}"


def test_the_test_codes_force_every_cell_kind(gpu_device):
    from ldpc_decoder import BasicMinSumDecoder
    kinds = set()
    for name in CODES:
        cells, _ = assert_compact(BasicMinSumDecoder(make_code(name), 0.7)._engine(torch.float32, gpu_device))
        kinds |= {"mixed" if c == MIXED else "holes" if c & HOLES else "uniform" if c else "empty" for c in cells}
    assert {"mixed", "holes", "uniform"} <= kinds


@pytest.mark.parametrize("name", ["ira", "spread", "full_round0"])
@pytest.mark.parametrize("T", [0, 1, 10])
def test_basic_vs_oracle(name, T, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = make_code(name, T)
    llr = llrs(10 + T, 37, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    assert_compact(eng)
    res = assert_same_as_stream(eng, torch.from_numpy(llr).to(gpu_device))
    ob, op, oi, os_ = oracle_mod.basic_minsum(oracle_graph(oracle_mod, code), llr, 0.7, T, early_stop=False,
                                              dtype=np.float32)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert_post(res.posterior.cpu().numpy(), op)


@pytest.mark.parametrize("name", ["spread", "full_round0"])
def test_basic_capped_vs_oracle(name, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = make_code(name)
    llr = llrs(20, 29, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    og = oracle_graph(oracle_mod, code)
    x = torch.from_numpy(llr).to(gpu_device)
    for c in (1, 6):
        res = assert_same_as_stream(eng, x, max_iters=c)
        ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, c, early_stop=False, dtype=np.float32)
        np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
        np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
        np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
        assert_post(res.posterior.cpu().numpy(), op)


@pytest.mark.parametrize("name", ["spread", "full_round0"])
@pytest.mark.parametrize("T", [1, 10])
def test_rcq_vs_oracle(name, T, gpu_device, oracle_mod):
    from rcq_decoder import RCQMinSumDecoder
    code = make_code(name, T)
    llr = llrs(30 + T, 21, code.n)
    dec = RCQMinSumDecoder(code, 3, 8, QP, T)
    eng = dec._get_engine(gpu_device)
    assert_compact(eng)
    assert_same_as_stream(eng, torch.from_numpy(llr).to(gpu_device))
    bits, succ, iters = dec.decode(torch.from_numpy(llr).to(gpu_device), early_stop=False)
    ob, _, oi, os_ = oracle_mod.rcq(oracle_graph(oracle_mod, code), llr, 3, QP, T, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.cpu().numpy(), os_)


@pytest.mark.parametrize("name", ["spread", "full_round0"])
@pytest.mark.parametrize("wtype", [1, 2])
def test_neural2d_posterior_vs_oracle(name, wtype, gpu_device, oracle_mod):
    """alpha columns read through vmeta (type 1: one column per variable)"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = make_code(name)
    rng = np.random.default_rng(40 + wtype)
    llr = llrs(41, 33, code.n)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=10)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    x = torch.from_numpy(llr).to(gpu_device)
    bits, post, iters = dec(x, early_stop=False)
    eng = dec._get_engine(gpu_device)
    assert_compact(eng)
    assert_same_as_stream(eng, x)
    ob, op, oi, _ = oracle_mod.neural2d(oracle_graph(oracle_mod, code), llr, wtype, 10, beta, alpha, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    assert_post(post.cpu().numpy(), op)


def test_info_reports_the_grid(gpu_device):
    from ldpc_decoder import BasicMinSumDecoder
    eng = BasicMinSumDecoder(make_code("ira"), 0.7)._engine(torch.float32, gpu_device)
    plan = eng.info()["compact_plan"]
    _, stats = grid_of(eng)
    assert plan["worst_wave_cost"] == stats[1] and plan["mixed_cells"] == stats[3]
    assert plan["mean_wave_cost"] == pytest.approx(stats[2] / 8)
