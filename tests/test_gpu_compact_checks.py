"""
GPU tests (-m gpu) of the scalar-counted check phase of the compact fixed-T kernel (resident_decode<..., CPT>,
res_check_body_uniform): a wave runs d_lo edges of every check on a scalar trip count -- groups of four and a tail of
d_lo & 3 -- and only the lanes of higher degree go on under a lane mask; a wave with d_lo < 4 keeps the per-lane form
(ldpc_debug_compact_checks reports the table).  Codes are built from lists of CHECK degrees so that every branch runs:
waves of one degree, spreads of 1 and of 3, every value of d_lo & 3, a partly filled and an empty last wave, waves
that fall back.  Basic, Neural-2D type 2 (one beta per check degree) and RCQ decodes are compared with the streaming
engine bit for bit in every output, and with the CPU oracle; a decoder with per-edge beta (type 1) keeps the per-lane
form in every wave.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
POST_TOL = 1e-5
PER_LANE = 1 << 31


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


# name: (seed, n, check degrees in any order -- the plan sorts them descending, 64 to a wave)
CODES = {
    # seven full waves of degree 8 (d_lo & 3 = 0), the eighth empty
    "uniform": (21, 1200, [8] * 448),
    # 13 (tail 1) | 11 (tail 3) | 9, 8, 7, 6 (d_lo 6: tail 2, spread 3) | 6, 5 (tail 1, spread 1) | 20 lanes of 4 (tail 0)
    "tails": (22, 900, [13] * 64 + [11] * 64 + [9, 8, 7, 6] * 16 + [6] * 32 + [5] * 32 + [4] * 20),
    # degree 8 | 8 .. 3 in one wave, then 3, 2 and 1: d_lo < 4, the per-lane form (with its degree-1 rule)
    "fallback": (23, 400, [8] * 96 + [5] * 20 + [3] * 40 + [2] * 24 + [1] * 12),
}
# (d_lo, spread, lanes, per-lane) of waves 0..7 as the comment above says
TABLES = {
    "uniform": [(8, 0, 64, False)] * 7 + [(0, 0, 0, False)],
    "tails": [(13, 0, 64, False), (11, 0, 64, False), (6, 3, 64, False), (5, 1, 64, False), (4, 0, 20, False)]
             + [(0, 0, 0, False)] * 3,
    "fallback": [(8, 0, 64, False), (3, 5, 64, True), (1, 2, 64, True)] + [(0, 0, 0, False)] * 5,
    "ira": [(14, 0, 64, False)] * 4 + [(13, 1, 64, False)] + [(13, 0, 64, False)] * 2 + [(13, 0, 38, False)],
}


def code_from_check_degrees(seed, n, dcs, T):
    """every check on the dc variables of lowest current degree (random tie break): variable degrees stay within one"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(seed)
    m = len(dcs)
    H = np.zeros((m, n), dtype=np.int64)
    deg = np.zeros(n, dtype=np.int64)
    for i in rng.permutation(m):
        cand = rng.permutation(n)
        pick = cand[np.argsort(deg[cand], kind="stable")[:dcs[i]]]
        H[i, pick] = 1
        deg[pick] += 1
    assert deg.min() >= 1 and deg.max() <= 8
    return LDPCCode(n=n, k=n - m, H=H, max_iterations=T)


def make_code(name, T=10):
    if name == "ira":
        import codes
        return codes.load_code("ira_1998_1512", max_iterations=T)
    seed, n, dcs = CODES[name]
    return code_from_check_degrees(seed, n, dcs, T)


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


def table_of(eng):
    import _native
    info = eng.info()
    assert info["engine"] == "resident" and info["threads_per_workgroup"] == 512 and info["workgroups_per_cu"] >= 3
    words = np.zeros(8, dtype=np.uint32)
    rc = eng._lib.ldpc_debug_compact_checks(eng.handle, 0, 0, 0, None, None, _native.ptr(words))
    assert rc == 0, "the engine has no compact plan"
    got = [(int(w) & 0xFF, int(w) >> 8 & 0xFF, int(w) >> 16 & 0xFF, bool(int(w) & PER_LANE)) for w in words]
    assert info["compact_plan"]["scalar_check_waves"] == sum(1 for g in got if g[2] and not g[3])
    return got


def assert_table(eng, name):
    """the engine decodes on the compact plan, and its check table holds the branches the code was built for"""
    assert table_of(eng) == TABLES[name]


def assert_same_as_stream(eng, x, **kw):
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


def test_the_codes_cover_every_branch():
    """host side of the case list: tails 0..3, spreads 0, 1 and >= 3, a partial and an empty wave, a fallback wave"""
    waves = [w for name in CODES for w in TABLES[name]]
    scalar = [w for w in waves if w[2] and not w[3]]
    assert {w[0] & 3 for w in scalar} == {0, 1, 2, 3}
    assert {0, 1} <= {w[1] for w in scalar} and any(w[1] >= 3 for w in scalar)
    assert any(0 < w[2] < 64 for w in scalar) and any(w[2] == 0 for w in waves) and any(w[3] for w in waves)
    assert all(w[1] == 0 for w in TABLES["uniform"])


@pytest.mark.parametrize("name", ["uniform", "tails", "fallback", "ira"])
@pytest.mark.parametrize("T", [1, 10])
def test_basic(name, T, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = make_code(name, T)
    llr = llrs(50 + T, 37, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    assert_table(eng, name)
    res = assert_same_as_stream(eng, torch.from_numpy(llr).to(gpu_device))
    ob, op, oi, os_ = oracle_mod.basic_minsum(oracle_graph(oracle_mod, code), llr, 0.7, T, early_stop=False,
                                              dtype=np.float32)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert_post(res.posterior.cpu().numpy(), op)


@pytest.mark.parametrize("name", ["uniform", "tails", "fallback", "ira"])
def test_neural2d_per_check_beta(name, gpu_device, oracle_mod):
    """sharing type 2: one beta per check degree and iteration, read per check (b_pre)"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = make_code(name)
    rng = np.random.default_rng(60)
    llr = llrs(61, 33, code.n)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=10)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    x = torch.from_numpy(llr).to(gpu_device)
    bits, post, iters = dec(x, early_stop=False)
    eng = dec._get_engine(gpu_device)
    assert_table(eng, name)
    res = assert_same_as_stream(eng, x)
    assert torch.equal(res.bits, bits) and torch.equal(res.posterior, post)
    ob, op, oi, _ = oracle_mod.neural2d(oracle_graph(oracle_mod, code), llr, 2, 10, beta, alpha, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    assert_post(post.cpu().numpy(), op)


@pytest.mark.parametrize("name", ["uniform", "tails", "fallback", "ira"])
@pytest.mark.parametrize("T", [1, 10])
def test_rcq(name, T, gpu_device, oracle_mod):
    from rcq_decoder import RCQMinSumDecoder
    code = make_code(name, T)
    llr = llrs(70 + T, 21, code.n)
    dec = RCQMinSumDecoder(code, 3, 8, QP, T)
    eng = dec._get_engine(gpu_device)
    assert_table(eng, name)
    x = torch.from_numpy(llr).to(gpu_device)
    assert_same_as_stream(eng, x)
    bits, succ, iters = dec.decode(x, early_stop=False)
    ob, _, oi, os_ = oracle_mod.rcq(oracle_graph(oracle_mod, code), llr, 3, QP, T, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.cpu().numpy(), os_)


def test_per_edge_beta_keeps_the_per_lane_form(gpu_device, oracle_mod):
    """sharing type 1 (one beta per edge position): not the select form, so the decoder's table marks every wave"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = make_code("tails")
    rng = np.random.default_rng(80)
    llr = llrs(81, 19, code.n)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=1, max_iterations=10)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    x = torch.from_numpy(llr).to(gpu_device)
    bits, post, iters = dec(x, early_stop=False)
    eng = dec._get_engine(gpu_device)
    got = table_of(eng)
    assert [g[:3] for g in got] == [t[:3] for t in TABLES["tails"]]
    assert all(g[3] for g in got if g[2]) and eng.info()["compact_plan"]["scalar_check_waves"] == 0
    assert_same_as_stream(eng, x)
    ob, op, oi, _ = oracle_mod.neural2d(oracle_graph(oracle_mod, code), llr, 1, 10, beta, alpha, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    assert_post(post.cpu().numpy(), op)
