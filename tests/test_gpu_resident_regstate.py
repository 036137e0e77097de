"""
GPU tests (-m gpu) of the LDS-resident engine's register-resident variable state (ldpc_resident.hip: ResVarState):
fixed-T decodes of codes with n <= 4 * threads per workgroup keep every lane's plan entries and LLRs in registers,
other codes and early-stop decodes keep the streaming variable loop.  Every case is compared bit for bit against the
CPU oracle on codes built to hit the edges of that choice: n not a multiple of 512, waves that mix degrees, variables
of degree 5-8, a row stride that is not a power of two, a code too long for the register form, odd batches.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
POST_TOL = 1e-5


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def balanced_code(seed, dvs, m):
    """H with the given variable degrees; each variable's checks are the least-filled of a random draw, so check
    degrees stay close to E/m (no check is split over lanes)"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(seed)
    n = len(dvs)
    H = np.zeros((m, n), dtype=np.int64)
    deg = np.zeros(m, dtype=np.int64)
    for j in rng.permutation(n):
        cand = rng.permutation(m)
        pick = cand[np.argsort(deg[cand], kind="stable")[:dvs[j]]]
        H[pick, j] = 1
        deg[pick] += 1
    assert deg.max() <= 32
    return LDPCCode(n=n, k=n - m, H=H, max_iterations=8)


def code_mixed_pow2():
    """n = 1700 (not a multiple of 512), m = 480 (row stride 512): 250 variables of degree 5-8 in front, then degrees
    1-3 in random proportions -- waves at the class boundaries mix degrees"""
    rng = np.random.default_rng(3)
    dvs = np.concatenate([rng.integers(5, 9, 250), rng.integers(1, 4, 1450)])
    return balanced_code(30, dvs[rng.permutation(len(dvs))], 480)


def code_mixed_stride():
    """n = 1100, m = 600: row stride m (not a power of two: the final syndrome reads the decisions from the slots)"""
    rng = np.random.default_rng(4)
    return balanced_code(40, rng.integers(2, 7, 1100), 600)


def code_long():
    """n = 4500: more than four variables per lane at any workgroup size -> the streaming variable loop"""
    rng = np.random.default_rng(5)
    return balanced_code(50, rng.integers(2, 4, 4500), 1500)


def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32)


def llrs(rng, B, n):
    """a mix of converging and non-converging codewords"""
    x = np.concatenate([awgn(rng, B - B // 2, n, 1.0), awgn(rng, B // 2, n, 5.0)])
    return x[rng.permutation(B)]


def rand_weights(dec, rng):
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    return ({k: float(v.item()) for k, v in dec.beta_weights.items()},
            {k: float(v.item()) for k, v in dec.alpha_weights.items()})


def assert_post(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    assert np.all(err <= POST_TOL * np.maximum(1.0, np.abs(b))), f"posterior max err {err.max()}"


def host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


CODES = {"mixed_pow2": code_mixed_pow2, "mixed_stride": code_mixed_stride, "long": code_long}


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_basic_and_rcq_vs_oracle(name, early_stop, B, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    code = CODES[name]()
    og = oracle_mod.OracleGraph(code.H)
    rng = np.random.default_rng(B)
    llr = llrs(rng, B, code.n)
    x = torch.from_numpy(llr).to(gpu_device)
    dec = BasicMinSumDecoder(code)
    bits, succ, iters = dec.decode(x, early_stop=early_stop)
    ob, _, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, 8, early_stop=early_stop, dtype=np.float32)
    np.testing.assert_array_equal(host(iters), oi)
    np.testing.assert_array_equal(host(succ), os_)
    np.testing.assert_array_equal(host(bits), ob)
    bits, succ, iters = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=8).decode(x, early_stop=early_stop)
    ob, _, oi, os_ = oracle_mod.rcq(og, llr, 3, QP, 8, early_stop=early_stop)
    np.testing.assert_array_equal(host(iters), oi)
    np.testing.assert_array_equal(host(succ), os_)
    np.testing.assert_array_equal(host(bits), ob)


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("early_stop", [False, True])
@pytest.mark.parametrize("wtype", [1, 2])
def test_neural2d_posterior_vs_oracle(name, early_stop, wtype, gpu_device, oracle_mod):
    """posterior on (Neural-2D returns it) with per-variable alpha columns (type 1) and one alpha per degree (type 2)"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = CODES[name]()
    og = oracle_mod.OracleGraph(code.H)
    rng = np.random.default_rng(11 + wtype)
    llr = llrs(rng, 33, code.n)
    x = torch.from_numpy(llr).to(gpu_device)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=8)
    beta, alpha = rand_weights(dec, rng)
    bits, post, iters = dec(x, early_stop=early_stop)
    ob, op, oi, _ = oracle_mod.neural2d(og, llr, wtype, 8, beta, alpha, early_stop=early_stop)
    np.testing.assert_array_equal(host(iters), oi)
    np.testing.assert_array_equal(host(bits), ob)
    assert_post(host(post), op)


@pytest.mark.parametrize("name", sorted(CODES))
@pytest.mark.parametrize("early_stop", [False, True])
def test_basic_fp64_vs_oracle(name, early_stop, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = CODES[name]()
    og = oracle_mod.OracleGraph(code.H)
    rng = np.random.default_rng(21)
    llr = llrs(rng, 9, code.n).astype(np.float64)
    bits, succ, iters = BasicMinSumDecoder(code).decode(torch.from_numpy(llr).to(gpu_device), early_stop=early_stop)
    ob, _, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, 8, early_stop=early_stop)
    np.testing.assert_array_equal(host(iters), oi)
    np.testing.assert_array_equal(host(succ), os_)
    np.testing.assert_array_equal(host(bits), ob)


def test_codes_take_the_resident_engine(gpu_device):
    """the cases above exercise the LDS-resident engine, not a streaming fallback"""
    from ldpc_decoder import BasicMinSumDecoder
    for name, make in CODES.items():
        dec = BasicMinSumDecoder(make())
        assert dec._engine(torch.float32, gpu_device).info()["engine"] == "resident"
        if name != "long":      # the fp64 engine needs two 8-byte slots per edge in 16-bit offsets: too many for "long"
            assert dec._engine(torch.float64, gpu_device).info()["engine"] == "resident"
