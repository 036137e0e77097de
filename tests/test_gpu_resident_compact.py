"""
GPU tests (-m gpu) of the compact fixed-T geometry of the LDS-resident engine (ldpc_resident.hip: resident_decode<..., CPT>):
fixed-iteration fp32 decodes of codes with m <= 496 whose message slots fit 54,613 bytes run three 512-thread workgroups
per CU -- row stride 496, no llr_s / bits_s / parity words / alpha table in LDS.  Early-stop and float64 decodes and codes
that do not fit keep the general geometry.  Every case is compared bit for bit against the CPU oracle on the (1998,1512)
code: Basic, RCQ and Neural-2D (posterior, bits, packed bits), odd batches and batches below three workgroups per CU,
T = 0 and 1, capped decodes.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
POST_TOL = 1e-5
LDS_THIRD = 160 * 1024 // 3          # bytes per workgroup at three workgroups per CU


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


def ira(T=10):
    import codes
    return codes.load_code("ira_1998_1512", max_iterations=T)


def oracle_graph(oracle_mod, code):
    g = code.tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32)


def llrs(rng, B, n):
    """a mix of converging and non-converging codewords"""
    x = np.concatenate([awgn(rng, B - B // 2, n, 1.5), awgn(rng, B // 2, n, 3.5)])
    return x[rng.permutation(B)]


def assert_post(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    assert np.all(err <= POST_TOL * np.maximum(1.0, np.abs(b))), f"posterior max err {err.max()}"


def unpack(packed, B, n):
    return ((packed.cpu().numpy()[:, :, None] >> np.arange(8)) & 1).reshape(B, -1)[:, :n]


def test_flagship_code_takes_the_compact_geometry(gpu_device):
    from ldpc_decoder import BasicMinSumDecoder
    dec = BasicMinSumDecoder(ira(), 0.7)
    info = dec._engine(torch.float32, gpu_device).info()
    assert info["engine"] == "resident"
    assert info["codewords_per_workgroup"] == 2 and info["threads_per_workgroup"] == 512
    assert info["lds_bytes"] <= LDS_THIRD and info["workgroups_per_cu"] == 3
    # float64 keeps the general geometry (one codeword in a float pair's slots, two workgroups per CU)
    info64 = dec._engine(torch.float64, gpu_device).info()
    assert info64["engine"] == "resident" and info64["workgroups_per_cu"] == 2


def test_code_that_does_not_fit_keeps_the_general_geometry(gpu_device, oracle_mod):
    """m = 600 > 496: the row stride of the compact layout cannot hold it; fixed-T decodes stay on the general kernel
    (which, at row stride m, fits three workgroups per CU of its own for this small code)"""
    from ldpc_decoder import BasicMinSumDecoder, LDPCCode
    rng = np.random.default_rng(4)
    n, m = 1100, 600
    H = np.zeros((m, n), dtype=np.int64)
    deg = np.zeros(m, dtype=np.int64)
    for j, dv in enumerate(rng.integers(2, 7, n)):
        cand = rng.permutation(m)
        pick = cand[np.argsort(deg[cand], kind="stable")[:dv]]
        H[pick, j] = 1
        deg[pick] += 1
    code = LDPCCode(n=n, k=n - m, H=H, max_iterations=8)
    dec = BasicMinSumDecoder(code)
    info = dec._engine(torch.float32, gpu_device).info()
    # the general carve holds every message slot AND the LLR rows (llr_s); the compact one only the slots
    assert info["engine"] == "resident" and info["lds_bytes"] >= 8 * (int(H.sum()) + n)
    llr = llrs(rng, 9, n)
    bits, succ, iters = dec.decode(torch.from_numpy(llr).to(gpu_device), early_stop=False)
    ob, _, oi, os_ = oracle_mod.basic_minsum(oracle_mod.OracleGraph(H), llr, 0.7, 8, early_stop=False, dtype=np.float32)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.cpu().numpy(), os_)


@pytest.mark.parametrize("B", [1, 7, 255, 1537])
def test_basic_posterior_bits_packed_vs_oracle(B, gpu_device, oracle_mod):
    """B = 1, 7, 255: fewer workgroups than three per CU; 1537: one past a full wave of 768 workgroups, odd"""
    from ldpc_decoder import BasicMinSumDecoder
    code = ira()
    rng = np.random.default_rng(100 + B)
    llr = llrs(rng, B, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    res = eng.decode(torch.from_numpy(llr).to(gpu_device), early_stop=False, want_packed=True)
    ob, op, oi, os_ = oracle_mod.basic_minsum(oracle_graph(oracle_mod, code), llr, 0.7, 10, early_stop=False,
                                              dtype=np.float32)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert_post(res.posterior.cpu().numpy(), op)
    np.testing.assert_array_equal(unpack(res.packed_bits, B, code.n), ob)


@pytest.mark.parametrize("B", [3, 130])
def test_rcq_vs_oracle(B, gpu_device, oracle_mod):
    from rcq_decoder import RCQMinSumDecoder
    code = ira()
    rng = np.random.default_rng(200 + B)
    llr = llrs(rng, B, code.n)
    bits, succ, iters = RCQMinSumDecoder(code, 3, 8, QP, 10).decode(torch.from_numpy(llr).to(gpu_device),
                                                                     early_stop=False)
    ob, _, oi, os_ = oracle_mod.rcq(oracle_graph(oracle_mod, code), llr, 3, QP, 10, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    np.testing.assert_array_equal(succ.cpu().numpy(), os_)


@pytest.mark.parametrize("wtype", [1, 2])
def test_neural2d_posterior_vs_oracle(wtype, gpu_device, oracle_mod):
    """alpha read from global memory (per-variable columns for type 1), posterior staged through the dead slots"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = ira()
    rng = np.random.default_rng(300 + wtype)
    llr = llrs(rng, 33, code.n)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=wtype, max_iterations=10)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    bits, post, iters = dec(torch.from_numpy(llr).to(gpu_device), early_stop=False)
    ob, op, oi, _ = oracle_mod.neural2d(oracle_graph(oracle_mod, code), llr, wtype, 10, beta, alpha, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    assert_post(post.cpu().numpy(), op)


@pytest.mark.parametrize("T", [0, 1])
def test_zero_and_one_iteration(T, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = ira(T)
    rng = np.random.default_rng(400 + T)
    llr = llrs(rng, 65, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    assert eng.info()["workgroups_per_cu"] == 3
    res = eng.decode(torch.from_numpy(llr).to(gpu_device), early_stop=False)
    ob, op, oi, os_ = oracle_mod.basic_minsum(oracle_graph(oracle_mod, code), llr, 0.7, T, early_stop=False,
                                              dtype=np.float32)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert_post(res.posterior.cpu().numpy(), op)


def test_capped_decodes_vs_oracle(gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = ira()
    rng = np.random.default_rng(500)
    llr = llrs(rng, 41, code.n)
    x = torch.from_numpy(llr).to(gpu_device)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    og = oracle_graph(oracle_mod, code)
    for c in (1, 4, 9):
        res = eng.decode(x, early_stop=False, max_iters=c, want_packed=True)
        ob, op, oi, os_ = oracle_mod.basic_minsum(og, llr, 0.7, c, early_stop=False, dtype=np.float32)
        np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
        np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
        np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
        assert_post(res.posterior.cpu().numpy(), op)
        np.testing.assert_array_equal(unpack(res.packed_bits, len(llr), code.n), ob)


def test_compact_and_general_kernels_agree_with_early_stop_off_and_on(gpu_device):
    """the fixed-T compact decode equals the streaming engine bit for bit; an early-stop decode of the same engine
    (general geometry) still runs and agrees with the streaming engine too"""
    from ldpc_decoder import BasicMinSumDecoder
    code = ira()
    rng = np.random.default_rng(600)
    x = torch.from_numpy(llrs(rng, 200, code.n)).to(gpu_device)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    for early in (False, True):
        eng.set_mode("auto")
        a = eng.decode(x, early_stop=early, want_packed=True)
        eng.set_mode("stream")
        b = eng.decode(x, early_stop=early, want_packed=True)
        eng.set_mode("auto")
        for f in ("bits", "posterior", "iterations", "success", "packed_bits"):
            assert torch.equal(getattr(a, f), getattr(b, f)), (early, f)
