"""
GPU tests (-m gpu) of the entry and exit of the compact fixed-T kernels (ldpc_resident.hip: resident_decode<..., CPT>):
the unbounded forms a full block takes (both codewords of the workgroup exist, n > 3 * 512) against the per-element
forms of the padded last block and of shorter codes, the init scatter on the scalar cell degree, the final syndrome's
scalar-counted walk and the output pass specialised for what was asked for.

Every case is compared with the CPU oracle: bits, iterations and success equal, posterior within POST_TOL, unpacked
packed bits equal to the bits.  Two codes: the (1998,1512) code (a partial last variable wave: 1998 = 31 * 64 + 14,
cells with holes, one mixed cell, variables of degree > 4), a generated (700,400) code of variable degrees 2-4
(n <= 3 * 512: the generic row loops, no upper offset half, empty rounds) and a generated (1700,1250) code, whose last
row of 512 positions holds two full waves, one partial wave (1700 = 1536 + 2 * 64 + 36) and five waves that lie wholly
past the row's end.  Batches 1 (only the padded block), 2 (one full block), 3 (both in one launch) and 5.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
POST_TOL = 1e-5
FACTOR = 0.7
CODES = ("ira", "small", "mid")
GENERATED = {"small": (700, 300, 18), "mid": (1700, 450, 19)}      # n, m, seed
OUTPUTS = {                      # want_bits, want_posterior, want_packed
    "bits": (True, False, False),            # what the benchmark's flagship decode asks for
    "posterior": (False, True, False),
    "packed": (False, False, True),
    "all": (True, True, True),
    "none": (False, False, False),           # iterations and success only
}


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


@functools.lru_cache(maxsize=None)
def gen_H(name):
    """variable degrees 2-4, checks filled evenly"""
    n, m, seed = GENERATED[name]
    rng = np.random.default_rng(seed)
    H = np.zeros((m, n), dtype=np.int64)
    deg = np.zeros(m, dtype=np.int64)
    for j, dv in enumerate(rng.integers(2, 5, n)):
        cand = rng.permutation(m)
        pick = cand[np.argsort(deg[cand], kind="stable")[:dv]]
        H[pick, j] = 1
        deg[pick] += 1
    H.setflags(write=False)
    return H


def make_code(name, T=10):
    if name == "ira":
        import codes
        return codes.load_code("ira_1998_1512", max_iterations=T)
    from ldpc_decoder import LDPCCode
    H = gen_H(name)
    return LDPCCode(n=H.shape[1], k=H.shape[1] - H.shape[0], H=np.array(H), max_iterations=T)


def oracle_graph(oracle_mod, name, code):
    if name in GENERATED:
        return oracle_mod.OracleGraph(np.array(gen_H(name)))
    g = code.tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32)


@functools.lru_cache(maxsize=None)
def llrs(name, B, seed=0):
    """converging and non-converging codewords side by side, so that success differs inside a workgroup's pair"""
    n = 1998 if name == "ira" else GENERATED[name][0]
    rng = np.random.default_rng(1800 + 10 * B + seed)
    lo, hi = {"ira": (1.5, 5.5), "small": (-1.0, 4.0), "mid": (1.5, 6.5)}[name]   # dB: fails / converges in 10 iterations
    x = np.stack([awgn(rng, 1, n, hi if (b & 1) else lo)[0] for b in range(B)])
    x.setflags(write=False)
    return x


_REF = {}


def basic_ref(oracle_mod, name, B, T=10, seed=0):
    """(bits, posterior, iterations, success) of the CPU oracle, computed once per case"""
    key = (name, B, T, seed)
    if key not in _REF:
        code = make_code(name, T)
        _REF[key] = oracle_mod.basic_minsum(oracle_graph(oracle_mod, name, code), np.array(llrs(name, B, seed)), FACTOR, T,
                                            early_stop=False, dtype=np.float32)
    return _REF[key]


def basic_engine(name, dev, T=10):
    from ldpc_decoder import BasicMinSumDecoder
    return BasicMinSumDecoder(make_code(name, T), FACTOR)._engine(torch.float32, dev)


def assert_post(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    err = np.abs(a - b)
    assert np.all(err <= POST_TOL * np.maximum(1.0, np.abs(b))), f"posterior max err {err.max()}"


def unpack(packed, B, n):
    return ((packed.cpu().numpy()[:, :, None] >> np.arange(8)) & 1).reshape(B, -1)[:, :n]


def check(res, ref, B, n, outputs="all"):
    """everything the decode was asked for against the oracle's (bits, posterior, iterations, success)"""
    ob, op, oi, os_ = ref
    want_bits, want_post, want_packed = OUTPUTS[outputs]
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert (res.bits is not None) == want_bits and (res.posterior is not None) == want_post
    assert (res.packed_bits is not None) == want_packed
    if want_bits:
        np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    if want_post:
        assert_post(res.posterior.cpu().numpy(), op)
    if want_packed:
        pk = res.packed_bits.cpu().numpy()
        assert pk.shape == (B, (n + 7) // 8)
        np.testing.assert_array_equal(unpack(res.packed_bits, B, n), ob)
        if n % 8:
            assert not np.any(pk[:, -1] >> (n % 8)), "bits past the row's end in the last packed byte"


def decode(eng, x, dev, outputs="all", **kw):
    want_bits, want_post, want_packed = OUTPUTS[outputs]
    return eng.decode(torch.from_numpy(np.array(x)).to(dev), early_stop=False, want_bits=want_bits, want_posterior=want_post,
                      want_packed=want_packed, **kw)


@pytest.mark.parametrize("name", CODES)
def test_both_codes_run_the_compact_kernel(name, gpu_device):
    info = basic_engine(name, gpu_device).info()
    assert info["engine"] == "resident" and info["threads_per_workgroup"] == 512
    # three workgroups per CU by the flagship's LDS carve; a smaller carve admits the four the wave slots allow
    assert info["codewords_per_workgroup"] == 2 and info["workgroups_per_cu"] in (3, 4)
    k = info["resident_kernel"]["fixed_T"]
    assert k["plan"] == "compact" and k["form"] == "NMS" and k["bpc"] and k["ms"] == 495
    n = make_code(name).n
    assert {"ira": n == 1998, "small": n <= 3 * 512, "mid": 3 * 512 + 64 < n <= 4 * 512 - 128}[name]


@pytest.mark.parametrize("B", [1, 2, 3, 5])
@pytest.mark.parametrize("name", CODES)
def test_batches_vs_oracle(name, B, gpu_device, oracle_mod):
    """1: only the padded block; 2: one full block; 3 and 5: full blocks and the padded one in one launch"""
    eng = basic_engine(name, gpu_device)
    res = decode(eng, llrs(name, B), gpu_device)
    check(res, basic_ref(oracle_mod, name, B), B, eng.graph.n)
    if B >= 2:
        ok = basic_ref(oracle_mod, name, B)[3]
        assert ok.any() and not ok.all(), "the case is meant to hold decodes that succeed and decodes that fail"


@pytest.mark.parametrize("outputs", list(OUTPUTS))
@pytest.mark.parametrize("name", CODES)
def test_every_output_combination_vs_oracle(name, outputs, gpu_device, oracle_mod):
    eng = basic_engine(name, gpu_device)
    res = decode(eng, llrs(name, 3), gpu_device, outputs)
    check(res, basic_ref(oracle_mod, name, 3), 3, eng.graph.n, outputs)


@pytest.mark.parametrize("outputs", ["bits", "all"])
@pytest.mark.parametrize("T", [0, 1])
@pytest.mark.parametrize("name", CODES)
def test_zero_and_one_iteration_vs_oracle(name, T, outputs, gpu_device, oracle_mod):
    eng = basic_engine(name, gpu_device, T)
    assert eng.info()["resident_kernel"]["fixed_T"]["plan"] == "compact"
    res = decode(eng, llrs(name, 3), gpu_device, outputs)
    check(res, basic_ref(oracle_mod, name, 3, T), 3, eng.graph.n, outputs)


@pytest.mark.parametrize("name", CODES)
def test_neural2d_type2_vs_oracle(name, gpu_device, oracle_mod):
    """alpha != 1: the instantiation's variable phase multiplies; entry and exit are the shared ones"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = make_code(name)
    rng = np.random.default_rng(1820)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=10)
    for p in dec.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.5, 1.0))))
    for p in dec.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.8, 1.2))))
    beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
    alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
    eng = dec._get_engine(gpu_device)
    k = eng.info()["resident_kernel"]["fixed_T"]
    assert k["plan"] == "compact" and not k["unit_alpha"]
    x = np.array(llrs(name, 3, seed=1))
    res = decode(eng, x, gpu_device)
    ob, op, oi, os_ = oracle_mod.neural2d(oracle_graph(oracle_mod, name, code), x, 2, 10, beta, alpha, early_stop=False)
    check(res, (ob, op, oi, os_), 3, code.n)


@pytest.mark.parametrize("name", CODES)
def test_rcq_vs_oracle(name, gpu_device, oracle_mod):
    from rcq_decoder import RCQMinSumDecoder
    code = make_code(name)
    dec = RCQMinSumDecoder(code, 3, 8, QP, 10)
    eng = dec._get_engine(gpu_device)
    k = eng.info()["resident_kernel"]["fixed_T"]
    assert k["plan"] == "compact" and k["form"] == "RCQ"
    x = np.array(llrs(name, 3, seed=2))
    res = decode(eng, x, gpu_device)
    ref = oracle_mod.rcq(oracle_graph(oracle_mod, name, code), x, 3, QP, 10, early_stop=False)
    check(res, ref, 3, code.n)


@pytest.mark.parametrize("name", CODES)
def test_a_decode_does_not_depend_on_what_the_buffers_held(name, gpu_device, oracle_mod):
    """The engine allocates its outputs uninitialised.  Blocks of the outputs' sizes are filled with junk and released
    to the caching allocator, then an engine that has just decoded a batch of 5 decodes a batch of 3 into those very
    blocks (asserted): every element of every output must be written (fast forms) and nothing beyond the rows (the
    padded block's missing codeword), so the results equal a fresh engine's and the oracle's."""
    n = make_code(name).n
    x3 = torch.from_numpy(np.array(llrs(name, 3, seed=3))).to(gpu_device)
    used = basic_engine(name, gpu_device)
    check(decode(used, llrs(name, 5), gpu_device), basic_ref(oracle_mod, name, 5), 5, n)
    junk = [torch.full((3, n), -1, dtype=torch.int32, device=gpu_device),
            torch.full((3, n), float("nan"), dtype=torch.float32, device=gpu_device),
            torch.full((3, (n + 7) // 8), 0xFF, dtype=torch.uint8, device=gpu_device),
            torch.full((3,), -1, dtype=torch.int32, device=gpu_device),
            torch.full((3,), 0xFF, dtype=torch.uint8, device=gpu_device)]
    torch.cuda.synchronize()
    held = {t.data_ptr() for t in junk}
    del junk
    a = used.decode(x3, early_stop=False, want_packed=True)
    got = {a.bits.data_ptr(), a.posterior.data_ptr(), a.packed_bits.data_ptr(), a.iterations.data_ptr()}
    assert got <= held, "the decode's outputs were meant to land in the blocks that held the junk"
    b = basic_engine(name, gpu_device).decode(x3, early_stop=False, want_packed=True)
    for f in ("bits", "posterior", "iterations", "success", "packed_bits"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    check(a, basic_ref(oracle_mod, name, 3, seed=3), 3, n)
