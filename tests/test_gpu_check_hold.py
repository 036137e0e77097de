"""
Tests of the held tail of the compact kernels' scalar-counted check phase (res_check_body_uniform with
res_cpt_check_walk): a wave of smallest degree d_lo >= 4 reads the edges in front of its last 4 + (d_lo & 3) in groups
of eight and one group of four, reads that tail as one group and keeps it in registers; pass 2 writes the tail from
the registers and re-reads only the edges in front of it.  Lanes of higher degree than d_lo take their extra edges one at
a time in both passes, waves with d_lo < 4 keep the per-lane form.

The codes are built from lists of check degrees (the builder of test_gpu_compact_checks.py) so that their waves hold
every d_lo from 4 to 14 -- every tail length 4..7 with 0, 4 and 8 edges in front of it -- a spread of 1 on d_lo = 13 as
wave 4 of the (1998,1512) code, a spread of 3, a partly filled last wave, empty waves and a per-lane wave.  The host-only
test checks that list against the plan's own check table; the GPU tests (-m gpu) compare Basic, Neural-2D type 2 and RCQ
decodes at T = 1, 2 and 10 with the streaming engine bit for bit in every output and with the CPU oracle.
"""
import numpy as np
import pytest
import torch

from test_gpu_compact_checks import (QP, assert_post, assert_same_as_stream, code_from_check_degrees, llrs,
                                     oracle_graph, table_of)

gpu = pytest.mark.gpu
B = 37
PER_LANE = 1 << 31

# name: (seed, n, check degrees -- the plan sorts them descending, 64 to a wave)
CODES = {
    # 14 | 12 | 10 | 9 | 8 | 6 | 5 | 20 lanes of 4: tails 6, 4, 6, 5, 4, 6, 5, 4 behind 8, 8, 4, 4, 4, 0, 0, 0 edges
    "steps": (31, 1200, [14] * 64 + [12] * 64 + [10] * 64 + [9] * 64 + [8] * 64 + [6] * 64 + [5] * 64 + [4] * 20),
    # 14, 13 (d_lo 13, spread 1) | 13 | 11 | 10, 9, 8, 7 (d_lo 7, spread 3) | 5 and 3: per lane, 50 lanes | three empty
    "mixed": (32, 1100, [14] * 32 + [13] * 32 + [13] * 64 + [11] * 64 + [10, 9, 8, 7] * 16 + [5] * 30 + [3] * 20),
}
# (d_lo, spread, lanes, per-lane) of waves 0..7
TABLES = {
    "steps": [(14, 0, 64, False), (12, 0, 64, False), (10, 0, 64, False), (9, 0, 64, False), (8, 0, 64, False),
              (6, 0, 64, False), (5, 0, 64, False), (4, 0, 20, False)],
    "mixed": [(13, 1, 64, False), (13, 0, 64, False), (11, 0, 64, False), (7, 3, 64, False), (3, 2, 50, True)]
             + [(0, 0, 0, False)] * 3,
    "ira": [(14, 0, 64, False)] * 4 + [(13, 1, 64, False)] + [(13, 0, 64, False)] * 2 + [(13, 0, 38, False)],
}


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


_codes = {}


def make_code(name, T):
    """one H per name (the builder is deterministic in its seed); a code object per (name, T)"""
    from ldpc_decoder import LDPCCode
    if name == "ira":
        import codes
        return codes.load_code("ira_1998_1512", max_iterations=T)
    if name not in _codes:
        seed, n, dcs = CODES[name]
        _codes[name] = code_from_check_degrees(seed, n, dcs, T).H
    H = _codes[name]
    return LDPCCode(n=H.shape[1], k=H.shape[1] - H.shape[0], H=H, max_iterations=T)


def held_split(d_lo):
    """(edges held between the passes, edges in front of them) of a scalar-counted wave"""
    tail = 4 + (d_lo & 3)
    return tail, d_lo - tail


def test_the_codes_cover_every_branch():
    """host side of the case list: the plan's check table of each built code is the one written down above, every code
    qualifies for the compact plan (m <= 495, n <= 2048, check degrees <= 14, variable degrees <= 8, three workgroups
    per CU: ldpc_debug_compact_checks refuses a graph that does not), and the tables hold every branch of the walk"""
    import _native
    lib = _native.load()
    for name in CODES:
        H = make_code(name, 10).H
        assert H.shape[0] <= 495 and H.shape[1] <= 2048 and H.sum(axis=1).max() <= 14 and H.sum(axis=0).max() <= 8
        cp = np.concatenate([[0], np.cumsum(H.sum(axis=1))]).astype(np.int32)
        vi = np.concatenate([np.nonzero(H[i])[0] for i in range(H.shape[0])]).astype(np.int32)
        words = np.full(8, 0xDEADBEEF, dtype=np.uint32)
        rc = lib.ldpc_debug_compact_checks(None, H.shape[1], H.shape[0], len(vi), _native.ptr(cp), _native.ptr(vi),
                                           _native.ptr(words))
        assert rc == 0, name
        got = [(int(w) & 0xFF, int(w) >> 8 & 0xFF, int(w) >> 16 & 0xFF, bool(int(w) & PER_LANE)) for w in words]
        assert got == TABLES[name], name
    waves = [w for name in CODES for w in TABLES[name]]
    scalar = [w for w in waves if w[2] and not w[3]]
    assert all(w[0] >= 4 for w in scalar)
    assert {w[0] for w in scalar} == set(range(4, 15))
    splits = {held_split(w[0]) for w in scalar}
    assert splits == {(t, b) for t in (4, 5, 6, 7) for b in (0, 4, 8) if t + b <= 14}
    assert all(b % 4 == 0 for _, b in splits)
    assert TABLES["ira"][4] in scalar                                        # spread 1 on d_lo = 13
    assert any(w[1] == 3 for w in scalar)
    assert any(0 < w[2] < 64 for w in scalar) and any(w[2] == 0 for w in waves)
    assert any(w[3] and w[2] and w[0] < 4 for w in waves)
    assert {held_split(w[0]) for w in TABLES["ira"]} == {(6, 8), (5, 8)}     # [8][6] and [8][5]


def assert_table(eng, name):
    assert table_of(eng) == TABLES[name]


@gpu
@pytest.mark.parametrize("name", ["steps", "mixed"])
@pytest.mark.parametrize("T", [1, 2, 10])
def test_basic(name, T, gpu_device, oracle_mod):
    from ldpc_decoder import BasicMinSumDecoder
    code = make_code(name, T)
    llr = llrs(150 + T, B, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    assert_table(eng, name)
    res = assert_same_as_stream(eng, torch.from_numpy(llr).to(gpu_device))
    ob, op, oi, os_ = oracle_mod.basic_minsum(oracle_graph(oracle_mod, code), llr, 0.7, T, early_stop=False,
                                              dtype=np.float32)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert_post(res.posterior.cpu().numpy(), op)


@gpu
@pytest.mark.parametrize("name", ["steps", "mixed"])
@pytest.mark.parametrize("T", [1, 2, 10])
def test_neural2d_per_check_beta(name, T, gpu_device, oracle_mod):
    """sharing type 2 with random weights: one beta per check degree and iteration, one alpha per variable degree"""
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = make_code(name, T)
    rng = np.random.default_rng(160 + T)
    llr = llrs(161 + T, B, code.n)
    dec = Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=T)
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
    ob, op, oi, _ = oracle_mod.neural2d(oracle_graph(oracle_mod, code), llr, 2, T, beta, alpha, early_stop=False)
    np.testing.assert_array_equal(bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(iters.cpu().numpy(), oi)
    assert_post(post.cpu().numpy(), op)


@gpu
@pytest.mark.parametrize("name", ["steps", "mixed"])
@pytest.mark.parametrize("T", [1, 2, 10])
def test_rcq(name, T, gpu_device, oracle_mod):
    from rcq_decoder import RCQMinSumDecoder
    code = make_code(name, T)
    llr = llrs(170 + T, B, code.n)
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


@gpu
def test_flagship_code(gpu_device, oracle_mod):
    """the (1998,1512) code itself: degree 14 as [8][6], degree 13 as [8][5], wave 4 with its one masked edge"""
    from ldpc_decoder import BasicMinSumDecoder
    code = make_code("ira", 10)
    llr = llrs(180, B, code.n)
    eng = BasicMinSumDecoder(code, 0.7)._engine(torch.float32, gpu_device)
    assert_table(eng, "ira")
    res = assert_same_as_stream(eng, torch.from_numpy(llr).to(gpu_device))
    ob, op, oi, os_ = oracle_mod.basic_minsum(oracle_graph(oracle_mod, code), llr, 0.7, 10, early_stop=False,
                                              dtype=np.float32)
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy(), os_)
    assert_post(res.posterior.cpu().numpy(), op)
