"""
Host tests (no GPU) of Monte-Carlo on random codewords: codes.Encoder against staircase_encode and H c = 0, the numpy
restatement of the information-bit stream (tests/encode_reference.py), the new symbols of include/ldpc_hip.h, the argument
checks a call makes before it touches a device, and SimulationConfig(codeword="random").
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import encode_reference as eref


@pytest.mark.parametrize("name", ["small_96_48", "ira_1998_1512"])
def test_encoder_equals_staircase_encode_under_both_methods(name):
    import codes
    g = codes.load_graph(name)
    k = g.n - g.m
    auto, elim = codes.Encoder.from_graph(g), codes.Encoder.from_graph(g, method="eliminate")
    assert auto.accumulate and not elim.accumulate
    assert int(auto.row_ptr[-1]) == int((np.asarray(g.var_idx) < k).sum())             # the sparse form: the information part of H
    u = np.random.default_rng(5).integers(0, 2, (9, k))
    want = codes.staircase_encode(g, u)
    for e in (auto, elim):
        assert (e.n, e.k, e.systematic) == (g.n, k, True)
        assert np.array_equal(e.info_pos, np.arange(k)) and np.array_equal(e.parity_pos, np.arange(k, g.n))
        got = e.encode(u)
        assert got.dtype == np.uint8 and np.array_equal(got, want)
        assert np.array_equal(e.encode(u[3]), want[3])
    assert np.array_equal(auto.encode(u), elim.encode(u))
    with pytest.raises(ValueError):
        auto.encode(np.zeros(k + 1, dtype=int))
    with pytest.raises(ValueError):
        auto.encode(np.full(k, 2))
    with pytest.raises(ValueError):
        codes.Encoder.from_graph(g, method="dense")


def test_the_committed_16200_code_takes_the_sparse_form():
    import codes
    g = codes.load_graph("dvbs2_like_16200_7200")
    e = codes.Encoder.from_graph(g)
    assert e.accumulate and e.systematic and (e.n, e.k) == (16200, 7200) and e.info_idx.size < g.E
    u = np.random.default_rng(6).integers(0, 2, (2, e.k))
    assert np.array_equal(e.encode(u), codes.staircase_encode(g, u))


def all_words(e):
    u = np.array([[(i >> j) & 1 for j in range(e.k)] for i in range(2 ** e.k)])
    return u, e.encode(u)


def test_toy_codes():
    import codes
    H = eref.toy_H()
    e = codes.Encoder.from_graph(eref.toy_graph())
    assert e.parity_pos.tolist() == [3, 4, 5, 6] and e.k == 3 and e.systematic and not e.accumulate   # the declared k = 4 is not the dimension
    u, c = all_words(e)
    assert len({tuple(r) for r in c}) == 8 and not (H @ c.T % 2).any() and np.array_equal(c[:, e.info_pos], u)
    # columns reversed: H c = 0.  (By the pivot rule columns 4 .. 6 have rank 3 and column 3 completes them, so the positions
    # of THIS matrix are still the identity split; the permuted toy below is the one with scattered positions.)
    Hr = H[:, ::-1]
    er = codes.Encoder.from_graph(eref.toy_graph("reversed"))
    ur, cr = all_words(er)
    assert er.k == 3 and len({tuple(r) for r in cr}) == 8 and not (Hr @ cr.T % 2).any()
    assert np.array_equal(cr[:, er.info_pos], ur)
    # columns 3, 4, 5, 6, 0, 1, 2: the last four are dependent, so a pivot is skipped and the positions are not the identity
    Hp = H[:, eref.TOY_PERMUTATION]
    ep = codes.Encoder.from_graph(eref.toy_graph("permuted"))
    assert not ep.systematic and ep.parity_pos.tolist() == [2, 4, 5, 6] and ep.info_pos.tolist() == [0, 1, 3]
    up, cp = all_words(ep)
    assert len({tuple(r) for r in cp}) == 8 and not (Hp @ cp.T % 2).any() and np.array_equal(cp[:, ep.info_pos], up)
    # a redundant row changes nothing
    Hd = np.vstack([H, H[0] ^ H[2]])
    ed = codes.Encoder.from_graph(eref.toy_graph("deficient"))
    assert ed.k == 3 and ed.parity_pos.tolist() == [3, 4, 5, 6] and ed.row_ptr.size == 5
    _, cd = all_words(ed)
    assert not (Hd @ cd.T % 2).any() and np.array_equal(cd, c)


def test_encoder_refuses_a_csr_above_2_pow_27(monkeypatch):
    import codes
    monkeypatch.setattr(codes.Encoder, "MAX_ENTRIES", 5)
    with pytest.raises(ValueError, match="9 entries"):                       # the toy's reduced rows hold 2 + 2 + 2 + 3 entries
        codes.Encoder.from_graph(eref.toy_graph())


def test_encoder_fields_are_validated():
    import codes
    e = codes.Encoder.from_graph(eref.toy_graph())
    args = dict(n=e.n, k=e.k, info_pos=e.info_pos, parity_pos=e.parity_pos, row_ptr=e.row_ptr, info_idx=e.info_idx,
                accumulate=False)
    codes.Encoder(**args)
    for key, bad in (("info_pos", [0, 1, 3]), ("parity_pos", [6, 5, 4, 3]), ("row_ptr", [0, 3, 2, 4, 6]),
                     ("info_idx", np.full(e.info_idx.size, 3))):
        with pytest.raises(ValueError):
            codes.Encoder(**{**args, key: bad})


def test_info_stream_reference_is_the_stated_stream():
    import philox_reference as ref
    seed, sid, f0 = (7 << 32) | 11, 9, 2 ** 40 + 7
    bits = eref.info_bits(3, 300, seed, sid, f0)
    assert bits.shape == (3, 300) and bits.dtype == np.uint8
    for b, i in ((0, 0), (1, 31), (1, 32), (2, 127), (2, 128), (0, 299)):
        f = f0 + b
        x = ref.philox4x32_10(f & 0xFFFFFFFF, f >> 32, 0x80000000 | (i // 128), sid, seed & 0xFFFFFFFF, seed >> 32)
        assert bits[b, i] == (int(x[(i // 32) % 4]) >> (i % 32)) & 1
    assert 0.4 < bits.mean() < 0.6
    assert np.array_equal(eref.info_bits(2, 300, seed, sid, f0 + 1), bits[1:])           # a frame's bits do not depend on the block


NEW = ("ldpc_encoder_create", "ldpc_encoder_destroy", "ldpc_encode", "ldpc_encode_random", "ldpc_channel_awgn_cw",
       "ldpc_simulate_enc_workspace_bytes", "ldpc_simulate_enc")


def test_new_symbols_are_declared_exported_and_prototyped():
    import os

    import _native
    from conftest import PKG
    header = open(_native.HEADER).read()
    lib = _native.load()
    raw = C.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for name in NEW:
        assert name + "(" in header and name in _native.PRODUCT_EXPORTS and hasattr(raw, name)
        assert getattr(lib, name).argtypes is not None
    assert "ldpc_encode.hip" in _native.SOURCES
    assert [len(getattr(lib, n).argtypes) for n in NEW] == [8, 1, 5, 8, 11, 3, 10]
    assert lib.ldpc_abi_version() == 1 and "#define LDPC_HIP_ABI_VERSION 1" in header
    assert "0x80000000 | (i / 128)" in header                                          # the stream is defined in the header


def test_argument_checks_come_before_any_device():
    import _native
    lib = _native.load()
    vp = C.c_void_p
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    # batch == 0 is LDPC_OK before any pointer is looked at; batch < 0 and a NULL encoder are LDPC_ERR_ARG
    assert lib.ldpc_encode(None, None, 0, None, None) == 0
    assert lib.ldpc_encode_random(None, 0, 1, 2, 3, None, None, None) == 0
    assert lib.ldpc_encode(None, None, -1, None, None) == -1 and lib.ldpc_encode_random(None, -1, 1, 2, 3, None, None, None) == -1
    assert lib.ldpc_encode(None, None, 4, None, None) == -1 and b"encoder" in lib.ldpc_last_error()
    assert lib.ldpc_encode_random(None, 4, 1, 2, 3, None, None, None) == -1 and b"encoder" in lib.ldpc_last_error()
    lib.ldpc_encoder_destroy(None)
    # the channel: the checks and their order are those of ldpc_channel_awgn_rm
    assert lib.ldpc_channel_awgn_cw(None, 0, 7, 1, 2, 3, 1.0, 1.0, None, None, None) == 0
    assert lib.ldpc_channel_awgn_cw(None, -1, 7, 1, 2, 3, 1.0, 1.0, None, None, None) == -1
    assert lib.ldpc_channel_awgn_cw(None, 0, 0, 1, 2, 3, 1.0, 1.0, None, None, None) == -1
    bad = _native.RateMatch(shortened_packed=8, short_llr=float("nan"))
    assert lib.ldpc_channel_awgn_cw(None, 0, 7, 1, 2, 3, 1.0, 1.0, None, C.byref(bad), None) == -1
    assert lib.ldpc_channel_awgn_cw(None, 5, 7, 1, 2, 3, 1.0, 1.0, None, None, None) == -1 and b"llr" in lib.ldpc_last_error()
    # the one-call point
    assert lib.ldpc_simulate_enc_workspace_bytes(None, 64, -1) == 0
    out = np.zeros(8, dtype=np.int64)
    desc = _native.SimDesc(max_frames=1, max_errors=1, block=1, poll_blocks=1)
    assert lib.ldpc_simulate_enc(None, C.byref(desc), None, None, -1, _native.ptr(out), None, None, 0, None) == -1
    # encoder_create validates the host arrays before it asks for a device
    e = vp()
    ip, pp, rp, ii = i32([0, 1, 2]), i32([3, 4, 5, 6]), i32([0, 2, 4, 6, 9]), i32([0, 1, 1, 2, 0, 2, 0, 1, 2])
    create = lambda n, k, a, b, c, d: lib.ldpc_encoder_create(C.byref(e), n, k, _native.ptr(a), _native.ptr(b), _native.ptr(c),
                                                              _native.ptr(d), 0)
    for args, word in (((0, 0, ip, pp, rp, ii), b"n >= 1"), ((7, 8, ip, pp, rp, ii), b"k <= n"),
                       ((7, 3, i32([0, 1, 3]), pp, rp, ii), b"permutation"), ((7, 3, ip, i32([3, 4, 5, 7]), rp, ii), b"range"),
                       ((7, 3, ip, pp, i32([0, 2, 1, 6, 9]), ii), b"monotone"), ((7, 3, ip, pp, i32([1, 2, 4, 6, 9]), ii), b"row_ptr"),
                       ((7, 3, ip, pp, rp, i32([0, 1, 1, 2, 0, 3, 0, 1, 2])), b"info_idx"),
                       ((7, 3, None, pp, rp, ii), b"NULL")):
        assert create(*args) == -1 and word in lib.ldpc_last_error(), (word, lib.ldpc_last_error())
        assert not e.value
    assert lib.ldpc_encoder_create(None, 7, 3, _native.ptr(ip), _native.ptr(pp), _native.ptr(rp), _native.ptr(ii), 0) == -1


def test_simulation_config_random_codeword():
    from simulation_framework import SimulationConfig
    names = [f.name for f in dataclasses.fields(SimulationConfig)]
    assert names[-1] == "rate_matching" and names.count("codeword") == 1 and len(names) == 20      # no new field
    assert SimulationConfig(channel="device", codeword="random").codeword == "random"
    for bad in ("Random", "zero", "", "all-zero"):
        with pytest.raises(ValueError, match="codeword"):
            SimulationConfig(channel="device", codeword=bad)
    with pytest.raises(ValueError):
        SimulationConfig(channel="torch", codeword="random")
    with pytest.raises(ValueError):
        SimulationConfig(codeword="random")
    cw = np.zeros(96, dtype=np.uint8)
    assert SimulationConfig(channel="device", codeword=cw).codeword is cw
    assert SimulationConfig().codeword is None
