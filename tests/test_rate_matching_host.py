"""
Rate matching, host side: RateMatching (validation, packed masks, rates, expand / where against the numpy restatement of
tests/rate_matching_reference.py), the SimulationConfig field, codes.staircase_encode, and what the native layer promises
without a device -- the six _rm symbols, their ctypes prototypes, the ldpc_rate_match layout, empty blocks and the
short_llr refusal.
"""
import ctypes
import dataclasses
import re

import numpy as np
import pytest
import torch

import rate_matching_reference as rmref

NEW = ("ldpc_channel_awgn_rm", "ldpc_channel_awgn_mix_rm", "ldpc_sim_count_rm", "ldpc_sim_count_diag_rm",
       "ldpc_simulate_rm", "ldpc_simulate_diag_rm")


# ---------------------------------------------------------------------------------------------------- RateMatching
def test_validation():
    from rate_matching import RateMatching
    rm = RateMatching(13)
    assert rm.n_transmitted == 13 and rm.n_punctured == rm.n_shortened == 0 and rm.count is None and rm.n_counted == 13
    assert rm.short_llr is None
    for bad in (dict(punctured=[13]), dict(punctured=[-1]), dict(punctured=[1, 1]), dict(punctured=np.zeros(12, bool)),
                dict(count=np.ones(14, bool)), dict(punctured=[0.5]), dict(punctured=[[1, 2]])):
        with pytest.raises(ValueError):
            RateMatching(13, **bad)
    with pytest.raises(ValueError):
        RateMatching(0)
    with pytest.raises(ValueError, match="both"):
        RateMatching(13, punctured=[1, 2], shortened=[2, 3], short_llr=8.0)
    # short_llr: required, finite and > 0 exactly when something is shortened
    with pytest.raises(ValueError, match="short_llr"):
        RateMatching(13, shortened=[3])
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError, match="short_llr"):
            RateMatching(13, shortened=[3], short_llr=bad)
    with pytest.raises(ValueError, match="short_llr"):
        RateMatching(13, punctured=[3], short_llr=8.0)
    # index arrays and boolean masks say the same thing
    mask = np.zeros(13, bool)
    mask[[2, 12]] = True
    a, b = RateMatching(13, punctured=[12, 2], count=range(5)), RateMatching(13, punctured=mask, count=np.arange(13) < 5)
    assert np.array_equal(a.punctured, b.punctured) and np.array_equal(a.count, b.count) and a.n_counted == 5
    assert a.n_transmitted == 11 and np.array_equal(a.transmitted, ~mask)


def test_packed_masks_and_the_native_struct():
    import _native
    from rate_matching import RateMatching, pack_mask
    rng = np.random.default_rng(5)
    for n in (1, 7, 8, 9, 13, 96, 1998):
        sel = rng.permutation(n)
        p, s, c = sel[:n // 3], sel[n // 3:n // 2], sel[n // 4:]
        rm = RateMatching(n, punctured=p, shortened=s, count=c, short_llr=9.5 if len(s) else None)
        got = rm.packed("cpu")
        assert rm.packed("cpu") is got                                   # cached
        for t, idx in zip(got, (p, s, c)):
            if t is None:
                assert len(idx) == 0
                continue
            assert t.dtype == torch.uint8 and t.shape == ((n + 7) // 8,)
            bits = np.unpackbits(t.numpy(), bitorder="little")
            assert not bits[n:].any()                                    # pad bits zero
            assert np.array_equal(np.nonzero(bits[:n])[0], np.sort(idx))
            assert np.array_equal(rmref.unpack(t.numpy(), n), bits[:n].astype(bool))
        st = rm.native("cpu")
        assert isinstance(st, _native.RateMatch)
        for t, ptr in zip(got, (st.punctured_packed, st.shortened_packed, st.count_packed)):
            assert ptr == (None if t is None else t.data_ptr())
        assert st.short_llr == (np.float32(9.5) if len(s) else 0.0)
    empty = RateMatching(20).packed("cpu")
    assert empty == (None, None, None)
    assert np.array_equal(pack_mask(np.array([1, 0, 0, 0, 0, 0, 0, 0, 1], bool)), [1, 1])


def test_effective_rate():
    from rate_matching import RateMatching
    assert RateMatching(96).effective_rate(48) == 0.5
    assert RateMatching(96, punctured=range(8)).effective_rate(48) == 48 / 88
    assert RateMatching(96, shortened=range(8), short_llr=20.0).effective_rate(48) == 40 / 88
    assert RateMatching(96, punctured=range(8, 24), shortened=range(8), short_llr=20.0).effective_rate(48) == 40 / 72
    with pytest.raises(ValueError):
        RateMatching(4, punctured=range(4)).effective_rate(2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_where_and_expand_against_the_restatement(dtype):
    from rate_matching import RateMatching
    rng = np.random.default_rng(11)
    n, B = 29, 5
    sel = rng.permutation(n)
    p, s = sel[:6], sel[6:11]
    c = rng.integers(0, 2, n)
    rm = RateMatching(n, punctured=p, shortened=s, short_llr=12.25)
    x = rng.standard_normal((B, n)).astype(np.float32 if dtype == torch.float32 else np.float64)
    x[0, p[0]] = -0.0                                                    # a punctured bit is +0.0 whatever was there
    for cw in (None, c):
        want = rmref.apply(x, rm.punctured, rm.shortened, 12.25, cw)
        got = rm.where(torch.from_numpy(x), cw)
        assert got.dtype == dtype and got.numpy().tobytes() == want.tobytes()
        assert not np.signbit(got.numpy()[:, p]).any() and (got.numpy()[:, p] == 0).all()
        sign = 1 - 2 * (c if cw is not None else np.zeros(n, int))
        assert np.array_equal(got.numpy()[:, s], np.broadcast_to(12.25 * sign[s], (B, len(s))))
        # expand: the transmitted columns in ascending variable order
        tx = x[:, rm.transmitted]
        assert rm.n_transmitted == n - 11 and tx.shape == (B, n - 11)
        ex = rm.expand(torch.from_numpy(tx), cw)
        assert ex.dtype == dtype and ex.numpy().tobytes() == want.tobytes()
    assert rm.where(torch.from_numpy(x)).data_ptr() != torch.from_numpy(x).data_ptr()
    with pytest.raises(ValueError):
        rm.expand(torch.zeros(B, n))
    with pytest.raises(ValueError):
        rm.where(torch.zeros(B, n + 1))
    with pytest.raises(ValueError):
        rm.where(torch.zeros(B, n), codeword=np.full(n, 2))
    # no profile: both are the identity on values
    e = RateMatching(n)
    assert torch.equal(e.where(torch.from_numpy(x)), torch.from_numpy(x)) and torch.equal(e.expand(torch.from_numpy(x)), torch.from_numpy(x))


def test_restated_counters():
    n = 13
    rng = np.random.default_rng(2)
    packed = rng.integers(0, 256, (6, 2), dtype=np.uint8)
    cw = rng.integers(0, 256, 2, dtype=np.uint8)
    count = np.array([0b10110001, 0b11101010], dtype=np.uint8)           # bits 13 .. 15 set: garbage in the pad bits
    bits = lambda a: np.unpackbits(a, axis=-1, bitorder="little")[..., :n].astype(bool)
    want = ((bits(packed) ^ bits(cw)[None]) & bits(count)[None]).sum(axis=1)
    assert np.array_equal(rmref.wrong_bits(packed, n, cw, count), want)
    assert np.array_equal(rmref.wrong_bits(packed, n, cw, None), (bits(packed) ^ bits(cw)[None]).sum(axis=1))
    import philox_reference as ref
    assert np.array_equal(rmref.wrong_bits(packed, n, cw), ref.wrong_bits(packed, n, cw))
    st = rmref.sim_fold([0] * 8, packed, np.arange(6), n, 10, 2, cw, count)
    assert st == ref.sim_fold([0] * 8, want, np.arange(6), 10, 2)


# ---------------------------------------------------------------------------------------------------- SimulationConfig
def test_simulation_config_field():
    from rate_matching import RateMatching
    from simulation_framework import SimulationConfig
    names = [f.name for f in dataclasses.fields(SimulationConfig)]
    assert names[:14] == ["snr_range", "snr_step", "max_frames", "max_errors", "min_frames", "parallel_workers", "device",
                          "save_results", "results_dir", "batch_frames", "seed", "llr_convention", "staged_early_stop",
                          "stage_min_block"]
    assert names[-2:] == ["capture_errors", "rate_matching"] and SimulationConfig().rate_matching is None
    rm = RateMatching(96, punctured=[1, 2])
    assert SimulationConfig(channel="device", rate_matching=rm).rate_matching is rm
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(rate_matching=rm)
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(channel="torch", rate_matching=rm)
    with pytest.raises(ValueError, match="RateMatching"):
        SimulationConfig(channel="device", rate_matching=np.zeros(96, bool))


def test_trainer_takes_the_profile_by_keyword_only():
    import inspect

    from training_framework import PosteriorJointTrainer
    sig = inspect.signature(PosteriorJointTrainer.__init__)
    assert list(sig.parameters) == ["self", "model", "config", "rate_matching"]
    assert sig.parameters["rate_matching"].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters["rate_matching"].default is None


# ---------------------------------------------------------------------------------------------------- staircase_encode
@pytest.mark.parametrize("name", ["small_96_48", "ira_1998_1512", "dvbs2_like_16200_7200"])
def test_staircase_encode(name):
    import codes
    g = codes.load_graph(name)
    k = g.n - g.m
    u = np.random.default_rng(7).integers(0, 2, (3, k))
    c = codes.staircase_encode(g, u)
    assert c.shape == (3, g.n) and c.dtype == np.uint8 and np.array_equal(c[:, :k], u) and c[:, k:].any()
    for row in c:                                                        # H c = 0: every check sees an even number of ones
        assert not (np.add.reduceat(row[g.var_idx].astype(np.int64), g.check_ptr[:-1]) & 1).any()
    assert np.array_equal(codes.staircase_encode(g, u[1]), c[1])
    assert not codes.staircase_encode(g, np.zeros(k, int)).any()
    for bad in (np.zeros(k + 1, int), np.full(k, 2), np.zeros((2, 2, k), int)):
        with pytest.raises(ValueError):
            codes.staircase_encode(g, bad)


def test_staircase_encode_refuses_another_graph():
    import codes
    from tanner_graph import TannerGraph
    H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1]])     # identity, not a staircase
    with pytest.raises(ValueError, match="staircase"):
        codes.staircase_encode(TannerGraph.from_dense(H), [0, 1, 1])
    H2 = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 1, 1, 0], [1, 0, 1, 0, 1, 1]])    # the staircase
    c = codes.staircase_encode(TannerGraph.from_dense(H2), [1, 0, 1])
    assert not (H2 @ c % 2).any()
    H3 = H2.copy()
    H3[2, 3] = 1                                                                   # one edge too many in a parity column
    with pytest.raises(ValueError, match="staircase"):
        codes.staircase_encode(TannerGraph.from_dense(H3), [1, 0, 1])


# ---------------------------------------------------------------------------------------------------- native layer
def test_symbols_are_declared_exported_and_prototyped():
    import _native
    assert set(NEW) <= set(_native.PRODUCT_EXPORTS) and len(set(_native.PRODUCT_EXPORTS)) == len(_native.PRODUCT_EXPORTS)
    header = open(_native.HEADER).read()
    assert "#define LDPC_HIP_ABI_VERSION 1" in header
    lib = _native.load()
    plain = {"ldpc_channel_awgn_rm": 10, "ldpc_channel_awgn_mix_rm": 11, "ldpc_sim_count_rm": 9, "ldpc_sim_count_diag_rm": 16,
             "ldpc_simulate_rm": 6, "ldpc_simulate_diag_rm": 8}
    rm_ptr = ctypes.POINTER(_native.RateMatch)
    for name in NEW:
        assert "int " + name + "(" in header
        fn, base = getattr(lib, name), getattr(lib, name[:-3])
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == plain[name] + 1 == len(base.argtypes) + 1
        at = list(fn.argtypes)
        where = 2 if "simulate" in name else len(at) - 2                 # after desc; else before stream
        assert at[where] is rm_ptr
        del at[where]
        assert at == list(base.argtypes)                                 # the plain argument list with rm inserted
    # the plain entry points keep their argument counts
    assert len(lib.ldpc_channel_awgn.argtypes) == 10 and len(lib.ldpc_sim_count.argtypes) == 9 and len(lib.ldpc_simulate.argtypes) == 6
    assert ctypes.sizeof(_native.SimDesc) == 72
    # the header's parameter lists end in "const ldpc_rate_match *rm, void *stream" (after desc for the simulate forms)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        params = [p.strip() for p in re.search(name + r"\s*\(([^()]*)\)\s*;", text).group(1).split(",")]
        assert params[2 if "simulate" in name else -2] == "const ldpc_rate_match *rm" and params[-1] == "void *stream"


def test_rate_match_layout():
    import _native
    r = _native.RateMatch
    assert [f[0] for f in r._fields_] == ["punctured_packed", "shortened_packed", "count_packed", "short_llr"]
    assert (r.punctured_packed.offset, r.shortened_packed.offset, r.count_packed.offset, r.short_llr.offset) == (0, 8, 16, 24)
    assert ctypes.sizeof(r) == 32 and r.short_llr.size == 4
    header = open(_native.HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} ldpc_rate_match;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == ["punctured_packed", "shortened_packed", "count_packed", "short_llr"]


def test_empty_blocks_and_the_short_llr_refusal_need_no_device():
    import _native
    lib = _native.load()
    R = _native.RateMatch
    fake = 0x1000                                                        # never dereferenced: every call below ends before a launch
    ok = R(punctured_packed=fake, shortened_packed=fake, count_packed=fake, short_llr=7.0)
    none = R()
    for rm in (None, ctypes.byref(none), ctypes.byref(ok)):
        assert lib.ldpc_channel_awgn_rm(None, 0, 8, 0, 0, 0, 1.0, 1.0, None, rm, None) == 0
        assert lib.ldpc_channel_awgn_mix_rm(None, 0, 8, 0, 0, 0, None, None, 1, None, rm, None) == 0
    # the plain calls' checks, in their order, before the profile is looked at
    bad = R(shortened_packed=fake, short_llr=0.0)
    assert lib.ldpc_channel_awgn_rm(None, -1, 8, 0, 0, 0, 1.0, 1.0, None, ctypes.byref(bad), None) == -1
    assert b"batch" in lib.ldpc_last_error()
    assert lib.ldpc_channel_awgn_rm(None, 0, 0, 0, 0, 0, 1.0, 1.0, None, ctypes.byref(bad), None) == -1 and b"n < 1" in lib.ldpc_last_error()
    assert lib.ldpc_channel_awgn_mix_rm(None, 0, 8, 0, 0, 0, None, None, 0, None, ctypes.byref(bad), None) == -1
    assert b"n_points" in lib.ldpc_last_error()
    # short_llr: finite and > 0 whenever shortened_packed is given -- refused even for an empty block; not read otherwise
    for v in (0.0, -3.0, float("inf"), float("-inf"), float("nan")):
        bad = R(shortened_packed=fake, short_llr=v)
        assert lib.ldpc_channel_awgn_rm(None, 0, 8, 0, 0, 0, 1.0, 1.0, None, ctypes.byref(bad), None) == -1
        assert b"short_llr" in lib.ldpc_last_error()
        assert lib.ldpc_channel_awgn_mix_rm(None, 0, 8, 0, 0, 0, None, None, 1, None, ctypes.byref(bad), None) == -1
        assert lib.ldpc_channel_awgn_rm(ctypes.c_void_p(fake), 4, 8, 0, 0, 0, 1.0, 1.0, None, ctypes.byref(bad), None) == -1
        assert lib.ldpc_sim_count_rm(None, None, None, 0, 8, None, 1, 1, ctypes.byref(bad), None) == -1
        assert b"short_llr" in lib.ldpc_last_error()
        assert lib.ldpc_sim_count_diag_rm(None, None, 3, 0, None, None, None, 0, 8, None, 0, 1, 1, None, 0, ctypes.byref(bad), None) == -1
        assert b"short_llr" in lib.ldpc_last_error()
        unused = R(punctured_packed=fake, short_llr=v)
        assert lib.ldpc_channel_awgn_rm(None, 0, 8, 0, 0, 0, 1.0, 1.0, None, ctypes.byref(unused), None) == 0
    # a NULL llr with frames to draw is refused as in the plain call
    assert lib.ldpc_channel_awgn_rm(None, 4, 8, 0, 0, 0, 1.0, 1.0, None, ctypes.byref(ok), None) == -1 and b"llr" in lib.ldpc_last_error()
    assert lib.ldpc_sim_count_rm(None, None, None, 0, 8, None, 1, 1, ctypes.byref(ok), None) == -1 and b"state" in lib.ldpc_last_error()
    out = np.zeros(8, dtype=np.int64)
    assert lib.ldpc_simulate_rm(None, None, ctypes.byref(ok), _native.ptr(out), None, 0, None) == -1
    assert lib.ldpc_simulate_diag_rm(None, None, ctypes.byref(ok), -1, _native.ptr(out), None, None, 0, None) == -1
    assert b"capture" in lib.ldpc_last_error()
