"""
The symbol channel without a device: the numpy restatement of its definition (tests/modulation_reference.py) against a
brute-force joint demapper, the Gray labelling and the constellations' energy, Modulation.amp, the new C symbols and the
ldpc_modulation layout, and every refusal that happens before a device is touched.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import modulation_reference as mref

ALL_M = (1, 2, 4, 6, 8)


@pytest.mark.parametrize("m", ALL_M)
def test_separable_demapper_equals_brute_force_maxlog(m):
    """the per-axis fp32 demapper against the float64 max-log over all 2^m complex points.  Signs must agree wherever the
    brute-force value is not within rounding of zero.  Values: |v| <= 40 and e * |a'| <= 4 * 15, so a distance term is at
    most t = 100 in magnitude; e * a', t and t * t each round once to fp32 (relative 2^-24), giving D an absolute error below
    3 * 2^-24 * 100^2 = 1.8e-3, and the difference of two minima and its rounding stay below 4e-3 in the LLR."""
    rng = np.random.default_rng(100 + m)
    N = 4000
    v = (rng.uniform(-40, 40, N) + 1j * rng.uniform(-40, 40, N)) * (rng.random(N) < 0.9)
    e = np.where(rng.random(N) < 0.1, 0.0, rng.uniform(0.0, 4.0, N))
    v32 = np.stack([v.real.astype(np.float32), (v.imag if m > 1 else 0 * v.imag).astype(np.float32)], -1)
    e32 = e.astype(np.float32)
    rec = np.zeros((1, N, 4), dtype=np.float32)
    rec[0, :, 0], rec[0, :, 1], rec[0, :, 2] = v32[:, 0], v32[:, 1], e32
    got = mref.demap(rec, m)[0]
    assert got.dtype == np.float32 and got.shape == (N, m)
    want = mref.brute_force_maxlog(v32[:, 0].astype(np.float64) + 1j * v32[:, 1].astype(np.float64), e32.astype(np.float64), m)
    tol = 4e-3
    assert np.abs(got.astype(np.float64) - want).max() <= tol
    clear = np.abs(want) > tol
    assert clear.mean() > 0.7 and np.array_equal(np.sign(got[clear]), np.sign(want[clear]))


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_the_labelling_is_gray_and_bit_zero_is_the_positive_half(h):
    labels = mref.level_labels(h)                                   # level i <-> amplitude (2^h - 1) - 2 i
    assert np.array_equal(mref.level_index(labels), np.arange(2 ** h))
    assert np.array_equal(mref.amplitude(labels), (2 ** h - 1) - 2 * np.arange(2 ** h))
    assert ((labels[1:] != labels[:-1]).sum(axis=1) == 1).all()     # neighbours differ in one bit
    assert np.array_equal(labels[:, 0] == 0, mref.amplitude(labels) > 0)
    assert len({tuple(r) for r in labels}) == 2 ** h
    if h == 1:
        assert mref.amplitude(np.array([0])) == 1 and mref.amplitude(np.array([1])) == -1


@pytest.mark.parametrize("scheme,m", sorted(mref.SCHEMES.items()))
def test_every_constellation_has_unit_energy_and_distinct_points(scheme, m):
    from modulation import Modulation, half_spacing
    pts, labels = mref.constellation(m)
    assert len(pts) == 2 ** m and len(set(np.round(pts, 9))) == 2 ** m
    assert abs(np.mean(np.abs(pts) ** 2) - 1.0) < 1e-12
    assert Modulation(scheme).bits_per_symbol == m and half_spacing(m) == pytest.approx(mref.half_spacing(m), rel=1e-15)
    # Gray on the grid: nearest neighbours (distance 2 d) differ in exactly one label bit
    d = mref.half_spacing(m)
    for i in range(len(pts)):
        near = np.nonzero(np.abs(np.abs(pts - pts[i]) - 2 * d) < 1e-9)[0]
        assert len(near) >= 1 and ((labels[near] != labels[i]).sum(axis=1) == 1).all()


def test_amp_follows_the_package_snr_convention():
    import engine
    from modulation import Modulation
    for snr in (-3.0, 0.0, 2.5, 11.0):
        n0 = 10.0 ** (-snr / 10.0)
        for scheme in ("bpsk", "qpsk"):
            assert 2.0 * Modulation(scheme).amp(snr) == pytest.approx(engine.awgn_scale_shift(snr)[0], rel=1e-14)
        assert Modulation("qam16").amp(snr) == pytest.approx(math.sqrt(1.0 / (5.0 * n0)), rel=1e-14)
        assert Modulation("qam64").amp(snr) == pytest.approx(math.sqrt(1.0 / (21.0 * n0)), rel=1e-14)
        assert Modulation("qam256").amp(snr) == pytest.approx(math.sqrt(1.0 / (85.0 * n0)), rel=1e-14)
        assert Modulation("qam16", fading="rayleigh").amp(snr) == Modulation("qam16").amp(snr)
    mod = Modulation("qam64")
    assert [mod.symbols(n) for n in (1, 6, 7, 1998)] == [1, 1, 2, 333] and Modulation("bpsk").symbols(7) == 7


def test_the_restated_stream_uses_its_own_counter_word():
    import philox_reference as ref
    seed, sid, f0 = (5 << 32) | 3, 77, 2 ** 32 - 1
    w = mref.symbol_words(2, 5, seed, sid, f0)
    assert w.shape == (2, 5, 4) and w.dtype == np.uint32
    for b, s in ((0, 0), (1, 4)):
        f = f0 + b
        x = ref.philox4x32_10(f & 0xFFFFFFFF, f >> 32, 0x40000000 | s, sid, seed & 0xFFFFFFFF, seed >> 32)
        assert [int(v) for v in x] == [int(v) for v in w[b, s]]
    assert not np.array_equal(w, ref.stream_words(2, 5, seed, sid, f0))             # not the BI-AWGN quads
    g = mref.fading_gain(mref.symbol_words(64, 64, seed, sid, 0))
    assert abs((g ** 2).mean() - 1.0) < 0.08 and (g >= 0).all()                      # E g^2 = 1: sigma / sqrt(4096) = 0.016
    z = mref.symbol_normals(mref.symbol_words(64, 64, seed, sid, 0))
    assert abs(z.mean()) < 0.05 and abs(z.var() - 1.0) < 0.08


NEW = ("ldpc_channel_sym", "ldpc_simulate_sym_workspace_bytes", "ldpc_simulate_sym")


def test_new_symbols_are_declared_exported_and_prototyped():
    import _native
    from conftest import PKG
    header = open(_native.HEADER).read()
    lib = _native.load()
    raw = C.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for name in NEW:
        assert name + "(" in header and name in _native.PRODUCT_EXPORTS and hasattr(raw, name)
        assert getattr(lib, name).argtypes is not None
    assert "ldpc_modulation.hip" in _native.SOURCES
    assert [len(getattr(lib, n).argtypes) for n in NEW] == [11, 3, 10]
    assert lib.ldpc_abi_version() == 1 and "#define LDPC_HIP_ABI_VERSION 1" in header
    assert "0x40000000 | s" in header                                                # the stream is defined in the header
    unit = open(os.path.join(PKG, "csrc", "ldpc_hip.hip")).read()
    assert unit.index('#include "ldpc_encode.hip"') < unit.index('#include "ldpc_modulation.hip"')


def test_ctypes_struct_matches_the_header():
    import _native
    header = open(_native.HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} ldpc_modulation;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    types = [d[:d.rindex(n)].replace(" ", "") for d, n in zip(decls, names)]
    assert names == [f[0] for f in _native.ModulationDesc._fields_] == ["bits_per_symbol", "fading", "amp", "position"]
    assert types == ["int32_t", "int32_t", "float", "constint32_t*"]
    assert [f[1] for f in _native.ModulationDesc._fields_] == [C.c_int32, C.c_int32, C.c_float, C.c_void_p]
    M = _native.ModulationDesc
    assert (M.bits_per_symbol.offset, M.fading.offset, M.amp.offset, M.position.offset) == (0, 4, 8, 16) and C.sizeof(M) == 24


def test_modulation_refuses_what_it_cannot_send():
    from modulation import Modulation
    for bad in ("8psk", "QPSK", "qam32", "apsk16", None, 4):
        with pytest.raises(ValueError, match="scheme"):
            Modulation(bad)
    for bad in ("block", "rician", 1, ""):
        with pytest.raises(ValueError, match="fading"):
            Modulation("qpsk", fading=bad)
    for bad in ([0, 0, 1], [1, 2, 3], [0.0, 1.0], [[0, 1]], []):
        with pytest.raises(ValueError, match="interleaver"):
            Modulation("qam16", interleaver=bad)
    mod = Modulation("qam16", fading="rayleigh", interleaver=[2, 0, 1])
    assert mod.interleaver.dtype == np.int32 and mod.fading == "rayleigh"
    with pytest.raises(ValueError, match="interleaver"):
        mod.check(4)                                                                 # a permutation of 3 on a frame of 4
    with pytest.raises(NotImplementedError):
        Modulation("bpsk").check(2 ** 29)


def test_simulation_config_refuses_before_any_device():
    from modulation import Modulation
    from rate_matching import RateMatching
    from simulation_framework import SimulationConfig
    q16, qpsk = Modulation("qam16"), Modulation("qpsk")
    cfg = SimulationConfig(channel="device", codeword="random", modulation=q16)
    assert cfg.modulation is q16 and SimulationConfig().modulation is None
    assert SimulationConfig(channel="device", modulation=qpsk).modulation is qpsk     # QPSK is symmetric: all-zero is allowed
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(channel="torch", modulation=qpsk)
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(modulation=qpsk)
    with pytest.raises(ValueError, match="rate_matching"):
        SimulationConfig(channel="device", codeword="random", modulation=q16, rate_matching=RateMatching(8, punctured=[1]))
    for scheme in ("qam16", "qam64", "qam256"):
        with pytest.raises(ValueError, match='codeword="random"'):
            SimulationConfig(channel="device", modulation=Modulation(scheme))
    with pytest.raises(ValueError, match="Modulation"):
        SimulationConfig(channel="device", modulation="qam16")


def test_argument_checks_come_before_any_device():
    import _native
    lib = _native.load()
    mod = lambda m=4, fading=0, amp=1.0: C.byref(_native.ModulationDesc(bits_per_symbol=m, fading=fading, amp=amp))
    call = lambda batch, n, md, stride=0, llr=None, rec=None: lib.ldpc_channel_sym(llr, batch, n, 1, 2, 3, md, None, stride,
                                                                                     rec, None)
    assert call(0, 7, mod()) == 0                                                    # an empty block: OK, no pointer looked at
    assert call(0, 7, mod(), stride=1) == 0
    assert call(-1, 7, mod()) == -1 and b"batch" in lib.ldpc_last_error()
    assert call(0, 0, mod()) == -1 and b"n < 1" in lib.ldpc_last_error()
    assert call(0, 7, None) == -1 and b"mod" in lib.ldpc_last_error()
    for m in (0, 3, 5, 7, 10, -2):
        assert call(0, 7, mod(m)) == -1 and b"bits_per_symbol" in lib.ldpc_last_error()
    assert call(0, 7, mod(fading=2)) == -1 and b"fading" in lib.ldpc_last_error()
    for amp in (float("nan"), float("inf"), -float("inf"), -1.0):
        assert call(0, 7, mod(amp=amp)) == -1 and b"amp" in lib.ldpc_last_error()
    assert call(0, 7, mod(amp=0.0)) == 0
    assert call(0, 7, mod(), stride=2) == -1 and b"stride" in lib.ldpc_last_error()
    assert call(0, 2 ** 29, mod(1)) == -3 and b"2^29" in lib.ldpc_last_error()       # S >= 2^29: LDPC_ERR_UNSUPPORTED
    assert call(0, 2 ** 29 - 1, mod(1)) == 0 and call(0, 2 ** 30 - 2, mod(2)) == 0   # S = 2^29 - 1
    assert call(0, 2 ** 30 - 1, mod(2)) == -3
    assert call(0, 2 ** 31 - 1, mod(4)) == -3 and call(0, 2 ** 31 - 1, mod(6)) == 0
    assert call(5, 7, mod()) == -1 and b"llr" in lib.ldpc_last_error()               # pointers only after batch == 0
    # the one-call point
    assert lib.ldpc_simulate_sym_workspace_bytes(None, 64, -1) == 0
    out = np.zeros(8, dtype=np.int64)
    desc = _native.SimDesc(max_frames=1, max_errors=1, block=1, poll_blocks=1)
    assert lib.ldpc_simulate_sym(None, C.byref(desc), None, mod(), -1, _native.ptr(out), None, None, 0, None) == -1
