"""
The constellation channel without a device: the tables and factories of ``modulation.Constellation``, what it refuses, the
ldpc_constellation layout and the new C symbols, the native argument checks in their order (none needs a device), and the
numpy restatement of the joint rule (tests/constellation_reference.py) against a float64 brute force.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import constellation_reference as cref
import modulation_reference as mref

NEW = ("ldpc_channel_con", "ldpc_channel_con_mix", "ldpc_demap_con", "ldpc_simulate_con")


def apsk16(**kw):
    from modulation import Constellation
    return Constellation.apsk((4, 12), (1.0, 2.6), **kw)


def apsk32(**kw):
    from modulation import Constellation
    return Constellation.apsk((4, 12, 16), (1.0, 2.64, 4.64), **kw)


def random_table(count, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=count) + 1j * rng.normal(size=count)


def tables():
    """one table per m = 1 .. 6"""
    from modulation import Constellation
    return [Constellation.psk(2), Constellation.psk(4), Constellation.psk(8), apsk16(), apsk32(),
            Constellation(random_table(64, 64))]


# ------------------------------------------------------------------ tables and factories
def test_tables_are_normalised_to_unit_energy_and_cast_once():
    from modulation import Constellation, Modulation
    for con in tables() + [Constellation(7.0 * random_table(8, 3)), Constellation(np.array([[3.0, 0.0], [0.0, -4.0]]))]:
        assert isinstance(con, Modulation)
        pts = con.points
        assert pts.dtype == np.float32 and pts.shape == (2 ** con.bits_per_symbol, 2) and pts.flags.c_contiguous
        # the cast moves a coordinate by 2^-24 relative at most: the mean energy by 2^-23
        assert abs((pts.astype(np.float64) ** 2).sum(axis=1).mean() - 1.0) <= 2.0 ** -22
        assert np.allclose(con.complex_points, pts[:, 0] + 1j * pts[:, 1])
    raw = random_table(16, 5)
    con = Constellation(raw)
    want = raw / math.sqrt(np.mean(np.abs(raw) ** 2))
    assert np.array_equal(con.points, np.stack([want.real, want.imag], -1).astype(np.float32))     # double, then one cast
    same = Constellation(np.stack([raw.real, raw.imag], -1))
    assert np.array_equal(con.points, same.points)                                                  # [M, 2] real is the same table
    assert [Constellation(random_table(c, 1)).bits_per_symbol for c in (2, 4, 8, 16, 32, 64)] == [1, 2, 3, 4, 5, 6]
    assert Constellation(np.array([1.0, 1.0, -1.0, -1.0]) + 0j).bits_per_symbol == 2               # duplicates are allowed
    assert con.scheme == "constellation" and Constellation(raw, name="mine").scheme == "mine"
    assert Constellation(raw, "rayleigh", None, "exact").demapper == "exact" and Constellation(raw, "rayleigh").fading == "rayleigh"
    assert repr(con) == "Constellation(<16 points>, fading=None, interleaver=None)"
    assert [con.symbols(n) for n in (1, 4, 5, 1998)] == [1, 1, 2, 500] and Constellation.psk(8).symbols(1998) == 666


@pytest.mark.parametrize("M", [2, 4, 8, 16, 32, 64])
def test_psk_is_gray_on_the_circle(M):
    from modulation import Constellation
    for phase in (None, 0.0, 0.3):
        con = Constellation.psk(M, phase)
        z = con.complex_points
        assert np.allclose(np.abs(z), 1.0, atol=1e-6) and con.scheme == f"psk{M}" and con.bits_per_symbol == int(math.log2(M))
        phi0 = math.pi / M if phase is None else phase
        j = np.arange(M)
        label = j ^ (j >> 1)                                        # position j carries label j ^ (j >> 1)
        assert np.allclose(z[label], np.exp(1j * (phi0 + 2 * math.pi * j / M)), atol=1e-6)
        # neighbouring positions (the circle closes) differ in exactly one label bit
        diff = label ^ np.roll(label, -1)
        assert all(bin(int(d)).count("1") == 1 for d in diff)
        assert len(set(label.tolist())) == M


def test_apsk_rings_radii_phases_and_labels():
    from modulation import Constellation
    for sizes, radii in (((4, 12), (1.0, 2.6)), ((4, 12, 16), (1.0, 2.64, 4.64)), ((8, 8), (2.0, 5.0)), ((64,), (1.0,))):
        con = Constellation.apsk(sizes, radii)
        z = con.complex_points
        assert con.scheme == "apsk" + "+".join(map(str, sizes)) and len(z) == sum(sizes)
        scale = math.sqrt(sum(k * r * r for k, r in zip(sizes, radii)) / sum(sizes))
        start = 0
        for k, r in zip(sizes, radii):
            ring = z[start:start + k]                                # running index: inner ring first
            assert np.allclose(np.abs(ring), r / scale, atol=1e-6)
            want = (r / scale) * np.exp(1j * (math.pi / k + 2 * math.pi * np.arange(k) / k))      # counter-clockwise from pi / k
            assert np.allclose(ring, want, atol=1e-6)
            start += k
    con = Constellation.apsk((4, 12), (1.0, 2.6), phases=(0.0, 0.1))
    z = con.complex_points
    assert np.angle(z[0]) == pytest.approx(0.0, abs=1e-6) and np.angle(z[4]) == pytest.approx(0.1, abs=1e-6)
    lab = np.random.default_rng(1).permutation(16)
    plain, perm = Constellation.apsk((4, 12), (1.0, 2.6)), Constellation.apsk((4, 12), (1.0, 2.6), labels=lab)
    assert np.array_equal(perm.points[lab], plain.points)           # point i of the running order carries label lab[i]
    for bad in (np.arange(15), np.zeros(16, int), np.arange(16) + 1, np.arange(16.0), [[0] * 16]):
        with pytest.raises(ValueError, match="labels"):
            Constellation.apsk((4, 12), (1.0, 2.6), labels=bad)
    for sizes, radii in (((4, 11), (1, 2)), ((4, 12), (1,)), ((4, 12), (1, -2)), ((4, 12), (1, float("nan"))), ((), ()),
                         ((64, 64), (1, 2)), ((0, 16), (1, 2))):
        with pytest.raises(ValueError):
            Constellation.apsk(sizes, radii)
    with pytest.raises(ValueError, match="phases"):
        Constellation.apsk((4, 12), (1, 2), phases=(0.0,))
    assert "NOT the DVB-S2 bit maps" in Constellation.apsk.__doc__


@pytest.mark.parametrize("scheme", ["bpsk", "qpsk", "qam16", "qam64"])
def test_from_modulation_is_the_schemes_table(scheme):
    from modulation import Constellation, Modulation
    pos = np.random.default_rng(2).permutation(12)
    mod = Modulation(scheme, "rayleigh", pos, "exact")
    con = Constellation.from_modulation(mod)
    m = mref.SCHEMES[scheme]
    pts, labels = mref.constellation(m)
    assert np.array_equal(labels, cref.label_bits(m))
    # the double table is the reference's up to the normalisation's rounding (a few 2^-53), the cast is the only fp32 step
    assert np.abs(con.complex_points - pts).max() <= 2.0 ** -24 * np.abs(pts).max() + 1e-15
    assert (con.bits_per_symbol, con.fading, con.demapper, con.scheme) == (m, "rayleigh", "exact", scheme)
    assert np.array_equal(con.interleaver, pos)
    assert Constellation.from_modulation(mod, fading=None, demapper="maxlog").fading is None


def test_from_modulation_refuses_256_points_and_tables():
    from modulation import Constellation, Modulation
    with pytest.raises(ValueError, match="64"):
        Constellation.from_modulation(Modulation("qam256"))
    for bad in ("qam16", None, Constellation.psk(8)):
        with pytest.raises(ValueError):
            Constellation.from_modulation(bad)


def test_amp_and_normalise_received_follow_the_definition():
    import torch
    from modulation import Constellation, Modulation
    con = Constellation.psk(8)
    for snr in (-3.0, 0.0, 2.5, 11.0):
        n0 = 10.0 ** (-snr / 10.0)
        for c in (con, Constellation.psk(2), apsk32()):
            assert c.amp(snr) == pytest.approx(1.0 / math.sqrt(n0 / 2.0), rel=1e-14)           # 1 / sigma, m = 1 included
        # a QAM table at snr_db has the gain e * x the string scheme has: amp * d against amp
        for scheme in ("qpsk", "qam16", "qam64"):
            mod = Modulation(scheme)
            d = mref.half_spacing(mod.bits_per_symbol)
            assert Constellation.from_modulation(mod).amp(snr) * d == pytest.approx(mod.amp(snr), rel=1e-14)
    tab = con.amp_table([0.0, 3.0, 6.5])
    assert tab.dtype == np.float32 and np.array_equal(tab, np.array([con.amp(s) for s in (0.0, 3.0, 6.5)]).astype(np.float32))
    y = np.array([[1 + 2j, -0.5j, 3.0]])
    h = np.array([[2j, 0.0, -0.5]])
    sig = math.sqrt(0.5 / 2.0)
    out = con.normalise_received(y, h, noise_var=0.5)
    assert out.dtype == torch.float32 and tuple(out.shape) == (1, 3, 4)
    want = np.zeros((1, 3, 4))
    rot = y * np.array([[-1j, 1.0, -1.0]])                           # conj(h) / |h|; |h| = 0 leaves y as it is
    want[..., 0], want[..., 1], want[..., 2] = rot.real / sig, rot.imag / sig, np.abs(h) / sig
    assert np.array_equal(out.numpy(), want.astype(np.float32))
    one = Constellation.psk(2).normalise_received(y, snr_db=3.0)      # m = 1 keeps its quadrature component
    s3 = math.sqrt(10 ** -0.3 / 2)
    assert np.array_equal(one.numpy()[..., 1], (y.imag / s3).astype(np.float32)) and (one.numpy()[..., 2] == np.float32(1 / s3)).all()
    for bad in ({}, {"snr_db": 1.0, "noise_var": 0.5}):
        with pytest.raises(ValueError, match="exactly one"):
            con.normalise_received(y, **bad)
    with pytest.raises(ValueError):
        con.normalise_received(y, np.ones((1, 2)), snr_db=1.0)


# ------------------------------------------------------------------ refusals
def test_constellation_refuses_what_it_cannot_send():
    from modulation import Constellation
    for count in (1, 3, 6, 12, 48, 65, 128):
        with pytest.raises(ValueError, match="power of two"):
            Constellation(random_table(count, count))
    for bad in (np.array([1.0, float("nan"), 0, 0]) + 0j, np.array([[1.0, float("inf")], [0.0, 0.0]])):
        with pytest.raises(ValueError, match="finite"):
            Constellation(bad)
    with pytest.raises(ValueError, match="zero"):
        Constellation(np.zeros(4, complex))
    for bad in (np.zeros((4, 3)), np.zeros(4), np.zeros((2, 2, 2)), np.zeros((2, 4), complex), "psk", [["a", "b"]] * 2, 1.0):
        with pytest.raises(ValueError, match="points"):
            Constellation(bad)
    ok = random_table(8, 1)
    with pytest.raises(ValueError, match="fading"):
        Constellation(ok, fading="block")
    with pytest.raises(ValueError, match="demapper"):
        Constellation(ok, demapper="logmap")
    with pytest.raises(ValueError, match="interleaver"):
        Constellation(ok, interleaver=[0, 0, 1])
    with pytest.raises(ValueError, match="name"):
        Constellation(ok, name=8)
    for M in (0, 1, 3, 12, 128):
        with pytest.raises(ValueError, match="power of two"):
            Constellation.psk(M)
    con = Constellation(ok, interleaver=[2, 0, 1])
    with pytest.raises(ValueError, match="interleaver"):
        con.check(4)
    with pytest.raises(NotImplementedError):
        Constellation.psk(2).check(2 ** 29)
    # the string schemes keep their refusal and now say where to go
    from modulation import Modulation
    with pytest.raises(ValueError, match="Constellation"):
        Modulation("8psk")


def test_simulation_config_and_trainer_refuse_before_any_device():
    import codes
    from modulation import Constellation
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rate_matching import RateMatching
    from simulation_framework import SimulationConfig
    from training_framework import PosteriorJointTrainer, TrainingConfig
    psk8, bpsk = Constellation.psk(8), Constellation.psk(2)
    cfg = SimulationConfig(channel="device", codeword="random", modulation=psk8)
    assert cfg.modulation is psk8
    assert SimulationConfig(channel="device", codeword=np.zeros(96, np.uint8), modulation=psk8).modulation is psk8
    for con in (psk8, bpsk, Constellation.psk(4)):                    # no table is assumed symmetric, two points included
        with pytest.raises(ValueError, match='codeword="random"'):
            SimulationConfig(channel="device", modulation=con)
    with pytest.raises(ValueError, match="rate_matching"):
        SimulationConfig(channel="device", codeword="random", modulation=psk8, rate_matching=RateMatching(8, punctured=[1]))
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(channel="torch", codeword="random", modulation=psk8)
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(codeword="random", modulation=psk8)
    code = codes.load_code("small_96_48", max_iterations=2)
    tcfg = TrainingConfig(batch_size=8, num_epochs=1, device="cpu", seed=1)
    make = lambda **kw: PosteriorJointTrainer(Neural2DMinSumDecoder(code, 2, 2), tcfg, **kw)
    assert make(modulation=psk8, codeword="random").modulation is psk8
    for con in (psk8, bpsk):
        with pytest.raises(ValueError, match='codeword="random"'):
            make(modulation=con)
    with pytest.raises(ValueError, match="rate_matching"):
        make(modulation=psk8, codeword="random", rate_matching=RateMatching(96, punctured=[1]))


def test_engine_refuses_before_a_device_is_asked_for():
    import torch
    import engine
    from modulation import Constellation
    con = Constellation.psk(8)
    good = torch.zeros((2, 32, 4), dtype=torch.float32)
    for bad in (good.numpy(), good.double(), good[:, :, :3], good[:, :31], torch.zeros((2, 48, 4))):   # 48 = 96 / 2: not 8-PSK's S
        with pytest.raises(ValueError, match="received"):
            engine.demap(bad, 96, modulation=con)
    with pytest.raises(ValueError, match="demapper"):
        engine.demap(good, 96, modulation=con, demapper="logmap")
    with pytest.raises(ValueError, match="GPU"):
        engine.demap(good, 96, modulation=con)
    with pytest.raises(ValueError, match="snr_db or amp"):
        engine.sym_llr_mix(2, 96, seed=1, modulation=con)


# ------------------------------------------------------------------ ABI
def test_ctypes_struct_matches_the_header():
    import _native
    header = open(_native.HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} ldpc_constellation;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls]
    types = [d[:d.rindex(n)].replace(" ", "") for d, n in zip(decls, names)]
    D = _native.ConstellationDesc
    assert names == [f[0] for f in D._fields_] == ["bits_per_symbol", "fading", "amp", "position", "points"]
    assert types == ["int32_t", "int32_t", "float", "constint32_t*", "constfloat*"]
    assert [f[1] for f in D._fields_] == [C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]
    assert (D.bits_per_symbol.offset, D.fading.offset, D.amp.offset, D.position.offset, D.points.offset) == (0, 4, 8, 16, 24)
    assert C.sizeof(D) == 32
    # ldpc_modulation keeps its layout
    M = _native.ModulationDesc
    assert [f[0] for f in M._fields_] == names[:4] and C.sizeof(M) == 24


def test_new_symbols_are_declared_exported_and_prototyped():
    import _native
    from conftest import PKG
    header = open(_native.HEADER).read()
    lib = _native.load()
    raw = C.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for name in NEW:
        assert name + "(" in header and name in _native.PRODUCT_EXPORTS and hasattr(raw, name)
        assert getattr(lib, name).restype is C.c_int
        assert not hasattr(raw, name + "_dm")                       # every entry point takes the demapper: no twins
    assert [len(getattr(lib, n).argtypes) for n in NEW] == [12, 14, 7, 11]
    # the argument lists are the _dm forms' with the constellation where the modulation stands
    con, mod = C.POINTER(_native.ConstellationDesc), C.POINTER(_native.ModulationDesc)
    for new, old in (("ldpc_channel_con", "ldpc_channel_sym_dm"), ("ldpc_channel_con_mix", "ldpc_channel_sym_mix_dm"),
                     ("ldpc_demap_con", "ldpc_demap_sym"), ("ldpc_simulate_con", "ldpc_simulate_sym_dm")):
        assert [con if a is mod else a for a in getattr(lib, old).argtypes] == list(getattr(lib, new).argtypes), new
    assert lib.ldpc_abi_version() == 1 and "#define LDPC_HIP_ABI_VERSION 1" in header
    assert "ldpc_constellation.hip" in _native.SOURCES
    unit = open(os.path.join(PKG, "csrc", "ldpc_hip.hip")).read()
    assert unit.index('#include "ldpc_modulation.hip"') < unit.index('#include "ldpc_constellation.hip"')
    # the header defines the rule and no longer lists PSK and APSK as missing
    assert "D_c = (tI * tI) + (tQ * tQ)" in header and "logf(S_0) - logf(S_1)" in header
    missing = header[header.index("Not provided: rate matching together with a modulation"):]
    assert "APSK are" not in missing[:missing.index("*/")]
    for proto_of in NEW:
        proto = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\(([^;]*)\);" % proto_of, header).group(1))
        assert "const ldpc_constellation *con" in proto and "int32_t demapper" in proto


# ------------------------------------------------------------------ native argument checks: no device is needed
def test_argument_checks_come_before_any_device():
    import _native
    lib = _native.load()
    tab = np.zeros((64, 2), dtype=np.float32)                       # host memory: never read, the checks look at the address only
    base = tab.ctypes.data
    assert base % 8 == 0

    def con(m=4, fading=0, amp=1.0, points=base):
        return C.byref(_native.ConstellationDesc(bits_per_symbol=m, fading=fading, amp=amp, points=points))

    err = lib.ldpc_last_error
    chan = lambda batch, n, cd, stride=0, dm=0, llr=None, rec=None: lib.ldpc_channel_con(llr, batch, n, 1, 2, 3, cd, None, stride,
                                                                                         rec, dm, None)
    mix = lambda batch, n, cd, stride=0, dm=0, K=3, amp_tab=None, first=3: lib.ldpc_channel_con_mix(
        None, batch, n, 1, 2, first, cd, amp_tab, K, None, stride, None, dm, None)
    dem = lambda batch, n, cd, dm=0, llr=None, rec=None: lib.ldpc_demap_con(llr, batch, n, cd, dm, rec, None)
    for call in (chan, mix, dem):
        assert call(0, 7, con()) == 0                                # an empty block: OK, no pointer looked at
        assert call(-1, 7, con()) == -1 and b"batch" in err()
        assert call(0, 0, con()) == -1 and b"n < 1" in err()
        assert call(0, 7, None) == -1 and b"con" in err()
        for m in (0, 7, 8, -2):
            assert call(0, 7, con(m)) == -1 and b"bits_per_symbol" in err()
        for m in (1, 2, 3, 4, 5, 6):
            assert call(0, 7, con(m)) == 0
        assert call(0, 7, con(points=None)) == -1 and b"NULL points" in err()
        assert call(0, 7, con(points=None), dm=2) == -1 and b"points" in err()                   # points before the demapper
        assert call(0, 7, con(), dm=2) == -1 and b"demapper" in err()
        assert call(0, 7, con(), dm=-1) == -1 and call(0, 7, con(), dm=1) == 0
        assert call(0, 2 ** 29, con(1)) == -3 and b"2^29" in err()                              # S >= 2^29: LDPC_ERR_UNSUPPORTED
        assert call(0, 2 ** 29 - 1, con(1)) == 0 and call(0, 2 ** 30 - 2, con(2)) == 0           # S = 2^29 - 1
        assert call(0, 2 ** 31 - 1, con(3)) == -3 and call(0, 2 ** 31 - 1, con(4)) == -3 and call(0, 2 ** 31 - 1, con(5)) == 0
        assert call(0, 2 ** 29, con(1), dm=2) == -1 and b"demapper" in err()                    # the scalars before S
        assert call(0, 7, con(points=base + 4)) == 0                                             # alignment only after batch == 0
    # fading and amp: the channel looks at both, the mix at fading only, the demapper at neither
    assert chan(0, 7, con(fading=2)) == -1 and b"fading" in err() and mix(0, 7, con(fading=2)) == -1 and dem(0, 7, con(fading=2)) == 0
    for amp in (float("nan"), float("inf"), -1.0):
        assert chan(0, 7, con(amp=amp)) == -1 and b"amp" in err()
        assert mix(0, 7, con(amp=amp)) == 0 and dem(0, 7, con(amp=amp)) == 0
    assert chan(0, 7, con(amp=0.0)) == 0
    assert chan(0, 7, con(points=None, fading=2)) == -1 and b"points" in err()                   # points before fading
    assert chan(0, 7, con(fading=2, amp=-1.0)) == -1 and b"fading" in err()                      # fading before amp
    for call in (chan, mix):
        assert call(0, 7, con(), stride=2) == -1 and b"stride" in err() and call(0, 7, con(), stride=1) == 0
        assert call(0, 7, con(), stride=2, dm=2) == -1 and b"stride" in err()                    # the stride before the demapper
    assert chan(0, 7, con(amp=-1.0), stride=2) == -1 and b"amp" in err()                         # amp before the stride
    for K in (0, -1, 4097):
        assert mix(0, 7, con(), K=K) == -1 and b"n_points" in err()
    assert mix(0, 7, con(), K=4096) == 0
    assert mix(0, 7, con(), K=0, dm=2) == -1 and b"demapper" in err()                            # the demapper before n_points
    assert mix(0, 2 ** 29, con(1), K=0) == -1 and b"n_points" in err()                           # n_points before S
    assert mix(2 ** 31, 7, con()) == -1 and b"2^31" in err()
    assert mix(2, 7, con(), first=2 ** 64 - 1) == -1 and b"wraps" in err()
    assert mix(2, 7, con()) == -1 and b"amp_tab" in err()
    # the pointers, after batch == 0: llr, then received, then the table's alignment
    assert chan(5, 7, con()) == -1 and b"NULL llr" in err()
    assert chan(5, 7, con(), llr=base + 2) == -1 and b"4-byte" in err()
    assert chan(5, 7, con(points=base + 4), llr=base, rec=base + 8) == -1 and b"16-byte" in err()
    assert chan(5, 7, con(points=base + 4), llr=base) == -1 and b"8-byte" in err()
    assert dem(5, 7, con()) == -1 and b"NULL llr" in err()
    assert dem(5, 7, con(), llr=base) == -1 and b"NULL received" in err()
    assert dem(5, 7, con(), llr=base, rec=base + 8) == -1 and b"16-byte" in err()
    assert dem(5, 7, con(points=base + 4), llr=base, rec=base) == -1 and b"8-byte" in err()
    # the one-call point
    out = np.zeros(8, dtype=np.int64)
    desc = _native.SimDesc(max_frames=1, max_errors=1, block=1, poll_blocks=1)
    assert lib.ldpc_simulate_con(None, C.byref(desc), None, con(), 0, -1, _native.ptr(out), None, None, 0, None) == -1
    assert b"NULL decoder" in err()


# ------------------------------------------------------------------ the restatement
def random_samples(table, N, seed):
    """received [1, N, 4]: v around scaled points of the table and far from them, a tenth of the gains zero"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((1, N, 4), dtype=np.float32)
    rec[0, :, 2] = np.where(rng.random(N) < 0.1, 0.0, rng.uniform(0.0, 12.0, N))
    x = np.asarray(table, dtype=np.float64)[rng.integers(0, len(table), N)]
    far = rng.random(N) < 0.2
    for a in (0, 1):
        rec[0, :, a] = np.where(far, rng.uniform(-40, 40, N), rec[0, :, 2] * x[:, a] + rng.normal(size=N))
    return rec


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_fp32_restatement_agrees_with_the_float64_brute_force(m):
    """Both rules, on 4000 random samples: the fp32 restatement against float64 arithmetic on the same fp32 (v, e, table),
    within cref.llr_tolerance (derived there from the roundings of one distance) -- plus, for the exact rule,
    cref.correction_tolerance(m) for the fp32 sums and logs and one ulp for the final addition."""
    con = tables()[m - 1]
    assert con.bits_per_symbol == m
    rec = random_samples(con.points, 4000, 40 + m)
    v = rec[..., 0].astype(np.float64) + 1j * rec[..., 1].astype(np.float64)
    e = rec[..., 2].astype(np.float64)
    tol = cref.llr_tolerance(rec, con.points)[..., None]
    got = cref.demap(rec, con.points)
    want = cref.brute_force_maxlog(v, e, con.points)
    assert got.dtype == np.float32 and got.shape == (1, 4000, m)
    gap = np.abs(got.astype(np.float64) - want)
    print(f"m = {m}: max-log gap {gap.max():.3e} (largest bound {tol.max():.3e}), worst ratio {(gap / np.maximum(tol, 1e-300)).max():.3f}")
    assert (gap <= tol).all()
    clear = np.abs(want) > tol
    assert clear.mean() > 0.7 and np.array_equal(np.sign(got[clear]), np.sign(want[clear]))
    ex = cref.exact(rec, con.points)
    want_ex = cref.brute_force_exact(v, e, con.points)
    tol_ex = tol + cref.correction_tolerance(m) + cref.ulp32(want_ex)
    gap_ex = np.abs(ex.astype(np.float64) - want_ex)
    print(f"m = {m}: exact gap {gap_ex.max():.3e}, worst ratio {(gap_ex / tol_ex).max():.3f}")
    assert np.isfinite(ex).all() and (gap_ex <= tol_ex).all()
    # max-log + float64 correction is the exact rule; the correction is bounded by (m - 1) log 2 and is zero at e = 0
    corr = cref.correction(rec, con.points)
    assert (np.abs(corr) <= (m - 1) * math.log(2.0) + 1e-12).all()
    assert np.abs(got.astype(np.float64) + corr - ex).max() <= cref.correction_tolerance(m) + cref.ulp32(ex).max()
    dead = rec[0, :, 2] == 0
    assert dead.sum() > 100 and (got[0, dead] == 0).all() and (ex[0, dead] == 0).all() and not np.signbit(ex[0, dead]).any()
    if m == 1:
        assert np.array_equal(ex.view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("scheme", ["qpsk", "qam16", "qam64"])
def test_a_qam_table_restates_the_separable_brute_force(scheme):
    """for a QAM table the joint rule is mref.brute_force_maxlog (which works in integer-amplitude units: e' = e d).  The
    table's coordinates are d a rounded to fp32, so e x differs from e d a by 2^-24 relative: the bound is llr_tolerance with
    that one more rounding per coordinate, i.e. computed at twice EPS."""
    from modulation import Constellation, Modulation
    m = mref.SCHEMES[scheme]
    con = Constellation.from_modulation(Modulation(scheme))
    d = mref.half_spacing(m)
    rec = random_samples(con.points, 3000, 7 + m)
    v = rec[..., 0].astype(np.float64) + 1j * rec[..., 1].astype(np.float64)
    want = mref.brute_force_maxlog(v, rec[..., 2].astype(np.float64) * d, m)
    got = cref.demap(rec, con.points).astype(np.float64)
    tol = 2.0 * cref.llr_tolerance(rec, con.points)[..., None]
    assert (np.abs(got - want) <= tol).all()


def test_labels_and_layout_of_the_restatement():
    bits = mref.symbol_bits(np.array([[1, 0, 1, 1, 0, 0, 1]]), 3)       # n = 7, m = 3: three symbols, two pad bits
    assert bits.shape == (1, 3, 3) and cref.labels_of(bits).tolist() == [[5, 1, 1]]
    pos = np.array([6, 5, 4, 3, 2, 1, 0])
    assert cref.labels_of(mref.symbol_bits(np.array([[1, 0, 1, 1, 0, 0, 1]]), 3, pos)).tolist() == [[1, 3, 1]]
    from modulation import Constellation
    tab = Constellation.psk(8).points
    assert np.array_equal(cref.sent_points(tab, bits)[0], tab[[5, 1, 1]]) and cref.bits_of(tab) == 3
    assert np.array_equal(cref.label_bits(3)[5], [1, 0, 1])
    assert [cref.correction_tolerance(m) > cref.correction_tolerance(m - 1) for m in range(2, 7)] == [True] * 5
    assert cref.correction_tolerance(1) == 0.0 and cref.correction_tolerance(6) < 2e-5
