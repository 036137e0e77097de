"""
The exact demapper without a device: the fp32 restatement of the rule (tests/demap_reference.py) against a brute-force float64
log-sum-exp over all 2^m constellation points, the properties of the rule (h = 1 is max-log, the bounded correction, finite at
high SNR, erasures, oddness), Modulation(demapper=) and normalise_received, and the four new C symbols.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import demap_reference as dref
import modulation_reference as mref

ALL_M = (1, 2, 4, 6, 8)
F32 = np.float32


def d_rounding(v, e, h):
    """float64 [...]: a bound on the error of any fp32 distance D(a') of the axis against the exact (v - e a')^2, from the
    three roundings that form it (each at most 2^-24 of its result): ec = fl(e a') is off by 2^-24 |ec|, t = fl(v - ec) by
    that plus 2^-24 |t|, D = fl(t t) by 2 |t| times that plus 2^-24 t^2 (second-order terms, 2^-48, are covered by the factor
    1.01):  |dD| <= 2^-24 (3 t^2 + 2 |t| |ec|), the largest over the axis' levels"""
    L = 2 ** h
    amps = ((L - 1) - 2 * np.arange(L)).astype(np.float64)
    ec = np.asarray(e, np.float64)[..., None] * amps
    t = np.asarray(v, np.float64)[..., None] - ec
    return 1.01 * 2.0 ** -24 * (3.0 * t * t + 2.0 * np.abs(t) * np.abs(ec)).max(axis=-1)


@pytest.mark.parametrize("m", ALL_M)
def test_restated_exact_rule_equals_brute_force_log_sum_exp(m):
    """exp(-|v - e x|^2 / 2) factors over the axes and a bit's two sets differ on its own axis only, so the joint log-MAP LLR
    is the axis' own; and log sum exp(-D / 2) = -m_b / 2 + log S_b whatever m_b is.  What is left is rounding.  An LLR is
    log sum_0 - log sum_1 and d(log sum exp(-D / 2)) / dD_c = -w_c / 2 with weights w_c summing to 1, so distances off by dD
    move each log-sum by at most dD / 2 and the LLR by at most dD: TOL = d_rounding (the fp32 rounding of D, derived above)
    of the sample.  On top of it come only the roundings of the fp32 arithmetic after D, which no demapper in fp32 escapes:
    dref.correction_tolerance(h) for the sums and logs and one ulp each for 0.5f * (m1 - m0) and the final sum."""
    h = mref.axis_bits(m)
    rng = np.random.default_rng(200 + m)
    N = 3000
    v = (rng.uniform(-40, 40, N) + 1j * rng.uniform(-40, 40, N)) * (rng.random(N) < 0.9)
    e = np.where(rng.random(N) < 0.1, 0.0, rng.uniform(0.0, 4.0, N))
    rec = np.zeros((1, N, 4), dtype=F32)
    rec[0, :, 0], rec[0, :, 2] = v.real, e
    if m > 1:
        rec[0, :, 1] = v.imag
    got = dref.exact(rec, m)[0]
    assert got.dtype == F32 and got.shape == (N, m)
    v64 = rec[0, :, 0].astype(np.float64) + 1j * rec[0, :, 1].astype(np.float64)
    want = dref.brute_force_exact(v64, rec[0, :, 2].astype(np.float64), m)
    tol = np.empty((N, m))
    tol[:, :h] = d_rounding(rec[0, :, 0], rec[0, :, 2], h)[:, None]
    if m > 1:
        tol[:, h:] = d_rounding(rec[0, :, 1], rec[0, :, 2], h)[:, None]
    tol = tol + dref.correction_tolerance(h) + 2.0 * dref.ulp32(want)
    err = np.abs(got.astype(np.float64) - want)
    print(f"m = {m}: max |fp32 rule - brute force| = {err.max():.3e}, max over its bound = {(err / tol).max():.3f}")
    assert (err <= tol).all()
    # and the brute force is not max-log: from 16-QAM up the correction is there
    if m >= 4:
        assert np.abs(want - mref.brute_force_maxlog(v64, rec[0, :, 2].astype(np.float64), m)).max() > 0.5


@pytest.mark.parametrize("h", [1, 2, 3, 4])
def test_properties_of_the_exact_rule(h):
    rng = np.random.default_rng(300 + h)
    N = 20000
    L = 2 ** h
    e = rng.uniform(0.0, 8.0, N).astype(F32)
    v = (e * rng.choice((L - 1) - 2 * np.arange(L), N) + rng.standard_normal(N) * rng.choice([1.0, 3.0], N)).astype(F32)
    ex, ml = dref.exact_axis(v, e, h), mref.demap_axis(v, e, h)
    assert ex.dtype == F32 and ex.shape == (N, h) and np.isfinite(ex).all()
    if h == 1:
        assert np.array_equal(ex.view(np.int32), ml.view(np.int32))                   # bit for bit, signed zeros included
    # |exact - maxlog| <= log(L / 2): both sums lie in [1, L / 2].  Rounding: the correction's own and the final sum's ulp
    bound = np.log(L / 2) + dref.correction_tolerance(h) + dref.ulp32(ex)
    assert (np.abs(ex.astype(np.float64) - ml.astype(np.float64)) <= bound).all()
    if h >= 2:
        assert np.abs(ex - ml).max() > 0.3                                             # and it is not max-log
    # the float64 correction from the same distances: the fp32 arithmetic stays within the derived bound
    c64 = dref.correction64(v, e, h)
    err = np.abs(ex.astype(np.float64) - (ml.astype(np.float64) + c64))
    assert (err <= dref.correction_tolerance(h) + dref.ulp32(ex)).all(), err.max()
    # finite at e up to 8 * 15 (amp = 8 under a deep fade's opposite, the far corner): the per-set form never reaches log(0)
    big = np.array([8.0 * 15.0, 100.0, 64.0, 8.0], dtype=F32)
    for a in ((L - 1), -(L - 1), 1):
        far = dref.exact_axis((big * a + F32(6.76)).astype(F32), big, h)
        assert np.isfinite(far).all() and (far != 0).all()
    # e = 0: every distance equal, +0.0 (an erasure), sign bit clear
    zero = dref.exact_axis(v[:100], np.zeros(100, F32), h)
    assert np.array_equal(zero.view(np.int32), np.zeros((100, h), np.int32))
    # reflection v -> -v mirrors the levels (c -> L - 1 - c), which flips b_0 and keeps every other bit: the b_0 LLR is odd.
    # D(-v, c) = D(v, L - 1 - c) exactly in fp32 (a sign flip rounds the same) and the minima with it; the sums run in
    # opposite orders, so the corrections agree to their bound and not bit for bit
    refl = dref.exact_axis(-v, e, h)
    assert (np.abs(refl[:, 0].astype(np.float64) + ex[:, 0].astype(np.float64))
            <= 2 * dref.correction_tolerance(h) + 2 * dref.ulp32(ex[:, 0])).all()
    if h == 1:
        assert np.array_equal((-refl[:, 0])[ex[:, 0] != 0], ex[:, 0][ex[:, 0] != 0])


def test_a_globally_normalised_form_would_underflow_and_the_definition_does_not():
    """256-QAM axis at e = 8, v at the positive corner: the b_0 = 1 set lies 8 * 2 or more away, exp(-D / 2) underflows in
    fp32 when normalised by the global minimum, and the per-set form returns the finite answer"""
    v, e = np.array([8.0 * 15.0], F32), np.array([8.0], F32)
    D = dref.distances(v, e, 4)[0]
    labels = mref.level_labels(4)
    glob = np.exp((F32(-0.5) * (D - D.min())).astype(F32))
    assert glob[labels[:, 0] == 1].sum() == 0.0                                      # logf of it: -inf
    out = dref.exact_axis(v, e, 4)
    assert np.isfinite(out).all() and out[0, 0] > 0


@pytest.mark.parametrize("scheme,m", sorted(mref.SCHEMES.items(), key=lambda kv: kv[1]))
def test_normalise_received_gives_a_received_block_back(scheme, m):
    """y = h x + noise built from a block's own (v, e) in double: e = |h| d / sigma and v = e a + z, so with sigma and a phase
    chosen freely y = sigma e^{j phi} (vI + j vQ) / 1 and h = sigma e / d e^{j phi}.  normalise_received undoes it in double
    and casts: the block comes back within a few float64 roundings of values of size |v| plus the cast, 2^-24 relative."""
    import torch
    from modulation import Modulation, half_spacing
    rng = np.random.default_rng(400 + m)
    B, S = 3, 41
    rec = np.zeros((B, S, 4), dtype=F32)
    rec[..., 2] = rng.uniform(0.05, 5.0, (B, S))
    rec[..., 0] = rng.uniform(-30, 30, (B, S))
    if m > 1:
        rec[..., 1] = rng.uniform(-30, 30, (B, S))
    rec[0, 0, 2] = 0.0                                                                # a dead symbol: |h| = 0
    mod = Modulation(scheme)
    d = half_spacing(m)
    for kw, n0 in (({"snr_db": 7.0}, 10.0 ** -0.7), ({"noise_var": 0.31}, 0.31)):
        sigma = np.sqrt(n0) if m == 1 else np.sqrt(n0 / 2.0)
        phi = rng.uniform(-np.pi, np.pi, (B, S))
        phi[0, 0] = 0.0                                                               # |h| = 0: v = y / sigma, no rotation
        rot = np.exp(1j * phi)
        v = rec[..., 0].astype(np.float64) + 1j * rec[..., 1].astype(np.float64)
        y = sigma * v * rot
        h = (sigma * rec[..., 2].astype(np.float64) / d) * rot
        got = mod.normalise_received(torch.from_numpy(y), torch.from_numpy(h), **kw)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (B, S, 4)
        got = got.numpy()
        tol = 2.0 ** -23 * np.maximum(np.abs(rec), 1.0) + 1e-12
        assert (np.abs(got.astype(np.float64) - rec.astype(np.float64)) <= tol).all()
        assert (got[..., 3] == 0).all() and got[0, 0, 2] == 0 and (m > 1 or (got[..., 1] == 0).all())
    # gain None is h = 1; arrays are taken as well as tensors
    one = mod.normalise_received(np.array([[1.0 + 0.5j]]), snr_db=0.0).numpy()
    sig = 1.0 if m == 1 else np.sqrt(0.5)
    assert one[0, 0, 0] == F32(1.0 / sig) and one[0, 0, 2] == F32(d / sig) and one[0, 0, 1] == (0 if m == 1 else F32(0.5 / sig))
    for bad in ({}, {"snr_db": 1.0, "noise_var": 0.5}):
        with pytest.raises(ValueError, match="exactly one"):
            mod.normalise_received(np.zeros((1, 1), complex), **bad)
    with pytest.raises(ValueError):
        mod.normalise_received(np.zeros((1, 1), complex), noise_var=0.0)
    with pytest.raises(ValueError):
        mod.normalise_received(np.zeros((2, 3), complex), np.ones((2, 2)), snr_db=1.0)
    with pytest.raises(ValueError):
        mod.normalise_received(np.zeros(3, complex), snr_db=1.0)


def test_modulation_takes_a_demapper_and_keeps_its_default_repr():
    from modulation import DEMAPPERS, Modulation
    assert DEMAPPERS == {"maxlog": 0, "exact": 1}
    assert Modulation("qam16").demapper == "maxlog" and Modulation("qam16", demapper="exact").demapper == "exact"
    assert Modulation("qam64", "rayleigh", None, "exact").demapper == "exact"
    for bad in ("logmap", "EXACT", "", None, 1, True):
        with pytest.raises(ValueError, match="demapper"):
            Modulation("qam16", demapper=bad)
    assert repr(Modulation("qam16")) == "Modulation('qam16', fading=None, interleaver=None)"
    assert repr(Modulation("qpsk", "rayleigh", [1, 0, 2])) == "Modulation('qpsk', fading='rayleigh', interleaver=<permutation of 3>)"
    assert repr(Modulation("qam16", demapper="exact")) == "Modulation('qam16', fading=None, interleaver=None, demapper='exact')"


NEW = ("ldpc_demap_sym", "ldpc_channel_sym_dm", "ldpc_channel_sym_mix_dm", "ldpc_simulate_sym_dm")


def test_new_symbols_are_declared_exported_and_prototyped():
    import _native
    from conftest import PKG
    header = open(_native.HEADER).read()
    lib = _native.load()
    raw = C.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    for name in NEW:
        assert name + "(" in header and name in _native.PRODUCT_EXPORTS and hasattr(raw, name)
        assert getattr(lib, name).restype is C.c_int
    # each _dm form is its counterpart with one int32 more: before the stream, and before `capture` in the simulate form
    i32 = C.c_int32
    for base, at in (("ldpc_channel_sym", -2), ("ldpc_channel_sym_mix", -2), ("ldpc_simulate_sym", 4)):
        old, new = list(getattr(lib, base).argtypes), list(getattr(lib, base + "_dm").argtypes)
        at = at % (len(old) + 1)
        assert new[:at] + new[at + 1:] == old and new[at] is i32, base
    assert [len(getattr(lib, n).argtypes) for n in NEW] == [7, 12, 14, 11]
    assert lib.ldpc_demap_sym.argtypes[4] is i32
    assert lib.ldpc_abi_version() == 1 and "#define LDPC_HIP_ABI_VERSION 1" in header
    assert re.search(r"enum \{ LDPC_DEMAP_MAXLOG = 0, LDPC_DEMAP_EXACT = 1 \};", header)
    assert (_native.DEMAP_MAXLOG, _native.DEMAP_EXACT) == (0, 1)
    # the header defines the exact rule and no longer lists it as missing
    assert "expf(-0.5f * (D(a') - m_b))" in header and "logf(S_0) - logf(S_1)" in header
    missing = header[header.index("Not provided: rate matching together with a modulation"):]
    assert "log-sum-exp" not in missing[:missing.index("*/")]
    # the prototypes in the header carry the argument where the loader puts it
    proto = re.search(r"int ldpc_simulate_sym_dm\(([^;]*)\);", header).group(1)
    assert re.search(r"const ldpc_modulation \*mod, int32_t demapper, int64_t capture", proto)
    for name in ("ldpc_channel_sym_dm", "ldpc_channel_sym_mix_dm"):
        proto = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\(([^;]*)\);" % name, header).group(1))
        assert re.search(r"int32_t demapper,\s*void \*stream$", proto.strip())


def test_demap_refuses_before_a_device_is_asked_for():
    """shape, dtype, contiguity and device of `received` and the demapper's name: all checked on the host"""
    import torch
    import engine
    from modulation import Modulation
    mod = Modulation("qam16")
    good = torch.zeros((2, 24, 4), dtype=torch.float32)
    for bad in (good.numpy(), good.double(), good[:, :, :3], good[:, :23], good.transpose(0, 1), good.reshape(2, 96),
                torch.zeros((2, 24, 8), dtype=torch.float32)[:, :, ::2]):
        with pytest.raises(ValueError, match="received"):
            engine.demap(bad, 96, modulation=mod)
    with pytest.raises(ValueError, match="demapper"):
        engine.demap(good, 96, modulation=mod, demapper="logmap")
    with pytest.raises(ValueError, match="modulation"):
        engine.demap(good, 96, modulation="qam16")
    with pytest.raises(ValueError, match="n must"):
        engine.demap(good, 0, modulation=mod)
    with pytest.raises(ValueError, match="GPU"):                                      # a host tensor: refused, not copied
        engine.demap(good, 96, modulation=mod)
