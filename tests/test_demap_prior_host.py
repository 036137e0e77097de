"""
The demapper with a priori LLRs without a device: the new C symbol and its prototype, the native argument checks in their
documented order (none needs a device), the numpy restatement of the rule (tests/demap_prior_reference.py) against
tests/constellation_reference.py at zero priors, against a float64 brute force and in the perfect-prior limit, and what
``SimulationConfig(iterative_demapping=K)`` and ``engine.demap`` refuse before a device is asked for.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import constellation_reference as cref
import demap_prior_reference as pref

NAME = "ldpc_demap_con_prior"


def tables():
    """one table per m = 1 .. 6: psk(2), psk(4), set-partitioned 8-PSK, a set-partitioned 16-point grid, 32-APSK, 64 points"""
    from modulation import Constellation
    return [Constellation.psk(2), Constellation.psk(4), Constellation(pref.sp_psk8(), name="psk8sp"),
            Constellation(pref.sp_qam16(), name="qam16sp"), Constellation.apsk((4, 12, 16), (1.0, 2.64, 4.64)),
            Constellation(pref.random_table(64, 64))]


def samples(table, N, seed, amp_hi=4.0):
    """received [1, N, 4]: v around scaled points of the table, a tenth of the gains zero"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((1, N, 4), dtype=np.float32)
    rec[0, :, 2] = np.where(rng.random(N) < 0.1, 0.0, rng.uniform(0.0, amp_hi, N))
    x = np.asarray(table, dtype=np.float64)[rng.integers(0, len(table), N)]
    for a in (0, 1):
        rec[0, :, a] = rec[0, :, 2] * x[:, a] + rng.normal(size=N)
    return rec


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------ ABI
def test_symbol_is_declared_exported_and_prototyped():
    import _native
    from conftest import PKG
    header = open(_native.HEADER).read()
    lib = _native.load()
    raw = C.CDLL(os.path.join(PKG, "libldpc_hip.so"))
    assert NAME + "(" in header and NAME in _native.PRODUCT_EXPORTS and hasattr(raw, NAME)
    fn = getattr(lib, NAME)
    vp = C.c_void_p
    assert fn.restype is C.c_int and len(fn.argtypes) == 10
    assert list(fn.argtypes) == [vp, C.c_int64, C.c_int32, C.POINTER(_native.ConstellationDesc), C.c_int32, vp, vp, vp,
                                 C.c_float, vp]
    # ldpc_demap_con's list with prior, prior_sub and prior_scale before the stream
    old = list(lib.ldpc_demap_con.argtypes)
    assert list(fn.argtypes) == old[:-1] + [vp, vp, C.c_float] + old[-1:]
    proto = re.sub(r"/\*.*?\*/", "", re.search(r"int %s\(([^;]*)\);" % NAME, header).group(1))
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == ["llr", "batch", "n", "con", "demapper", "received", "prior",
                                                                      "prior_sub", "prior_scale", "stream"]
    assert lib.ldpc_abi_version() == 1 and "#define LDPC_HIP_ABI_VERSION 1" in header          # additive: the ABI stays 1
    # the header defines the rule and no longer lists iterative demapping as missing
    assert "Lam_c = D_c + (2.0f * A_c)" in header and "- La_k" in header and "+-inf and NaN are outside the contract" in header
    block = header[header.index("constellation channel: a table of up to 64"):]
    missing = block[block.index("Not provided:"):]
    assert "iterative demapping" not in missing[:missing.index("*/")]


# ------------------------------------------------------------------ native argument checks: no device is needed
def test_argument_checks_come_in_their_documented_order():
    import _native
    lib = _native.load()
    tab = np.zeros((64, 2), dtype=np.float32)                       # host memory: never read, the checks look at the address only
    base = tab.ctypes.data
    assert base % 8 == 0
    base16 = (base + 15) // 16 * 16

    def con(m=4, fading=0, amp=1.0, points=base):
        return C.byref(_native.ConstellationDesc(bits_per_symbol=m, fading=fading, amp=amp, points=points))

    err = lib.ldpc_last_error
    call = lambda batch, n, cd, dm=0, llr=None, rec=None, prior=None, sub=None, scale=1.0: lib.ldpc_demap_con_prior(
        llr, batch, n, cd, dm, rec, prior, sub, scale, None)
    # ldpc_demap_con's scalars, in its order
    assert call(0, 7, con()) == 0                                    # an empty block: OK, no pointer looked at
    assert call(-1, 7, con()) == -1 and b"batch" in err()
    assert call(-1, 0, con()) == -1 and b"batch" in err()            # batch before n
    assert call(0, 0, con()) == -1 and b"n < 1" in err()
    assert call(0, 0, None) == -1 and b"n < 1" in err()              # n before con
    assert call(0, 7, None) == -1 and b"con" in err()
    for m in (0, 7, 8, -2):
        assert call(0, 7, con(m)) == -1 and b"bits_per_symbol" in err()
    for m in (1, 2, 3, 4, 5, 6):
        assert call(0, 7, con(m)) == 0 and call(0, 7, con(m), dm=1) == 0
    assert call(0, 7, con(points=None)) == -1 and b"NULL points" in err()
    assert call(0, 7, con(points=None), dm=2) == -1 and b"points" in err()                   # points before the demapper
    assert call(0, 7, con(), dm=2) == -1 and b"demapper" in err()
    assert call(0, 7, con(fading=2, amp=-1.0)) == 0                                          # neither is looked at
    # prior_scale: among the scalars, after the demapper, before S and before batch == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(0, 7, con(), scale=bad) == -1 and b"prior_scale" in err()
        assert call(0, 7, con(), dm=2, scale=bad) == -1 and b"demapper" in err()
        assert call(0, 2 ** 29, con(1), scale=bad) == -1 and b"prior_scale" in err()
    for fine in (0.0, -1.0, 0.5, 1e30):
        assert call(0, 7, con(), scale=fine) == 0
    assert call(0, 2 ** 29, con(1)) == -3 and b"2^29" in err()                               # S >= 2^29: LDPC_ERR_UNSUPPORTED
    assert call(0, 2 ** 29 - 1, con(1)) == 0
    assert call(0, 7, con(points=base + 4), prior=base + 2, sub=base + 2) == 0               # pointers only after batch == 0
    # the pointers: llr, received, prior, prior_sub, prior_sub without prior, points
    assert call(5, 7, con()) == -1 and b"NULL llr" in err()
    assert call(5, 7, con(), llr=base + 2) == -1 and b"llr must be 4-byte" in err()
    assert call(5, 7, con(), llr=base, prior=base + 2) == -1 and b"NULL received" in err()   # received before prior
    assert call(5, 7, con(), llr=base, rec=base16 + 8, prior=base + 2) == -1 and b"16-byte" in err()
    assert call(5, 7, con(points=base + 4), llr=base, rec=base16, prior=base + 2, sub=base + 2) == -1
    assert b"prior must be 4-byte" in err()                                                  # prior before prior_sub
    assert call(5, 7, con(points=base + 4), llr=base, rec=base16, prior=base, sub=base + 2) == -1
    assert b"prior_sub must be 4-byte" in err()
    assert call(5, 7, con(points=base + 4), llr=base, rec=base16, sub=base + 2) == -1 and b"prior_sub must be 4-byte" in err()
    assert call(5, 7, con(points=base + 4), llr=base, rec=base16, sub=base) == -1 and b"prior_sub without a prior" in err()
    assert call(5, 7, con(points=base + 4), llr=base, rec=base16, prior=base, sub=base) == -1 and b"8-byte" in err()
    assert call(5, 7, con(points=base + 4), llr=base, rec=base16) == -1 and b"8-byte" in err()   # prior == NULL: the same checks


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_zero_priors_restate_the_rule_without_priors(m):
    """+0.0 and -0.0 priors: Lam_c == D_c exactly, both rules are cref's bit for bit"""
    con = tables()[m - 1]
    assert con.bits_per_symbol == m
    rec = samples(con.points, 2000, 10 + m, amp_hi=12.0)
    for zero in (0.0, -0.0):
        la = np.full((1, 2000, m), zero, dtype=np.float32)
        assert same_bits(pref.metrics(rec, con.points, la), cref.distances(rec, con.points))
        assert same_bits(pref.demap(rec, con.points, la), cref.demap(rec, con.points))
        assert same_bits(pref.exact(rec, con.points, la), cref.exact(rec, con.points))
    # mixed signs of zero too
    la = np.where(np.random.default_rng(m).random((1, 2000, m)) < 0.5, 0.0, -0.0).astype(np.float32)
    assert same_bits(pref.demap(rec, con.points, la), cref.demap(rec, con.points))
    assert same_bits(pref.exact(rec, con.points, la), cref.exact(rec, con.points))


def test_label_sums_follow_the_ascending_order():
    """A_c by the recursion is the sum over the set bits in ascending j starting from 0.0f, rounding for rounding"""
    rng = np.random.default_rng(5)
    la = (rng.normal(size=(50, 6)) * np.array([1e-3, 1.0, 30.0, 1e3, 1.0, 1e-2])).astype(np.float32)
    A = pref.label_sums(la)
    assert A.dtype == np.float32 and A.shape == (50, 64) and (A[:, 0] == 0).all()
    for c in range(64):
        acc = np.zeros(50, dtype=np.float32)
        for j in range(6):
            if (c >> j) & 1:
                acc = (acc + la[:, j]).astype(np.float32)
        assert same_bits(A[:, c], acc), c
    # layout: transmit order through the interleaver, +0.0f at the pad bits
    pos = np.random.default_rng(6).permutation(7)
    flat = np.arange(14, dtype=np.float32).reshape(2, 7) + 1.0
    sym = pref.symbol_priors(flat, 3, pos)
    assert sym.shape == (2, 3, 3) and np.array_equal(sym.reshape(2, 9)[:, :7], flat[:, pos]) and (sym.reshape(2, 9)[:, 7:] == 0).all()
    assert not np.signbit(sym.reshape(2, 9)[:, 7:]).any()
    assert np.array_equal(pref.to_variables(sym, 7, pos), flat)
    assert same_bits(pref.apriori(flat, 0.5 * flat, 0.5), (np.float32(0.5) * (flat - np.float32(0.5) * flat)))


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 6])
def test_fp32_restatement_agrees_with_the_float64_brute_force(m):
    """Both rules on 3000 random samples and priors (normal, sigma 4, a few at +-60): the fp32 restatement against float64
    arithmetic on the same fp32 (v, e, table, La), within pref.llr_tolerance (derived there) -- plus, for the exact rule,
    cref.correction_tolerance(m) and the rounding of its one further addition (pref.exact_tolerance)."""
    con = tables()[m - 1]
    N = 3000
    rec = samples(con.points, N, 40 + m)
    rng = np.random.default_rng(70 + m)
    la = (4.0 * rng.normal(size=(1, N, m))).astype(np.float32)
    spikes = rng.random((1, N, m)) < 0.02
    la[spikes] = np.where(rng.random(int(spikes.sum())) < 0.5, 60.0, -60.0)
    v = rec[..., 0].astype(np.float64) + 1j * rec[..., 1].astype(np.float64)
    e = rec[..., 2].astype(np.float64)
    tol = pref.llr_tolerance(rec, con.points, la)[..., None]
    got = pref.demap(rec, con.points, la)
    want = pref.brute_force_maxlog(v, e, con.points, la)
    assert got.dtype == np.float32 and got.shape == (1, N, m)
    gap = np.abs(got.astype(np.float64) - want)
    print(f"m = {m}: max-log gap {gap.max():.3e} (largest bound {tol.max():.3e}), worst ratio {(gap / tol).max():.3f}")
    assert (gap <= tol).all()
    ex = pref.exact(rec, con.points, la)
    want_ex = pref.brute_force_exact(v, e, con.points, la)
    tol_ex = pref.exact_tolerance(rec, con.points, la)[..., None]
    gap_ex = np.abs(ex.astype(np.float64) - want_ex)
    print(f"m = {m}: exact gap {gap_ex.max():.3e}, worst ratio {(gap_ex / tol_ex).max():.3f}")
    assert np.isfinite(ex).all() and (gap_ex <= tol_ex).all()
    # the exact restatement against its own float64 sums, by the bound the device test uses
    gap_dev = np.abs(ex.astype(np.float64) - pref.exact64(rec, con.points, la))
    assert (gap_dev <= pref.device_exact_tolerance(m, pref.exact64(rec, con.points, la), la)).all()
    if m == 1:
        assert same_bits(ex, got)
    elif m >= 3:
        # the priors are used: the extrinsic LLRs move with the other bits' priors (Gray QPSK's two bits are independent)
        moved = pref.demap(rec, con.points, (la + np.float32(1.0)).astype(np.float32))
        assert np.abs(moved - got).max() > 0.5
    own = la.copy()
    own[..., 0] = own[..., 0] + np.float32(8.0)
    again = pref.demap(rec, con.points, own)
    if m >= 3:
        assert not same_bits(again[..., 1:], got[..., 1:])
    # ... both are within their bounds of the same float64 value, which does not depend on the bit's own prior
    assert (np.abs(again[..., 0].astype(np.float64) - got[..., 0]) <= tol[..., 0] + pref.llr_tolerance(rec, con.points, own)).all()


@pytest.mark.parametrize("m", [2, 3, 4, 5, 6])
def test_perfect_priors_leave_the_two_labels_that_differ_in_one_bit(m):
    """La_j = +-40 on the other bits, agreeing with one label, and 0 on bit k: bit k's LLR is 0.5 (D_c1 - D_c0) of the two
    labels that differ in bit k only.  Max-log: within pref.llr_tolerance, as long as no candidate with a wrong bit wins a
    minimum -- a wrong bit costs 80 in Lam, so that holds where the spread of D is below 80 (asserted).  Exact: the
    candidates with wrong bits add at most (2^(m-1) - 1) exp(-(80 - spread) / 2) to either sum, hence to either log."""
    con = tables()[m - 1]
    N = 400
    rec = samples(con.points, N, 90 + m, amp_hi=1.5)
    rng = np.random.default_rng(95 + m)
    D64 = cref._distances64(rec[..., 0].astype(np.float64) + 1j * rec[..., 1].astype(np.float64), rec[..., 2].astype(np.float64),
                            con.points)
    spread = D64.max(axis=-1) - D64.min(axis=-1)
    assert spread.max() < 70.0
    label = rng.integers(0, 2 ** m, size=(1, N))
    bits = (label[..., None] >> np.arange(m)) & 1
    for k in range(m):
        la = np.where(bits == 1, -40.0, 40.0).astype(np.float32)
        la[..., k] = 0.0
        c0, c1 = label & ~(1 << k), label | (1 << k)
        want = 0.5 * (np.take_along_axis(D64, c1[..., None], -1) - np.take_along_axis(D64, c0[..., None], -1))[..., 0]
        tol = pref.llr_tolerance(rec, con.points, la)
        got = pref.demap(rec, con.points, la)[..., k].astype(np.float64)
        assert (np.abs(got - want) <= tol).all(), k
        ex = pref.exact(rec, con.points, la)[..., k].astype(np.float64)
        tail = (2 ** (m - 1) - 1) * np.exp(-0.5 * (80.0 - spread))
        assert (np.abs(ex - want) <= pref.exact_tolerance(rec, con.points, la) + 2.0 * tail).all(), k


def test_the_shared_iterative_case_has_the_classes_it_was_chosen_for():
    """tests/decode_iterative_cases.restate -- channel restatement, rule restatement, oracle decoder, all on the CPU -- at the
    committed seed and Es/N0: 18 frames close in round 1, 24 in a later round, 25 never.  The GPU test asserts at least
    MIN_PER_CLASS of each on the device's own result; this keeps the choice reproducible."""
    import decode_iterative_cases as dc
    closed, iters = dc.restate()
    assert closed.shape == iters.shape == (dc.BATCH,)
    counts = (int((closed == 1).sum()), int((closed > 1).sum()), int((closed == 0).sum()))
    assert counts == (18, 24, 25) and min(counts) >= 5 * dc.MIN_PER_CLASS
    assert int(iters.sum()) == 1233 and (iters[closed == 0] == dc.ROUNDS * dc.T).all()
    # without feedback (the same LLRs decoded again) no frame could close after round 1: the later class is the feedback's
    never_fed, _ = dc.restate(rounds=1)
    assert int((never_fed == 1).sum()) == counts[0]


# ------------------------------------------------------------------ refusals before any device
def test_simulation_config_refuses_iterative_demapping_it_cannot_run():
    import dataclasses
    from modulation import Constellation, Modulation
    from simulation_framework import SimulationConfig
    psk8 = Constellation(pref.sp_psk8())
    cfg = SimulationConfig()
    assert cfg.iterative_demapping == 1 and cfg.demapping_feedback_scale == 1.0
    assert len(dataclasses.fields(SimulationConfig)) == 20                                   # init-only, as `modulation` is
    one = SimulationConfig(channel="device", codeword="random", modulation=psk8, iterative_demapping=1, diagnostics=True,
                           capture_errors=3)
    assert one.iterative_demapping == 1                                                      # K = 1 builds as today
    assert SimulationConfig(iterative_demapping=1).channel == "torch"
    ok = SimulationConfig(channel="device", codeword="random", modulation=psk8, iterative_demapping=4,
                          demapping_feedback_scale=0.75)
    assert ok.iterative_demapping == 4 and ok.demapping_feedback_scale == 0.75 and ok.modulation is psk8
    with pytest.raises(ValueError, match="Constellation"):
        SimulationConfig(channel="device", iterative_demapping=2)                            # no constellation
    with pytest.raises(ValueError, match="Constellation"):
        SimulationConfig(iterative_demapping=2)
    with pytest.raises(ValueError, match="from_modulation"):
        SimulationConfig(channel="device", codeword="random", modulation=Modulation("qam16"), iterative_demapping=2)
    with pytest.raises(ValueError, match="diagnostics"):
        SimulationConfig(channel="device", codeword="random", modulation=psk8, iterative_demapping=2, diagnostics=True)
    with pytest.raises(ValueError, match="capture_errors"):
        SimulationConfig(channel="device", codeword="random", modulation=psk8, iterative_demapping=2, capture_errors=1)
    for bad in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError, match="iterative_demapping"):
            SimulationConfig(channel="device", codeword="random", modulation=psk8, iterative_demapping=bad)
    for bad in (float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="demapping_feedback_scale"):
            SimulationConfig(channel="device", codeword="random", modulation=psk8, iterative_demapping=2,
                             demapping_feedback_scale=bad)


def test_engine_demap_checks_its_new_keywords_before_a_device_is_asked_for():
    import torch
    import engine
    from modulation import Constellation, Modulation
    con = Constellation(pref.sp_psk8())
    rec = torch.zeros((2, 32, 4), dtype=torch.float32)
    good = torch.zeros((2, 96), dtype=torch.float32)
    with pytest.raises(ValueError, match="from_modulation"):
        engine.demap(torch.zeros((2, 24, 4)), 96, modulation=Modulation("qam16"), prior=good)
    with pytest.raises(ValueError, match="prior_sub without a prior"):
        engine.demap(rec, 96, modulation=con, prior_sub=good)
    for bad in (float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="prior_scale"):
            engine.demap(rec, 96, modulation=con, prior=good, prior_scale=bad)
    with pytest.raises(ValueError, match="prior_scale without a prior"):
        engine.demap(rec, 96, modulation=con, prior_scale=0.5)
    for name in ("prior", "prior_sub", "out"):
        for bad in (good.numpy(), good.double(), good[:, :95], good[:1], good.t().contiguous().t(), torch.zeros((2, 96, 1))):
            kw = {"prior": good, name: bad}
            with pytest.raises(ValueError, match=name + " must be"):
                engine.demap(rec, 96, modulation=con, **kw)
    with pytest.raises(ValueError, match="GPU"):                                             # everything in order: now the device
        engine.demap(rec, 96, modulation=con, prior=good, prior_sub=good, prior_scale=0.5, out=good)
    assert engine.DecodeResult(None, None, good, good).rounds is None                       # the new field is optional
    assert [f.name for f in __import__("dataclasses").fields(engine.DecodeResult)][-1] == "rounds"
    assert hasattr(engine.DecodeEngine, "decode_iterative")
    assert math.isfinite(cref.correction_tolerance(6))
