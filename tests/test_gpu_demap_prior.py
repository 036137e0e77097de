"""
GPU tests (-m gpu) of the demapper with a priori LLRs (ldpc_demap_con_prior through engine.demap(prior=...)) against the numpy
restatement of its definition (tests/demap_prior_reference.py): zero priors against engine.demap without them, random finite
priors bit for bit under the max-log rule and within the derived bound under the exact one, prior_sub / prior_scale against
tensors formed by torch, in-place operation, and guard rows around the output.  Tables of 2, 4, 8, 16, 32 and 64 points
(m = 1 .. 6), n in {1, 7, 96} x batch in {1, 3, 67}, identity and a random interleaver: n = 7 with m = 3 and n = 1 have pad
bits, batch 67 at n = 96 spans more than one workgroup.
"""
import numpy as np
import pytest
import torch

import constellation_reference as cref
import demap_prior_reference as pref

pytestmark = pytest.mark.gpu

SEED, STREAM, FIRST = 0x51ed270b3c6ef372, 5100, 2 ** 32 - 30
NS, BATCHES = (1, 7, 96), (1, 3, 67)
TABLES = ("psk2", "psk4", "psk8sp", "qam16sp", "apsk32", "rand64")               # m = 1 .. 6
RULES = ("maxlog", "exact")
# (amp, fading): weak and strong samples, one fading case
DRAWS = ((0.6, None), (1.7, None), (1.7, "rayleigh"))


def table(name, fading=None, pos=None):
    from modulation import Constellation
    kw = dict(fading=fading, interleaver=pos, name=name)
    if name.startswith("psk") and name[3:].isdigit():
        return Constellation.psk(int(name[3:]), **kw)
    if name == "psk8sp":
        return Constellation(pref.sp_psk8(), **kw)
    if name == "qam16sp":
        return Constellation(pref.sp_qam16(), **kw)
    if name == "apsk32":
        return Constellation.apsk((4, 12, 16), (1.0, 2.64, 4.64), **kw)
    return Constellation(pref.random_table(64, 64), **kw)


def received(batch, n, con, amp, dev):
    """the samples of random codeword rows through the device channel"""
    import engine
    bits = (np.random.default_rng(n * 131 + batch).random((batch, n)) < 0.5).astype(np.uint8)
    rows = torch.from_numpy(np.packbits(bits, axis=1, bitorder="little")).to(dev)
    _, rec = engine.sym_llr(batch, n, seed=SEED, stream_id=STREAM, first_frame=FIRST, amp=amp, codeword=rows, device=dev,
                            modulation=con, want_received=True)
    return rec


def priors(batch, n, seed):
    """normal, sigma = 4, with a few entries at +-60"""
    rng = np.random.default_rng(seed)
    p = (4.0 * rng.normal(size=(batch, n))).astype(np.float32)
    spikes = rng.random((batch, n)) < 0.05
    p[spikes] = np.where(rng.random(int(spikes.sum())) < 0.5, 60.0, -60.0)
    return p


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def cases(n):
    """(table name, interleaver or None, amp, fading)"""
    pos = np.random.default_rng(n + 1).permutation(n)
    for name in TABLES:
        for i, (amp, fading) in enumerate(DRAWS):
            yield name, (pos if i != 0 else None), amp, fading


# ------------------------------------------------------------------ 1. zero priors
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_zero_priors_are_the_demapper_without_priors(batch, n, gpu_device):
    """prior=None (with an `out`), +0.0 and -0.0 priors: engine.demap(received) bit for bit under both rules"""
    import engine
    for name, pos, amp, fading in cases(n):
        con = table(name, fading, pos)
        rec = received(batch, n, con, amp, gpu_device)
        for rule in RULES:
            want = engine.demap(rec, n, modulation=con, demapper=rule).cpu().numpy()
            out = torch.full((batch, n), 7.0, dtype=torch.float32, device=gpu_device)
            got = engine.demap(rec, n, modulation=con, demapper=rule, out=out)
            assert got is out and same_bits(out.cpu().numpy(), want), (name, rule)
            for zero in (0.0, -0.0):
                z = torch.full((batch, n), zero, dtype=torch.float32, device=gpu_device)
                assert same_bits(engine.demap(rec, n, modulation=con, demapper=rule, prior=z).cpu().numpy(), want), (name, rule, zero)
                assert same_bits(engine.demap(rec, n, modulation=con, demapper=rule, prior=z, prior_sub=z,
                                              prior_scale=-3.0).cpu().numpy(), want), (name, rule, zero)


# ------------------------------------------------------------------ 2. random finite priors
WORST = {}


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_random_priors_against_the_restatement(batch, n, gpu_device):
    """max-log: the numpy restatement bit for bit.  exact: within pref.device_exact_tolerance of the restated value with
    float64 sums -- cref.correction_tolerance(m) for expf, logf and the sums, one ulp each for the final add and subtract
    (derived beside the constant).  The largest error over its bound is printed per m."""
    import engine
    for name, pos, amp, fading in cases(n):
        con = table(name, fading, pos)
        m = con.bits_per_symbol
        rec_t = received(batch, n, con, amp, gpu_device)
        rec = rec_t.cpu().numpy()
        p = priors(batch, n, n * 7 + batch)
        la = pref.symbol_priors(p, m, pos)
        p_t = torch.from_numpy(p).to(gpu_device)
        got = engine.demap(rec_t, n, modulation=con, demapper="maxlog", prior=p_t).cpu().numpy()
        assert same_bits(got, pref.to_variables(pref.demap(rec, con.points, la), n, pos)), (name, amp, fading)
        ex = engine.demap(rec_t, n, modulation=con, demapper="exact", prior=p_t).cpu().numpy()
        assert np.isfinite(ex).all()
        if m == 1:
            assert same_bits(ex, got)
            continue
        want = pref.to_variables(pref.exact64(rec, con.points, la), n, pos)
        tol = pref.device_exact_tolerance(m, want, p)
        gap = np.abs(ex.astype(np.float64) - want)
        ratio = float((gap / tol).max())
        WORST[m] = max(WORST.get(m, 0.0), ratio)
        print(f"{name} amp {amp} {fading} batch {batch} n {n}: exact max gap {gap.max():.3e}, worst ratio {ratio:.3f} "
              f"(worst so far for m = {m}: {WORST[m]:.3f})")
        assert (gap <= tol).all(), (name, amp, fading)
        if m >= 3 and n >= 2 * m and batch * n >= 50:
            # the priors matter (not for Gray QPSK, whose bits are independent; not with n = 1, whose symbol has one real
            # bit) and so does the correction
            plain = engine.demap(rec_t, n, modulation=con, demapper="maxlog").cpu().numpy()
            assert np.abs(got - plain).max() > 0.5 and np.abs(ex - got).max() > 0.05


# ------------------------------------------------------------------ 3. prior_sub, prior_scale, in place, guards
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_prior_sub_scale_in_place_and_guards(batch, n, gpu_device):
    import engine
    for name, pos, amp, fading in cases(n):
        con = table(name, fading, pos)
        rec = received(batch, n, con, amp, gpu_device)
        p = torch.from_numpy(priors(batch, n, n * 11 + batch)).to(gpu_device)
        q = torch.from_numpy(priors(batch, n, n * 13 + batch + 1)).to(gpu_device)
        for rule in RULES:
            kw = dict(modulation=con, demapper=rule)
            # prior - prior_sub formed in the kernel is the fp32 difference torch forms
            want = engine.demap(rec, n, prior=p - q, **kw).cpu().numpy()
            assert same_bits(engine.demap(rec, n, prior=p, prior_sub=q, **kw).cpu().numpy(), want), (name, rule)
            # ... and the scale is one fp32 product
            half = engine.demap(rec, n, prior=0.5 * p, **kw).cpu().numpy()
            assert same_bits(engine.demap(rec, n, prior=p, prior_scale=0.5, **kw).cpu().numpy(), half), (name, rule)
            third = engine.demap(rec, n, prior=(p - q) * np.float32(0.3), **kw).cpu().numpy()
            assert same_bits(engine.demap(rec, n, prior=p, prior_sub=q, prior_scale=0.3, **kw).cpu().numpy(), third), (name, rule)
            if con.bits_per_symbol >= 3 and n >= 2 * con.bits_per_symbol and batch * n >= 50:
                assert not same_bits(want, half)
            # in place: out = prior_sub, and out = prior
            sub = q.clone()
            assert engine.demap(rec, n, prior=p, prior_sub=sub, out=sub, **kw) is sub
            assert same_bits(sub.cpu().numpy(), want), (name, rule, "out=prior_sub")
            pri = p.clone()
            engine.demap(rec, n, prior=pri, prior_sub=q, out=pri, **kw)
            assert same_bits(pri.cpu().numpy(), want), (name, rule, "out=prior")
            # guard rows before and after the output keep their fill: nothing is written past column n of any row
            buf = torch.full((batch + 2, n), -77.25, dtype=torch.float32, device=gpu_device)
            engine.demap(rec, n, prior=p, prior_sub=q, out=buf[1:-1], **kw)
            host = buf.cpu().numpy()
            assert (host[0] == -77.25).all() and (host[-1] == -77.25).all() and same_bits(host[1:-1], want), (name, rule)
            # p and q are untouched by the out-of-place calls
        assert same_bits(p.cpu().numpy(), priors(batch, n, n * 11 + batch))


@pytest.mark.parametrize("name", ["psk2", "psk8sp", "rand64"])
def test_a_null_prior_through_the_entry_point_is_the_demapper_without_priors(name, gpu_device):
    """ldpc_demap_con_prior with prior == NULL launches ldpc_demap_con's kernel: called through ctypes (engine.demap goes to
    ldpc_demap_con itself when it has no prior), both rules, with an interleaver, any finite prior_scale"""
    import ctypes as C
    import _native
    import engine
    from modulation import DEMAPPERS
    batch, n = 67, 96
    con = table(name, None, np.random.default_rng(3).permutation(n))
    rec = received(batch, n, con, 1.7, gpu_device)
    desc, _keep = con.native(0.0, n, gpu_device)
    lib = _native.load()
    for rule in RULES:
        want = engine.demap(rec, n, modulation=con, demapper=rule)
        for scale in (1.0, -2.5):
            out = torch.full((batch, n), 7.0, dtype=torch.float32, device=gpu_device)
            with torch.cuda.device(gpu_device):
                stream = torch.cuda.current_stream(gpu_device).cuda_stream
                rc = lib.ldpc_demap_con_prior(C.c_void_p(out.data_ptr()), batch, n, C.byref(desc), DEMAPPERS[rule],
                                              C.c_void_p(rec.data_ptr()), None, None, scale, C.c_void_p(stream))
            assert rc == 0 and same_bits(out.cpu().numpy(), want.cpu().numpy()), (name, rule, scale)


def test_what_the_entry_point_refuses_on_the_device(gpu_device):
    import engine
    con = table("psk8sp")
    rec = received(3, 7, con, 1.0, gpu_device)
    p = torch.zeros((3, 7), dtype=torch.float32, device=gpu_device)
    with pytest.raises(ValueError, match="prior must be"):
        engine.demap(rec, 7, modulation=con, prior=p.cpu())
    with pytest.raises(ValueError, match="out must be"):
        engine.demap(rec, 7, modulation=con, prior=p, out=torch.zeros((3, 8), dtype=torch.float32, device=gpu_device)[:, :7])
    from modulation import Modulation
    qam = Modulation("qam16")
    rq = torch.zeros((3, 2, 4), dtype=torch.float32, device=gpu_device)
    with pytest.raises(ValueError, match="from_modulation"):
        engine.demap(rq, 7, modulation=qam, prior=p)
    assert engine.demap(rq, 7, modulation=qam, out=p) is p                                   # `out` alone is fine everywhere
