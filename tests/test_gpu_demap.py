"""
GPU tests (-m gpu) of the device soft demapper (ldpc_demap_sym, engine.demap) and of the exact rule in the channel kernels
(ldpc_channel_sym_dm, ldpc_channel_sym_mix_dm): the standalone max-log demap against the channel call that wrote the samples,
the exact rule against the restatement (tests/demap_reference.py) within a derived bound, fused against standalone, BPSK and
QPSK, the bounded correction, guard words at every store alignment and what the entry point refuses.
Shapes are those of tests/test_gpu_channel_sym.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import demap_reference as dref
import encode_reference as eref
import modulation_reference as mref

pytestmark = pytest.mark.gpu

SEED, STREAM = 0x9e3779b97f4a7c15, 4700
FIRST = 2 ** 32 - 30                                  # 67 frames cross into the high counter word
NS, BATCHES = (1, 7, 96, 1998), (1, 3, 67)
SCHEMES = tuple(sorted(mref.SCHEMES.items(), key=lambda kv: kv[1]))          # (name, m), m = 1, 2, 4, 6, 8
QAM = tuple(sm for sm in SCHEMES if sm[1] >= 4)
FADINGS = (None, "rayleigh")
# |device exact LLR - (restated max-log LLR + float64 correction from the restated fp32 distances)| <= C_TOL[h] + ulp(llr).
# The max-log part is known bit for bit (tests/test_gpu_channel_sym.py), so the device and the reference differ in the
# correction's fp32 arithmetic and in the rounding of the final sum alone.  dref.correction_tolerance derives the first from
# HIP's documented 1 ulp for expf and logf (taken at 2 ulp each, as G_RTOL of tests/test_gpu_channel_sym.py takes logf): a sum
# of T = 2^h / 2 terms is off by ((T - 1) (1 + 1 / e) + 2) 2^-23 relative, each logf adds 2 ulp of a value <= log T, the
# subtraction one more: 1.2e-6 for h = 2, 2.6e-6 for h = 3, 4.0e-6 for h = 4, and 0 for h = 1, where nothing is added.
C_TOL = {h: dref.correction_tolerance(h) for h in (1, 2, 3, 4)}


def rows_of(n, batch, dev):
    """random 0/1 rows -> (packed tensor [batch, ceil(n / 8)], 0/1 [batch, n])"""
    bits = (np.random.default_rng(1000 * n + batch).random((batch, n)) < 0.5).astype(np.uint8)
    return torch.from_numpy(eref.pack_rows(bits)).to(dev), bits


def draw(batch, n, scheme, dev, *, fading=None, amp=1.0, codeword=None, pos=None, demapper="maxlog", first=FIRST):
    import engine
    from modulation import Modulation
    return engine.sym_llr(batch, n, seed=SEED, stream_id=STREAM, first_frame=first, amp=amp, codeword=codeword, device=dev,
                          modulation=Modulation(scheme, fading, pos, demapper), want_received=True)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_standalone_maxlog_demap_is_the_channels_own_llr(batch, n, gpu_device):
    """engine.demap(rec, "maxlog") of the samples a sym_llr call wrote equals that call's llr bit for bit: every scheme, both
    fadings, with and without an interleaver, and whatever the modulation's own demapper says"""
    import engine
    from modulation import Modulation
    rows_t, _ = rows_of(n, batch, gpu_device)
    pos = np.random.default_rng(n).permutation(n)
    for scheme, m in SCHEMES:
        for fading in FADINGS:
            for p in (None, pos):
                llr, rec = draw(batch, n, scheme, gpu_device, fading=fading, amp=1.7, codeword=rows_t, pos=p)
                got = engine.demap(rec, n, modulation=Modulation(scheme, None, p), device=gpu_device)
                assert same(got, llr), (scheme, fading, p is not None)
                forced = engine.demap(rec, n, modulation=Modulation(scheme, fading, p, "exact"), demapper="maxlog")
                assert same(forced, llr), (scheme, fading, p is not None)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_exact_rule_on_the_kernels_own_samples(batch, n, gpu_device):
    import engine
    from modulation import Modulation
    rows_t, _ = rows_of(n, batch, gpu_device)
    pos = np.random.default_rng(n + 3).permutation(n)
    for scheme, m in SCHEMES:
        h = mref.axis_bits(m)
        worst, small, ratio, largest = 0.0, 0.0, 0.0, 0.0
        for fading in FADINGS:
            for amp, p in ((0.6, None), (1.7, pos)):
                _, rec = draw(batch, n, scheme, gpu_device, fading=fading, amp=amp, codeword=rows_t, pos=p)
                got = engine.demap(rec, n, modulation=Modulation(scheme, fading, p), demapper="exact").cpu().numpy()
                r = rec.cpu().numpy()
                ml, c64 = mref.demap(r, m), dref.correction(r, m)
                want = mref.to_variables(ml.astype(np.float64) + c64, n, p)
                err = np.abs(got.astype(np.float64) - want)
                bound = C_TOL[h] + dref.ulp32(got)
                near = np.abs(got) < 2.0                            # where the final sum's ulp is below 2.4e-7
                worst, largest = max(worst, err.max()), max(largest, np.abs(c64).max())
                small = max(small, err[near].max() if near.any() else 0.0)
                ratio = max(ratio, (err / np.maximum(bound, 1e-300)).max())
                assert np.isfinite(got).all()
                assert (err <= bound).all(), (scheme, fading, err.max())
        print(f"{scheme} batch {batch} n {n}: max |device exact - (max-log + c64)| = {worst:.3e}, where |llr| < 2 {small:.3e} "
              f"(C_TOL {C_TOL[h]:.3e}), largest error over its bound {ratio:.3f}, largest |c| = {largest:.3f}")
        assert m < 4 or largest > 0.1 or batch * n < 50             # the correction is there from 16-QAM up


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_fused_exact_equals_standalone_exact(batch, n, gpu_device):
    """the channel kernels' EXACT instantiations against sym_demap on the samples they wrote, bit for bit; the samples are
    the max-log call's; sym_llr_mix gives each frame what sym_llr gives it at the frame's point"""
    import engine
    from modulation import Modulation
    rows_t, _ = rows_of(n, batch, gpu_device)
    pos = np.random.default_rng(n + 5).permutation(n)
    tab = np.array([0.5, 1.1, 2.3], dtype=np.float32)
    points = engine.mix_points(FIRST, batch, 3).numpy()
    for scheme, m in QAM:
        for fading in FADINGS:
            for p in (None, pos):
                per_point = []
                for amp in tab:
                    fused, rec = draw(batch, n, scheme, gpu_device, fading=fading, amp=float(amp), codeword=rows_t, pos=p,
                                      demapper="exact")
                    alone = engine.demap(rec, n, modulation=Modulation(scheme, fading, p, "exact"))
                    assert same(fused, alone), (scheme, fading, p is not None)
                    ml, mrec = draw(batch, n, scheme, gpu_device, fading=fading, amp=float(amp), codeword=rows_t, pos=p)
                    assert same(rec, mrec) and (n * batch < 50 or not torch.equal(ml, fused))
                    per_point.append(alone)
                mix, targets = engine.sym_llr_mix(batch, n, seed=SEED, stream_id=STREAM, first_frame=FIRST, amp=tab,
                                                  modulation=Modulation(scheme, fading, p, "exact"), codeword=rows_t,
                                                  device=gpu_device, want_targets=True)
                want = torch.stack([per_point[points[b]][b] for b in range(batch)])
                assert same(mix, want), (scheme, fading, p is not None)
                plain_targets = engine.sym_llr_mix(batch, n, seed=SEED, stream_id=STREAM, first_frame=FIRST, amp=tab,
                                                   modulation=Modulation(scheme, fading, p), codeword=rows_t,
                                                   device=gpu_device, want_targets=True)[1]
                assert torch.equal(targets, plain_targets)


@pytest.mark.parametrize("n", NS)
def test_bpsk_and_qpsk_exact_is_maxlog_bit_for_bit(n, gpu_device):
    import engine
    from modulation import Modulation
    batch = 67
    rows_t, _ = rows_of(n, batch, gpu_device)
    pos = np.random.default_rng(n + 7).permutation(n)
    for scheme in ("bpsk", "qpsk"):
        for fading in FADINGS:
            for p in (None, pos):
                ml, rec = draw(batch, n, scheme, gpu_device, fading=fading, amp=0.9, codeword=rows_t, pos=p)
                ex, erec = draw(batch, n, scheme, gpu_device, fading=fading, amp=0.9, codeword=rows_t, pos=p, demapper="exact")
                assert same(ml, ex) and same(rec, erec)
                assert same(engine.demap(rec, n, modulation=Modulation(scheme, fading, p, "exact")), ml)
                mix = [engine.sym_llr_mix(batch, n, seed=SEED, stream_id=STREAM, first_frame=FIRST, amp=[0.9, 1.4],
                                          modulation=Modulation(scheme, fading, p, d), codeword=rows_t, device=gpu_device)
                       for d in ("maxlog", "exact")]
                assert same(mix[0], mix[1])


@pytest.mark.parametrize("n", NS)
def test_the_correction_is_bounded_and_amp_8_decides_the_sent_bits(n, gpu_device):
    """|exact - maxlog| <= log(L / 2) on device output (plus the correction's rounding bound and the final sum's ulp); at
    amp = 8 without fading |z| <= 6.76 < 8 keeps every symbol in its cell, the output is finite and its signs are the sent bits"""
    batch = 67
    rows_t, rows = rows_of(n, batch, gpu_device)
    pos = np.random.default_rng(n + 9).permutation(n)
    for scheme, m in SCHEMES:
        h = mref.axis_bits(m)
        for fading, amp in ((None, 0.4), ("rayleigh", 1.3), (None, 8.0)):
            for p in (None, pos):
                ml, _ = draw(batch, n, scheme, gpu_device, fading=fading, amp=amp, codeword=rows_t, pos=p)
                ex, _ = draw(batch, n, scheme, gpu_device, fading=fading, amp=amp, codeword=rows_t, pos=p, demapper="exact")
                ml, ex = ml.cpu().numpy(), ex.cpu().numpy()
                assert np.isfinite(ex).all()
                bound = np.log(2 ** h / 2) + C_TOL[h] + dref.ulp32(ex)
                assert (np.abs(ex.astype(np.float64) - ml.astype(np.float64)) <= bound).all(), (scheme, fading, amp)
                if amp == 8.0:
                    assert (ex != 0).all() and np.array_equal(ex < 0, rows == 1), (scheme, p is not None)


@pytest.mark.parametrize("n", [1, 7, 1997, 1998])
def test_nothing_is_written_past_the_block(n, gpu_device):
    """llr inside a larger buffer at a base that is only 4-byte aligned: the words before and after stay untouched and the
    block holds what engine.demap returns.  An odd n puts the rows of the batch at the 0-, 4-, 8- and 12-byte phases, the four
    skews move them all"""
    import _native
    import engine
    from modulation import Modulation
    lib = _native.load()
    batch, guard, fill = 5, 64, 0x7fc0dead
    rows_t, _ = rows_of(n, batch, gpu_device)
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    pos = np.random.default_rng(n + 1).permutation(n)
    for scheme, m in SCHEMES:
        for p in (None, pos):
            _, rec = draw(batch, n, scheme, gpu_device, fading="rayleigh", amp=1.2, codeword=rows_t, pos=p)
            for rule in ("maxlog", "exact"):
                mod = Modulation(scheme, None, p, rule)
                want = engine.demap(rec, n, modulation=mod).cpu().numpy().view(np.int32).reshape(-1)
                desc, keep = mod.native(0.0, n, gpu_device)
                for skew in (0, 1, 2, 3):
                    buf = torch.full((guard + skew + batch * n + guard,), fill, dtype=torch.int32, device=gpu_device)
                    _native.check(lib.ldpc_demap_sym(C.c_void_p(buf.data_ptr() + 4 * (guard + skew)), batch, n, C.byref(desc),
                                                     _native.DEMAP_EXACT if rule == "exact" else _native.DEMAP_MAXLOG,
                                                     C.c_void_p(rec.data_ptr()), stream), "ldpc_demap_sym")
                    host = buf.cpu().numpy()
                    lo = guard + skew
                    assert (host[:lo] == fill).all() and (host[lo + batch * n:] == fill).all(), (scheme, rule, skew)
                    assert np.array_equal(host[lo:lo + batch * n], want), (scheme, rule, skew)


def test_what_the_entry_point_refuses(gpu_device):
    import _native
    import engine
    from modulation import Modulation
    lib = _native.load()
    buf = torch.zeros(256, dtype=torch.float32, device=gpu_device)
    p, off = C.c_void_p(buf.data_ptr()), lambda k: C.c_void_p(buf.data_ptr() + k)
    rec = off(512)                                                                     # 16-byte aligned, 2 symbols of n = 8
    mod = C.byref(_native.ModulationDesc(bits_per_symbol=4, fading=0, amp=1.0))
    call = lambda llr, batch, md, rec, dm=0: lib.ldpc_demap_sym(llr, batch, 8, md, dm, rec, None)
    for dm in (2, -1, 7):
        assert call(p, 1, mod, rec, dm) == -1 and b"demapper" in lib.ldpc_last_error()
    assert call(p, 1, mod, None) == -1 and b"NULL received" in lib.ldpc_last_error()
    assert call(p, 1, mod, off(512 + 4)) == -1 and b"16-byte" in lib.ldpc_last_error()
    assert call(None, 1, mod, rec) == -1 and b"NULL llr" in lib.ldpc_last_error()
    assert call(off(2), 1, mod, rec) == -1 and b"4-byte" in lib.ldpc_last_error()
    assert call(p, 1, None, rec) == -1 and b"mod" in lib.ldpc_last_error()
    assert call(p, -1, mod, rec) == -1 and lib.ldpc_demap_sym(p, 1, 0, mod, 0, rec, None) == -1
    # the order: scalars (the demapper among them), then batch == 0 is OK whatever the pointers are, then the pointers
    assert call(None, 0, mod, None) == 0 and call(off(2), 0, mod, off(4), 1) == 0
    assert call(None, 0, mod, None, 2) == -1
    assert call(None, 0, C.byref(_native.ModulationDesc(bits_per_symbol=3)), None) == -1
    # amp and fading are not read: e travels with the samples
    odd = C.byref(_native.ModulationDesc(bits_per_symbol=4, fading=9, amp=float("nan")))
    assert call(off(4), 1, odd, rec, 1) == 0 and call(off(4), 1, mod, rec, 0) == 0       # a skewed llr is fine
    torch.cuda.synchronize()
    # the _dm channel entry points refuse a bad demapper as an argument error, after the modulation and before the pointers
    assert lib.ldpc_channel_sym_dm(p, 1, 8, 0, 0, 0, mod, None, 0, None, 2, None) == -1 and b"demapper" in lib.ldpc_last_error()
    assert lib.ldpc_channel_sym_dm(None, 0, 8, 0, 0, 0, mod, None, 0, None, 2, None) == -1
    assert lib.ldpc_channel_sym_dm(None, 0, 8, 0, 0, 0, mod, None, 0, None, 1, None) == 0
    assert lib.ldpc_channel_sym_mix_dm(p, 1, 8, 0, 0, 0, mod, off(64), 1, None, 0, None, 5, None) == -1
    assert b"demapper" in lib.ldpc_last_error()
    # engine.demap: the modulation's own rule unless one is named; the interleaver must fit n
    q16 = Modulation("qam16", demapper="exact")
    llr, samples = engine.sym_llr(4, 96, seed=1, modulation=q16, snr_db=9.0, device=gpu_device, want_received=True)
    assert torch.equal(engine.demap(samples, 96, modulation=q16), llr)
    assert torch.equal(engine.demap(samples, 96, modulation=Modulation("qam16"), demapper="exact"), llr)
    assert not torch.equal(engine.demap(samples, 96, modulation=q16, demapper="maxlog"), llr)
    assert engine.demap(samples[:0], 96, modulation=q16).shape == (0, 96)
    with pytest.raises(ValueError):
        engine.demap(samples, 96, modulation=Modulation("qam16", interleaver=[1, 0]))
    with pytest.raises(ValueError, match="received"):
        engine.demap(samples, 95, modulation=Modulation("qam64"))                      # 16 symbols, not 24
