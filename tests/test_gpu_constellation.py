"""
GPU tests (-m gpu) of the constellation channel kernels (ldpc_channel_con, ldpc_channel_con_mix, ldpc_demap_con) against the
numpy restatement of their definition (tests/constellation_reference.py): the received samples within a derived bound of the
float64 restatement from the Philox words, the max-log LLRs bit for bit from the kernel's own samples, engine.demap against the
call that wrote the samples, the exact rule within the derived bound of max-log plus the float64 correction, the mixed-SNR draw
frame by frame, the noise of a QAM table against the string scheme's, guard words at every store alignment, and what the entry
points refuse.  Tables of 2, 4, 8, 16, 32 and 64 points: m = 3 and m = 5 with n = 7 and n = 1998 give short last symbols and
symbol runs at every alignment of a 16-byte boundary.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import constellation_reference as cref
import encode_reference as eref
import modulation_reference as mref

pytestmark = pytest.mark.gpu

SEED, STREAM = 0x9e3779b97f4a7c15, 4700
FIRST = 2 ** 32 - 30                                  # 67 frames cross into the high counter word
NS, BATCHES = (1, 7, 96, 1998), (1, 3, 67)
# tests/test_gpu_channel_sym.py derives both: (zI, zQ) is the Box-Muller pair of two words, within 1e-5 of the float64 pair;
# g = sqrtf(-logf(u)) is within 5 * 2^-23 relative of sqrt(-log(u)).  The stream is the same, word for word.
Z_TOL = 1e-5
G_RTOL = 5 * 2.0 ** -23
EPS = cref.EPS
TABLES = ("psk2", "psk4", "psk8", "apsk16", "apsk32", "rand64", "rand8")        # m = 1, 2, 3, 4, 5, 6, 3


def table(name, fading=None, pos=None, demapper="maxlog"):
    from modulation import Constellation
    kw = dict(fading=fading, interleaver=pos, demapper=demapper)
    if name.startswith("psk"):
        return Constellation.psk(int(name[3:]), **kw)
    if name == "apsk16":
        return Constellation.apsk((4, 12), (1.0, 2.6), **kw)
    if name == "apsk32":
        return Constellation.apsk((4, 12, 16), (1.0, 2.64, 4.64), **kw)
    if name == "rand64":
        rng = np.random.default_rng(64)
        return Constellation(rng.normal(size=64) + 1j * rng.normal(size=64), **kw)
    # eight random points, by angle, labelled by a permutation under which neighbours differ in up to three bits
    rng = np.random.default_rng(8)
    pts = rng.normal(size=8) + 1j * rng.normal(size=8)
    pts = pts[np.argsort(np.angle(pts))]
    out = np.empty(8, dtype=np.complex128)
    out[[0, 7, 3, 4, 5, 2, 6, 1]] = pts
    return Constellation(out, name="rand8", **kw)


def codeword_rows(n, batch, dev):
    """packed rows of encode_random where the package has a code of this n, random rows elsewhere -> (tensor, 0/1 [batch, n])"""
    import codes
    import engine
    name = {96: "small_96_48", 1998: "ira_1998_1512"}.get(n)
    if name:
        enc = codes.Encoder.from_graph(codes.load_graph(name))
        cw = engine.encode_random(enc, batch, seed=SEED, stream_id=STREAM, first_frame=FIRST, device=dev)
        return cw, eref.unpack_rows(cw.cpu().numpy(), n)
    bits = (np.random.default_rng(n + batch).random((batch, n)) < 0.5).astype(np.uint8)
    return torch.from_numpy(eref.pack_rows(bits)).to(dev), bits


def draw(batch, n, con, dev, *, amp=1.0, codeword=None, first=FIRST):
    import engine
    llr, rec = engine.sym_llr(batch, n, seed=SEED, stream_id=STREAM, first_frame=first, amp=amp, codeword=codeword, device=dev,
                              modulation=con, want_received=True)
    m = con.bits_per_symbol
    assert llr.shape == (batch, n) and llr.dtype == torch.float32 and rec.shape == (batch, (n + m - 1) // m, 4)
    return llr.cpu().numpy(), rec.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ------------------------------------------------------------------ (a) received samples
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_received_samples_against_the_float64_restatement(batch, n, gpu_device):
    """v = (e * x_l) + z and e = g * amp against float64 arithmetic on the Philox words, the fp32 table and the fp32 amp.
    From Z_TOL and G_RTOL, to first order (1 % is added for the second):
      e = fl(g_dev * amp):   |e - e_ref| <= (G_RTOL + EPS) e_ref under fading; e = amp exactly without
      fl(e * x):             |. - e_ref x| <= (G_RTOL + 2 EPS) |e_ref x|          (2 EPS |e_ref x| without fading: EPS is counted
                                                                                   for e all the same)
      + z, and its rounding: |v - v_ref| <= (G_RTOL + 2 EPS) |e_ref x| + Z_TOL + EPS |v_ref|
    The fourth word is 0.0f; the sent point is the table entry of the label sum_k b_k 2^k of the symbol's bits."""
    rows_t, rows = codeword_rows(n, batch, gpu_device)
    amp = np.float32(1.7)
    for name in TABLES:
        for fading in (None, "rayleigh"):
            con = table(name, fading)
            m = con.bits_per_symbol
            S = (n + m - 1) // m
            words = mref.symbol_words(batch, S, SEED, STREAM, FIRST)
            z_ref = mref.symbol_normals(words)
            g_ref = mref.fading_gain(words) if fading else np.ones((batch, S))
            g_tol = G_RTOL if fading else 0.0
            e_ref = g_ref * float(amp)
            bits = mref.symbol_bits(rows, m)
            x = cref.sent_points(con.points, bits).astype(np.float64)
            v_ref = cref.received64(con.points, bits, e_ref, z_ref)
            _, rec = draw(batch, n, con, gpu_device, amp=float(amp), codeword=rows_t)
            assert (rec[..., 3] == 0).all() and not np.signbit(rec[..., 3]).any()
            de = np.abs(rec[..., 2].astype(np.float64) - e_ref)
            assert (de <= 1.01 * (g_tol + EPS) * e_ref).all(), (name, fading)
            if not fading:
                assert (rec[..., 2] == amp).all()
            bound = 1.01 * ((g_tol + 2 * EPS) * np.abs(e_ref[..., None] * x) + Z_TOL + EPS * np.abs(v_ref))
            dv = np.abs(rec[..., :2].astype(np.float64) - v_ref)
            print(f"{name} {fading} batch {batch} n {n}: max |dv| = {dv.max():.3e}, worst ratio {(dv / bound).max():.3f}")
            assert (dv <= bound).all(), (name, fading)


# ------------------------------------------------------------------ (b) max-log LLRs
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_maxlog_llrs_are_the_restated_rule_of_the_kernels_own_samples(batch, n, gpu_device):
    """bit for bit: both fadings, the identity and a random interleaver, per-frame random codewords; and the samples are
    fl(fl(e * x_l) + z) of the z of the amp = 0 run and the e the run itself reports"""
    rows_t, rows = codeword_rows(n, batch, gpu_device)
    pos = np.random.default_rng(n).permutation(n)
    for name in TABLES:
        for fading in (None, "rayleigh"):
            for p in (None, pos):
                con = table(name, fading, p)
                m = con.bits_per_symbol
                _, zrec = draw(batch, n, con, gpu_device, amp=0.0, codeword=rows_t)
                llr, rec = draw(batch, n, con, gpu_device, amp=1.7, codeword=rows_t)
                assert (zrec[..., 2] == 0).all()
                want_v = cref.received32(con.points, mref.symbol_bits(rows, m, p), rec[..., 2], zrec[..., :2])
                assert same_bits(rec[..., :2], want_v), (name, fading, p is not None)
                want = cref.to_variables(cref.demap(rec, con.points), n, p)
                assert same_bits(llr, want), (name, fading, p is not None)
                if n >= 96:
                    assert (llr != 0).mean() > 0.9
    # e = 0: every distance is equal and the LLR is +0.0f
    for name in ("psk8", "rand64"):
        for dm in ("maxlog", "exact"):
            llr, _ = draw(batch, n, table(name, demapper=dm), gpu_device, amp=0.0, codeword=rows_t)
            assert (llr == 0).all() and not np.signbit(llr).any()


# ------------------------------------------------------------------ (c) engine.demap against sym_llr
@pytest.mark.parametrize("n", NS)
def test_demap_gives_the_llrs_of_the_call_that_wrote_the_samples(n, gpu_device):
    import engine
    batch = 67
    rows_t, _ = codeword_rows(n, batch, gpu_device)
    pos = np.random.default_rng(n + 3).permutation(n)
    for name in TABLES:
        for p in (None, pos):
            got = {}
            for dm in ("maxlog", "exact"):
                con = table(name, "rayleigh", p, dm)
                llr, rec = engine.sym_llr(batch, n, seed=SEED, stream_id=STREAM, first_frame=FIRST, amp=1.4, codeword=rows_t,
                                          device=gpu_device, modulation=con, want_received=True)
                got[dm] = (llr, rec)
                assert torch.equal(engine.demap(rec, n, modulation=con).view(torch.int32), llr.view(torch.int32)), (name, dm)
            # the samples do not depend on the demapper, and either rule can be asked of either modulation
            assert torch.equal(got["maxlog"][1].view(torch.int32), got["exact"][1].view(torch.int32))
            plain = table(name, None, p)                                       # fading is not used: e travels with the samples
            for dm in ("maxlog", "exact"):
                out = engine.demap(got["maxlog"][1], n, modulation=plain, demapper=dm)
                assert torch.equal(out.view(torch.int32), got[dm][0].view(torch.int32)), (name, dm)


# ------------------------------------------------------------------ (d) the exact rule
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_exact_rule_is_maxlog_plus_the_correction(batch, n, gpu_device):
    """the device's exact LLRs within cref.correction_tolerance(m) + ulp(llr) of (restated max-log + float64 correction from
    the restated fp32 distances), finite everywhere, within (m - 1) log 2 + that bound of the max-log LLRs, and the correction
    is there: its largest magnitude exceeds 0.1 from 8 points up.  Two points: the max-log rule bit for bit."""
    rows_t, _ = codeword_rows(n, batch, gpu_device)
    pos = np.random.default_rng(n + 1).permutation(n)
    for name in TABLES:
        for fading, p in ((None, None), ("rayleigh", pos)):
            con = table(name, fading, p, "exact")
            m = con.bits_per_symbol
            llr, rec = draw(batch, n, con, gpu_device, amp=1.3, codeword=rows_t)
            ml, mrec = draw(batch, n, table(name, fading, p), gpu_device, amp=1.3, codeword=rows_t)
            assert same_bits(rec, mrec) and np.isfinite(llr).all()
            restated = cref.to_variables(cref.demap(rec, con.points), n, p)
            assert same_bits(ml, restated)
            corr = cref.to_variables(cref.correction(rec, con.points), n, p)
            want = restated.astype(np.float64) + corr
            tol = cref.correction_tolerance(m) + cref.ulp32(want)
            gap = np.abs(llr.astype(np.float64) - want)
            print(f"{name} {fading} batch {batch} n {n}: max gap {gap.max():.3e}, worst ratio {(gap / np.maximum(tol, 1e-300)).max():.3f}, "
                  f"largest |c| {np.abs(corr).max():.3f}")
            assert (gap <= tol).all(), (name, fading)
            assert (np.abs(llr.astype(np.float64) - ml) <= (m - 1) * math.log(2.0) + tol).all()
            if m >= 3 and batch * n >= 50:
                assert np.abs(corr).max() > 0.1 and np.abs(llr - ml).max() > 0.1
            if m == 1:
                assert same_bits(llr, ml)


# ------------------------------------------------------------------ (e) the mixed-SNR draw
@pytest.mark.parametrize("n", NS)
def test_mix_gives_each_frame_its_point_and_the_sent_bits(n, gpu_device):
    """frame f gets, bit for bit, what sym_llr gives it at amp_tab[f mod K], under both rules; the targets are the sent bits;
    pad bits are stored in neither output (the outputs are exactly [batch, n]: the guard test looks past their end)"""
    import engine
    batch, K = 67, 5
    rows_t, rows = codeword_rows(n, batch, gpu_device)
    amps = np.array([0.0, 0.6, 1.1, 1.9, 3.2], dtype=np.float32)
    pos = np.random.default_rng(n + 2).permutation(n)
    point = engine.mix_points(FIRST, batch, K).numpy()
    for name in TABLES:
        for fading, p, dm in ((None, None, "maxlog"), ("rayleigh", pos, "maxlog"), ("rayleigh", None, "exact"), (None, pos, "exact")):
            con = table(name, fading, p, dm)
            kw = dict(seed=SEED, stream_id=STREAM, first_frame=FIRST, modulation=con, codeword=rows_t, device=gpu_device)
            llr, tgt = engine.sym_llr_mix(batch, n, amp=amps, want_targets=True, **kw)
            assert same_bits(tgt.cpu().numpy(), rows.astype(np.float32)), (name, fading, dm)
            only = engine.sym_llr_mix(batch, n, amp=amps, **kw)
            assert torch.equal(only.view(torch.int32), llr.view(torch.int32))
            llr = llr.cpu().numpy()
            for k in range(K):
                want = engine.sym_llr(batch, n, amp=float(amps[k]), **kw).cpu().numpy()
                sel = point == k
                assert sel.any() and same_bits(llr[sel], want[sel]), (name, fading, dm, k)
    # snr_db goes through Constellation.amp_table, and one word for every frame gives constant targets
    con = table("psk8")
    a = engine.sym_llr_mix(8, n, seed=1, modulation=con, snr_db=[2.0, 7.5], device=gpu_device)
    b = engine.sym_llr_mix(8, n, seed=1, modulation=con, amp=con.amp_table([2.0, 7.5]), device=gpu_device)
    assert torch.equal(a, b)
    _, t0 = engine.sym_llr_mix(8, n, seed=1, modulation=con, snr_db=[2.0], device=gpu_device, want_targets=True)
    assert (t0 == 0).all()


# ------------------------------------------------------------------ (f) the noise of the string schemes
@pytest.mark.parametrize("scheme", ["qam16", "qam64"])
def test_a_qam_table_draws_the_string_schemes_noise(scheme, gpu_device):
    """Constellation.from_modulation(Modulation(scheme)) against Modulation(scheme) at the same (seed, stream, frame) and
    codewords.  At amp = 0 both store v = z and at amp = 1 both store e = g: bit for bit.  At a working amplitude
    (amp_c = A for the table, amp_s = fl(A d) for the string scheme, d the half-spacing) z recovered from either `received`
    agrees within the roundings of its own v = fl(fl(e x) + z): EPS (|e x| + |v|) each.
    The LLRs.  As real numbers e_s a and e_c x_c differ by the roundings of amp_s, of the table's cast, and of the two products
    g * amp: 4 half ulps, 2 EPS relative, so at most 2 EPS e R for any point (e R = e times the largest coordinate).  The two
    fp32 samples v_s, v_c each carry that for the sent point plus a product and a sum rounding: |v_s - v_c| <= 4 EPS e R +
    2 EPS |v|.  A candidate's offset t = v - e x therefore differs by dt <= 6 EPS e R + 2 EPS |v| per coordinate between the
    two models, its distance by 2 (|tI| + |tQ|) dt <= 2 sqrt(2 Dm) dt, and a max-log LLR, half a difference of two minima,
    by the same amount.  Each device result is within cref.llr_tolerance of float64 arithmetic on its own model (the
    separable rule does a subset of the joint rule's roundings): the bound is 2 llr_tolerance + 1.01 * 2 sqrt(2 Dm) dt."""
    import engine
    from modulation import Constellation, Modulation
    n, batch = 1998, 67
    m = mref.SCHEMES[scheme]
    d = mref.half_spacing(m)
    rows_t, rows = codeword_rows(n, batch, gpu_device)
    A = np.float32(2.3)
    amp_s = float(np.float32(float(A) * d))
    for fading in (None, "rayleigh"):
        mod = Modulation(scheme, fading)
        con = Constellation.from_modulation(mod)
        kw = dict(seed=SEED, stream_id=STREAM, first_frame=FIRST, codeword=rows_t, device=gpu_device, want_received=True)
        for amp in (0.0, 1.0):
            _, rs = engine.sym_llr(batch, n, modulation=mod, amp=amp, **kw)
            _, rc = engine.sym_llr(batch, n, modulation=con, amp=amp, **kw)
            if amp == 0.0:
                assert torch.equal(rs[..., :2].view(torch.int32), rc[..., :2].view(torch.int32))      # z
            assert torch.equal(rs[..., 2].view(torch.int32), rc[..., 2].view(torch.int32))            # e = g * amp
        ls, rs = engine.sym_llr(batch, n, modulation=mod, amp=amp_s, **kw)
        lc, rc = engine.sym_llr(batch, n, modulation=con, amp=float(A), **kw)
        ls, rs, lc, rc = (t.cpu().numpy().astype(np.float64) for t in (ls, rs, lc, rc))
        R = float(np.abs(con.points).max())
        live = rc[..., 2] > 0
        assert live.mean() > 0.99
        assert np.abs(rs[..., 2][live] * (2 ** (m // 2) - 1) / (rc[..., 2][live] * R) - 1.0).max() <= 2 * EPS   # e_s a_max = e_c x_max
        # z from either array: v minus e times the sent point, against the z both stored at amp = 0
        _, zrec = engine.sym_llr(batch, n, modulation=con, amp=0.0, **kw)
        z = zrec[..., :2].cpu().numpy().astype(np.float64)
        bits = mref.symbol_bits(rows, m)
        sent_s = rs[..., 2:3] * mref.sent_amplitudes(bits, m)
        sent_c = rc[..., 2:3] * cref.sent_points(con.points, bits).astype(np.float64)
        for r, sent in ((rs, sent_s), (rc, sent_c)):
            assert (np.abs((r[..., :2] - sent) - z) <= EPS * (np.abs(sent) + np.abs(r[..., :2]))).all()
        rec32 = rc.astype(np.float32)
        Dm = cref.distances(rec32, con.points).astype(np.float64).max(axis=-1)
        dt = 6 * EPS * rc[..., 2] * R + 2 * EPS * np.abs(rc[..., :2]).max(axis=-1)
        tol = 2 * cref.llr_tolerance(rec32, con.points) + 1.01 * 2 * np.sqrt(2 * Dm) * dt
        tol = cref.to_variables(np.repeat(tol[..., None], m, axis=-1), n)
        gap = np.abs(ls - lc)
        print(f"{scheme} {fading}: max LLR gap {gap.max():.3e}, worst ratio {(gap / tol).max():.3f}")
        assert (gap <= tol).all() and gap.max() > 0


# ------------------------------------------------------------------ (g) guard words
@pytest.mark.parametrize("name", ["psk8", "apsk32", "rand64"])
def test_nothing_is_written_past_the_block(name, gpu_device):
    """llr, received and targets inside larger buffers, the fp32 rows at every 4-byte skew of their start: the words before and
    after stay untouched and the block holds what a plain call returns.  n = 1998 is no multiple of 4, 5 or 6 and n = 7 has a
    short last symbol in every row: each row of a batch starts at another alignment, so sym_store takes every one of its paths
    for m = 3 and m = 5."""
    import _native
    import engine
    lib = _native.load()
    batch, guard, fill = 5, 64, 0x7fc0dead
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    amps = torch.tensor([0.7, 1.2, 2.0], dtype=torch.float32, device=gpu_device)
    for n in (7, 1998):
        rows_t, _ = codeword_rows(n, batch, gpu_device)
        pos = np.random.default_rng(n + 1).permutation(n)
        for p in (None, pos):
            for dm in ("maxlog", "exact"):
                con = table(name, "rayleigh", p, dm)
                m = con.bits_per_symbol
                S = (n + m - 1) // m
                code = {"maxlog": 0, "exact": 1}[dm]
                want_llr, want_rec = draw(batch, n, con, gpu_device, amp=1.2, codeword=rows_t)
                kw = dict(seed=SEED, stream_id=STREAM, first_frame=FIRST, modulation=con, codeword=rows_t, device=gpu_device)
                want_mix, want_tgt = (t.cpu().numpy() for t in engine.sym_llr_mix(batch, n, amp=amps, want_targets=True, **kw))
                desc, keep = con.native(1.2, n, gpu_device)
                for skew in (0, 1, 2, 3):
                    new = lambda words: torch.full((guard + skew + words + guard,), fill, dtype=torch.int32, device=gpu_device)
                    at = lambda buf: C.c_void_p(buf.data_ptr() + 4 * (guard + skew))
                    buf, mbuf, tbuf, dbuf = new(batch * n), new(batch * n), new(batch * n), new(batch * n)
                    rbuf = torch.full((guard + batch * S * 4 + guard,), fill, dtype=torch.int32, device=gpu_device)
                    rptr = C.c_void_p(rbuf.data_ptr() + 4 * guard)
                    head = (batch, n, SEED, STREAM, FIRST, C.byref(desc))
                    cw = (C.c_void_p(rows_t.data_ptr()), (n + 7) // 8)
                    _native.check(lib.ldpc_channel_con(at(buf), *head, *cw, rptr, code, stream), "ldpc_channel_con")
                    _native.check(lib.ldpc_channel_con_mix(at(mbuf), *head, C.c_void_p(amps.data_ptr()), 3, *cw, at(tbuf), code,
                                                           stream), "ldpc_channel_con_mix")
                    _native.check(lib.ldpc_demap_con(at(dbuf), batch, n, C.byref(desc), code, rptr, stream), "ldpc_demap_con")
                    lo = guard + skew
                    for b, want in ((buf, want_llr), (mbuf, want_mix), (tbuf, want_tgt), (dbuf, want_llr)):
                        host = b.cpu().numpy()
                        assert (host[:lo] == fill).all() and (host[lo + batch * n:] == fill).all(), (n, dm, skew)
                        assert np.array_equal(host[lo:lo + batch * n], want.view(np.int32).reshape(-1)), (n, dm, skew)
                    rhost = rbuf.cpu().numpy()
                    assert (rhost[:guard] == fill).all() and (rhost[guard + batch * S * 4:] == fill).all(), (n, dm, skew)
                    assert np.array_equal(rhost[guard:guard + batch * S * 4], want_rec.view(np.int32).reshape(-1))


# ------------------------------------------------------------------ (h) argument checks
def test_what_the_entry_points_refuse(gpu_device):
    import _native
    import engine
    lib = _native.load()
    buf = torch.zeros(1024, dtype=torch.float32, device=gpu_device)
    p, off = C.c_void_p(buf.data_ptr()), lambda k: C.c_void_p(buf.data_ptr() + k)
    tab = buf.data_ptr() + 2048                                       # 16 zero points: any table will do

    def con(m=4, fading=0, amp=1.0, points=tab):
        return C.byref(_native.ConstellationDesc(bits_per_symbol=m, fading=fading, amp=amp, points=points))

    err = lib.ldpc_last_error
    chan = lambda llr, batch, cd, rec=None, stride=0, dm=0, n=8: lib.ldpc_channel_con(llr, batch, n, 0, 0, 0, cd, None, stride, rec,
                                                                                      dm, None)
    mix = lambda llr, batch, cd, tgt=None, amp_tab=off(3072), K=2, dm=0, n=8, stride=0: lib.ldpc_channel_con_mix(
        llr, batch, n, 0, 0, 0, cd, amp_tab, K, None, stride, tgt, dm, None)
    dem = lambda llr, batch, cd, rec=None, dm=0, n=8: lib.ldpc_demap_con(llr, batch, n, cd, dm, rec, None)
    # the scalars, in the header's order: m, points, fading, amp, stride, demapper, n_points; then S
    assert chan(p, 1, None) == -1 and b"con" in err()
    assert chan(p, 1, con(7, points=None, fading=2)) == -1 and b"bits_per_symbol" in err()
    assert chan(p, 1, con(points=None, fading=2)) == -1 and b"points" in err()
    assert chan(p, 1, con(fading=2, amp=-1.0)) == -1 and b"fading" in err()
    assert chan(p, 1, con(amp=-1.0), stride=3) == -1 and b"amp" in err()
    assert chan(p, 1, con(), stride=3, dm=2) == -1 and b"stride" in err()
    assert chan(p, 1, con(1), dm=2, n=2 ** 29) == -1 and b"demapper" in err()
    assert mix(p, 1, con(), dm=2, K=0) == -1 and b"demapper" in err()
    assert mix(p, 1, con(1), K=0, n=2 ** 29) == -1 and b"n_points" in err()
    assert mix(p, 1, con(1), n=2 ** 29) == -3 and chan(p, 1, con(1), n=2 ** 29) == -3 and dem(p, 1, con(1), p, n=2 ** 29) == -3
    assert mix(p, 1, con(), amp_tab=None) == -1 and b"amp_tab" in err()
    # batch == 0 is OK whatever the pointers are; the pointers come after it
    assert chan(None, 0, con()) == 0 and chan(off(2), 0, con(points=tab + 4), off(4)) == 0
    assert mix(None, 0, con(), amp_tab=None) == 0 and dem(None, 0, con()) == 0
    assert chan(None, 1, con()) == -1 and b"NULL llr" in err()
    assert chan(off(2), 1, con()) == -1 and b"4-byte" in err()
    assert chan(p, 1, con(), off(1024 + 4)) == -1 and b"16-byte" in err()
    assert chan(p, 1, con(points=tab + 4)) == -1 and b"8-byte" in err()
    assert mix(p, 1, con(), off(1024 + 2)) == -1 and b"targets" in err()
    assert mix(p, 1, con(), amp_tab=off(2)) == -1 and b"amp_tab" in err()
    assert mix(p, 1, con(points=tab + 4)) == -1 and b"8-byte" in err()
    assert dem(p, 1, con()) == -1 and b"NULL received" in err()
    assert dem(p, 1, con(), off(1024 + 8)) == -1 and b"16-byte" in err()
    assert dem(p, 1, con(points=tab + 4), off(1024)) == -1 and b"8-byte" in err()
    # skewed outputs and a table that is only 8-byte aligned are fine
    assert chan(off(4), 1, con(points=tab + 8), off(1024)) == 0 and mix(off(4), 1, con(points=tab + 8), off(1024 + 4)) == 0
    assert dem(off(4), 1, con(points=tab + 8), off(1024)) == 0
    torch.cuda.synchronize()
    psk8 = table("psk8")
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=psk8, device=gpu_device)                # neither snr_db nor amp
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=psk8, amp=-1.0, device=gpu_device)
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=table("psk8", pos=[1, 0]), snr_db=1.0, device=gpu_device)
    a = engine.sym_llr(4, 96, seed=1, stream_id=2, modulation=psk8, snr_db=7.0, device=gpu_device)
    b = engine.sym_llr(4, 96, seed=1, stream_id=2, modulation=psk8, amp=psk8.amp(7.0), device=gpu_device)
    assert torch.equal(a, b)
    # the table is uploaded once per device and kept
    d1, keep1 = psk8.native(1.0, 96, gpu_device)
    d2, keep2 = psk8.native(2.0, 96, gpu_device)
    assert d1.points == d2.points and keep1[1] is keep2[1] and d1.points % 8 == 0
    assert np.array_equal(keep1[1].cpu().numpy(), psk8.points)
