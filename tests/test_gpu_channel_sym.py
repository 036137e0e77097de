"""
GPU tests (-m gpu) of the symbol channel kernel (ldpc_channel_sym) against the numpy restatement of its definition
(tests/modulation_reference.py): the normals and the fading gain within derived tolerances, the received samples and the LLRs
bit for bit from what the kernel itself drew, hard decisions, block independence, per-frame rows, common noise, the
interleaver, guard words around both outputs at every store alignment, and what the entry point refuses.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import encode_reference as eref
import modulation_reference as mref

pytestmark = pytest.mark.gpu

SEED, STREAM = 0x9e3779b97f4a7c15, 4500
FIRST = 2 ** 32 - 30                                  # 67 frames cross into the high counter word
NS, BATCHES = (1, 7, 96, 1998), (1, 3, 67)
SCHEMES = tuple(sorted(mref.SCHEMES.items(), key=lambda kv: kv[1]))          # (name, m), m = 1, 2, 4, 6, 8
# the derivation of tests/test_gpu_sim_channel.py's Z_TOL holds unchanged: (zI, zQ) is the same Box-Muller pair of two words
Z_TOL = 1e-5
# g = sqrtf(-logf(u)) with u exact in fp32, against sqrt(-log(u)) in float64.  HIP documents logf to 1 ulp and sqrtf to 1 ulp;
# taking logf at 2 ulp to be on the safe side, L = -logf(u) has relative error <= 2 * 2^-23 (an ulp is at most 2^-23 of the
# value), the square root halves that to 2^-23, and its own rounding adds at most 1 ulp = 2^-23: 2 * 2^-23 = 2.4e-7 relative
# in all.  The float64 side is exact to 1e-16.  The bound allows 2.5 times that, as Z_TOL does for z.
G_RTOL = 5 * 2.0 ** -23


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


def draw(batch, n, scheme, dev, *, fading=None, amp=1.0, codeword=None, pos=None, first=FIRST):
    import engine
    from modulation import Modulation
    llr, rec = engine.sym_llr(batch, n, seed=SEED, stream_id=STREAM, first_frame=first, amp=amp, codeword=codeword, device=dev,
                              modulation=Modulation(scheme, fading, pos), want_received=True)
    m = mref.SCHEMES[scheme]
    assert llr.shape == (batch, n) and llr.dtype == torch.float32 and rec.shape == (batch, (n + m - 1) // m, 4)
    return llr.cpu().numpy(), rec.cpu().numpy()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_noise_and_fading_against_the_restatement(batch, n, gpu_device):
    for scheme, m in SCHEMES:
        S = (n + m - 1) // m
        words = mref.symbol_words(batch, S, SEED, STREAM, FIRST)
        z_ref, g_ref = mref.symbol_normals(words), mref.fading_gain(words)
        _, rec = draw(batch, n, scheme, gpu_device, amp=0.0)
        dz = np.abs(rec[..., :2 if m > 1 else 1].astype(np.float64) - z_ref[..., :2 if m > 1 else 1]).max()
        assert dz <= Z_TOL, (scheme, dz)
        assert (rec[..., 2:] == 0).all() and (m > 1 or (rec[..., 1] == 0).all())      # e = 0 and the fourth word; vQ of BPSK
        _, ray = draw(batch, n, scheme, gpu_device, fading="rayleigh", amp=1.0)
        dg = np.abs(ray[..., 2].astype(np.float64) - g_ref)
        print(f"{scheme} batch {batch} n {n}: max |dz| = {dz:.3e}, max rel dg = {(dg / np.maximum(g_ref, 1e-300)).max():.3e}")
        assert (dg <= G_RTOL * g_ref).all(), scheme
        assert (ray[..., 3] == 0).all()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_received_samples_and_llrs_are_the_definition_bit_for_bit(batch, n, gpu_device):
    """v = float32(float32(e * a) + z) of the z of the amp = 0 run and e = float32(g * amp) of the g of the amp = 1 Rayleigh run;
    the LLRs are the restated fp32 demapper of the kernel's own received samples.  Every m, both fadings, the all-zero word,
    one word for every frame and one row per frame."""
    rows_t, rows = codeword_rows(n, batch, gpu_device)
    one = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    amp = np.float32(1.7)
    for scheme, m in SCHEMES:
        _, zrec = draw(batch, n, scheme, gpu_device, amp=0.0)
        _, grec = draw(batch, n, scheme, gpu_device, fading="rayleigh", amp=1.0)
        z, g = zrec[..., :2], grec[..., 2]
        for fading in (None, "rayleigh"):
            e_want = (g * amp).astype(np.float32) if fading else np.full_like(g, amp)
            for cw, sent in ((None, np.zeros((batch, n), np.uint8)), (one, np.broadcast_to(one, (batch, n))), (rows_t, rows)):
                llr, rec = draw(batch, n, scheme, gpu_device, fading=fading, amp=float(amp), codeword=cw)
                a = mref.sent_amplitudes(mref.symbol_bits(sent, m), m).astype(np.float32)
                v_want = ((e_want[..., None] * a).astype(np.float32) + z).astype(np.float32)
                if m == 1:
                    v_want[..., 1] = 0.0
                assert np.array_equal(rec[..., 2].view(np.int32), e_want.view(np.int32)), (scheme, fading)
                assert np.array_equal(rec[..., :2].view(np.int32), v_want.view(np.int32)), (scheme, fading)
                want = mref.to_variables(mref.demap(rec, m), n)
                assert np.array_equal(llr.view(np.int32), want.view(np.int32)), (scheme, fading)


@pytest.mark.parametrize("n", NS)
def test_hard_decisions_at_amp_8_are_the_sent_bits(n, gpu_device):
    """|z| <= 6.76 < 8 = half the spacing between neighbouring points: without fading every symbol stays in its own cell"""
    batch = 67
    rows_t, rows = codeword_rows(n, batch, gpu_device)
    pos = np.random.default_rng(n).permutation(n)
    for scheme, m in SCHEMES:
        for p in (None, pos):
            llr, _ = draw(batch, n, scheme, gpu_device, amp=8.0, codeword=rows_t, pos=p)
            assert (llr != 0).all() and np.array_equal(llr < 0, rows == 1), (scheme, p is not None)
            again, _ = draw(batch, n, scheme, gpu_device, amp=8.0, codeword=rows_t, pos=p)
            assert np.array_equal(llr.view(np.int32), again.view(np.int32))


def test_a_frame_gets_the_same_llrs_in_any_block_and_its_own_row(gpu_device):
    for n in (96, 1998, 7):
        rows_t, _ = codeword_rows(n, 67, gpu_device)
        for scheme, m in SCHEMES:
            for fading in (None, "rayleigh"):
                kw = dict(fading=fading, amp=1.3)
                whole, wrec = draw(67, n, scheme, gpu_device, codeword=rows_t, **kw)
                part, prec = draw(10, n, scheme, gpu_device, codeword=rows_t[10:20].contiguous(), first=FIRST + 10, **kw)
                assert np.array_equal(whole[10:20].view(np.int32), part.view(np.int32))
                assert np.array_equal(wrec[10:20].view(np.int32), prec.view(np.int32))
                assert not np.array_equal(whole[0:10], part)
                # row b of a per-frame call equals the single-frame call with that row as the one codeword
                for b in (0, 29, 30, 66):                          # 29 / 30: either side of the high counter word
                    single, _ = draw(1, n, scheme, gpu_device, codeword=rows_t[b], first=FIRST + b, **kw)
                    assert np.array_equal(single[0].view(np.int32), whole[b].view(np.int32)), (n, scheme, b)


def test_fading_leaves_the_noise_as_it_is(gpu_device):
    for n in (7, 1998):
        for scheme, m in SCHEMES:
            _, plain = draw(5, n, scheme, gpu_device, amp=0.0)
            _, faded = draw(5, n, scheme, gpu_device, fading="rayleigh", amp=0.0)
            assert np.array_equal(plain[..., :2].view(np.int32), faded[..., :2].view(np.int32))
            assert (faded[..., 2] == 0).all()


@pytest.mark.parametrize("n", [7, 96, 1998])
def test_interleaver_is_the_identity_run_on_the_permuted_codeword(n, gpu_device):
    batch = 5
    rows_t, c = codeword_rows(n, batch, gpu_device)
    pos = np.random.default_rng(17 * n).permutation(n)
    cp = np.ascontiguousarray(c[:, pos])                           # c'[t] = c[pos[t]]
    cp_t = torch.from_numpy(eref.pack_rows(cp)).to(gpu_device)
    for scheme, m in SCHEMES:
        for fading in (None, "rayleigh"):
            perm, prec = draw(batch, n, scheme, gpu_device, fading=fading, amp=1.1, codeword=rows_t, pos=pos)
            ident, irec = draw(batch, n, scheme, gpu_device, fading=fading, amp=1.1, codeword=cp_t)
            assert np.array_equal(perm[:, pos].view(np.int32), ident.view(np.int32)), (scheme, fading)
            assert np.array_equal(prec.view(np.int32), irec.view(np.int32))


@pytest.mark.parametrize("n", NS)
def test_nothing_is_written_past_the_block(n, gpu_device):
    """llr inside a larger buffer at a base that is only 4-byte aligned, received inside one at a 16-byte aligned base: the
    words before and after stay untouched and the block holds what a plain call returns.  n = 1998 with m = 6 puts every row
    of the batch at another store alignment."""
    import _native
    from modulation import Modulation
    lib = _native.load()
    batch, guard, fill = 5, 64, 0x7fc0dead
    rows_t, _ = codeword_rows(n, batch, gpu_device)
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    pos = np.random.default_rng(n + 1).permutation(n)
    for scheme, m in SCHEMES:
        S = (n + m - 1) // m
        for p in (None, pos):
            mod = Modulation(scheme, "rayleigh", p)
            want_llr, want_rec = draw(batch, n, scheme, gpu_device, fading="rayleigh", amp=1.2, codeword=rows_t, pos=p)
            desc, keep = mod.native(1.2, n, gpu_device)
            for skew in (0, 1, 2, 3):
                buf = torch.full((guard + skew + batch * n + guard,), fill, dtype=torch.int32, device=gpu_device)
                rbuf = torch.full((guard + batch * S * 4 + guard,), fill, dtype=torch.int32, device=gpu_device)
                _native.check(lib.ldpc_channel_sym(C.c_void_p(buf.data_ptr() + 4 * (guard + skew)), batch, n, SEED, STREAM, FIRST,
                                                   C.byref(desc), C.c_void_p(rows_t.data_ptr()), (n + 7) // 8,
                                                   C.c_void_p(rbuf.data_ptr() + 4 * guard), stream), "ldpc_channel_sym")
                host, rhost = buf.cpu().numpy(), rbuf.cpu().numpy()
                lo = guard + skew
                assert (host[:lo] == fill).all() and (host[lo + batch * n:] == fill).all(), (scheme, skew)
                assert (rhost[:guard] == fill).all() and (rhost[guard + batch * S * 4:] == fill).all(), (scheme, skew)
                assert np.array_equal(host[lo:lo + batch * n], want_llr.view(np.int32).reshape(-1)), (scheme, skew)
                assert np.array_equal(rhost[guard:guard + batch * S * 4], want_rec.view(np.int32).reshape(-1))


def test_what_the_entry_point_refuses(gpu_device):
    import _native
    import engine
    import torch_ops  # noqa: F401  (registers torch.ops.ldpc.*)
    from modulation import Modulation
    lib = _native.load()
    buf = torch.empty(256, dtype=torch.float32, device=gpu_device)
    p, off = C.c_void_p(buf.data_ptr()), lambda k: C.c_void_p(buf.data_ptr() + k)
    mod = C.byref(_native.ModulationDesc(bits_per_symbol=4, fading=0, amp=1.0))
    call = lambda llr, batch, md, rec=None: lib.ldpc_channel_sym(llr, batch, 8, 0, 0, 0, md, None, 0, rec, None)
    assert call(None, 1, mod) == -1 and b"NULL llr" in lib.ldpc_last_error()
    assert call(off(2), 1, mod) == -1 and b"4-byte" in lib.ldpc_last_error()
    assert call(p, 1, mod, off(512 + 4)) == -1 and b"16-byte" in lib.ldpc_last_error()
    assert call(p, 1, None) == -1 and b"mod" in lib.ldpc_last_error()
    # the order: scalars, then batch == 0 is OK whatever the pointers are, then the pointers
    assert call(off(2), 0, mod, off(4)) == 0 and call(None, 0, mod) == 0
    assert call(off(2), 0, C.byref(_native.ModulationDesc(bits_per_symbol=3, amp=1.0))) == -1
    assert call(off(4), 1, mod, off(512)) == 0                                         # a skewed llr is fine
    torch.cuda.synchronize()
    qpsk = Modulation("qpsk")
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=qpsk, device=gpu_device)                # neither snr_db nor amp
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=qpsk, snr_db=1.0, amp=1.0, device=gpu_device)
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation="qpsk", snr_db=1.0, device=gpu_device)
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=qpsk, snr_db=1.0, codeword=np.zeros(9), device=gpu_device)
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=Modulation("qpsk", interleaver=[1, 0]), snr_db=1.0, device=gpu_device)
    with pytest.raises(ValueError):
        engine.sym_llr(2, 8, seed=0, modulation=qpsk, amp=-1.0, device=gpu_device)
    # snr_db is amp(snr_db) rounded to fp32, and the torch op is the same call
    a = engine.sym_llr(4, 96, seed=1, stream_id=2, modulation=Modulation("qam16"), snr_db=7.0, device=gpu_device)
    b = engine.sym_llr(4, 96, seed=1, stream_id=2, modulation=Modulation("qam16"), amp=Modulation("qam16").amp(7.0),
                       device=gpu_device)
    op = torch.ops.ldpc.sym_llr(4, 96, 1, 2, 0, "qam16", False, Modulation("qam16").amp(7.0), None, None, gpu_device)
    assert torch.equal(a, b) and torch.equal(a, op)
