"""
GPU tests (-m gpu) of the mixed-SNR symbol channel kernel (ldpc_channel_sym_mix, engine.sym_llr_mix).  The yardstick is the
one-point kernel ldpc_channel_sym (engine.sym_llr), which tests/test_gpu_channel_sym.py pins to the numpy restatement of the
definition: a frame of the mix draw must equal, bit for bit, the one-point draw of that frame at the amp of its point, and the
targets must be the bits that were sent.  Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import encode_reference as eref
import modulation_reference as mref

pytestmark = pytest.mark.gpu

SEED, STREAM = 0x9e3779b97f4a7c15, 4600
FIRST = 2 ** 32 - 30                                  # 67 frames cross into the high counter word
NS, BATCHES = (1, 7, 96, 1998), (1, 3, 67)
SCHEMES = tuple(sorted(mref.SCHEMES.items(), key=lambda kv: kv[1]))          # (name, m), m = 1, 2, 4, 6, 8


def table(K):
    """well separated amplitudes: a wrong point cannot pass"""
    return (0.5 + 0.37 * np.arange(K)).astype(np.float32)


def rows_for(n, batch, dev, first=FIRST):
    """packed rows of encode_random where the package has a code of this n, random rows elsewhere -> (tensor, 0/1 [batch, n])"""
    import codes
    import engine
    name = {96: "small_96_48", 1998: "ira_1998_1512"}.get(n)
    if name:
        enc = codes.Encoder.from_graph(codes.load_graph(name))
        cw = engine.encode_random(enc, batch, seed=SEED, stream_id=STREAM, first_frame=first, device=dev)
        return cw, eref.unpack_rows(cw.cpu().numpy(), n)
    bits = (np.random.default_rng(n + batch).random((batch, n)) < 0.5).astype(np.uint8)
    return torch.from_numpy(eref.pack_rows(bits)).to(dev), bits


def mix(batch, n, mod, dev, *, amp, codeword=None, first=FIRST, want_targets=False):
    import engine
    return engine.sym_llr_mix(batch, n, seed=SEED, stream_id=STREAM, first_frame=first, modulation=mod, amp=amp,
                              codeword=codeword, device=dev, want_targets=want_targets)


def one_point(batch, n, mod, dev, *, amp, codeword=None, first=FIRST):
    import engine
    return engine.sym_llr(batch, n, seed=SEED, stream_id=STREAM, first_frame=first, modulation=mod, amp=amp, codeword=codeword,
                          device=dev)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def mods(n):
    from modulation import Modulation
    pos = np.random.default_rng(31 * n + 1).permutation(n)
    for scheme, m in SCHEMES:
        for fading in (None, "rayleigh"):
            for p in (None, pos):
                yield Modulation(scheme, fading, p)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_every_frame_is_the_one_point_draw_at_its_point(batch, n, gpu_device):
    import engine
    rows_t, _ = rows_for(n, batch, gpu_device)
    for K in (1, 3, 13):
        tab = table(K)
        points = engine.mix_points(FIRST, batch, K, device=gpu_device)
        assert points.tolist() == [(FIRST + b) % K for b in range(batch)]
        for mod in mods(n):
            got = mix(batch, n, mod, gpu_device, amp=tab, codeword=rows_t)
            assert got.shape == (batch, n) and got.dtype == torch.float32
            seen = 0
            for p in range(K):
                want = one_point(batch, n, mod, gpu_device, amp=float(tab[p]), codeword=rows_t)
                sel = points == p
                seen += int(sel.sum())
                assert same_bits(got[sel], want[sel]), (K, p, mod)
                if K == 1:
                    assert same_bits(got, want)
            assert seen == batch


def test_the_table_on_the_device_and_snr_db_are_the_same_call(gpu_device):
    import engine
    from modulation import Modulation
    mod = Modulation("qam64", "rayleigh")
    grid = engine.snr_grid((2.0, 14.0), 1.0)
    tab = mod.amp_table(grid)
    kw = dict(seed=SEED, stream_id=STREAM, first_frame=FIRST, modulation=mod, device=gpu_device)
    a = engine.sym_llr_mix(67, 96, snr_db=grid, **kw)
    b = engine.sym_llr_mix(67, 96, amp=tab, **kw)
    c = engine.sym_llr_mix(67, 96, amp=torch.from_numpy(tab).to(gpu_device), **kw)
    assert same_bits(a, b) and same_bits(a, c)
    points = engine.mix_points(FIRST, 67, len(grid)).tolist()
    for b_ in (0, 29, 30, 66):                          # snr_db of the mix is snr_db of the one-point call, frame by frame
        one = engine.sym_llr(1, 96, seed=SEED, stream_id=STREAM, first_frame=FIRST + b_, modulation=mod,
                             snr_db=float(grid[points[b_]]), device=gpu_device)
        assert same_bits(a[b_:b_ + 1], one)
    with pytest.raises(ValueError):
        engine.sym_llr_mix(4, 96, amp=torch.from_numpy(tab.astype(np.float64)).to(gpu_device), **kw)
    with pytest.raises(ValueError):
        engine.sym_llr_mix(4, 96, amp=torch.from_numpy(tab), **kw)                         # a host tensor
    assert engine.sym_llr_mix(0, 96, amp=tab, **kw).shape == (0, 96)


@pytest.mark.parametrize("first", [0, 4095, 2 ** 32 - 30, 2 ** 63 + 5, 2 ** 64 - 67])
def test_remainder_at_4096_points(first, gpu_device):
    from modulation import Modulation
    K, batch, n = 4096, 67, 7
    tab = table(K)
    mod = Modulation("qpsk")
    rows_t, _ = rows_for(n, batch, gpu_device)
    got = mix(batch, n, mod, gpu_device, amp=tab, codeword=rows_t, first=first)
    for b in range(batch):
        p = (first + b) % K                                                             # Python integers
        want = one_point(1, n, mod, gpu_device, amp=float(tab[p]), codeword=rows_t[b], first=first + b)
        assert same_bits(got[b:b + 1], want), (first, b, p)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("batch", BATCHES)
def test_targets_are_the_bits_that_were_sent(batch, n, gpu_device):
    rows_t, rows = rows_for(n, batch, gpu_device)
    one = (np.random.default_rng(5).random(n) < 0.5).astype(np.uint8)
    tab = table(3)
    want_rows = torch.from_numpy(rows.astype(np.float32)).to(gpu_device)
    want_one = torch.from_numpy(np.broadcast_to(one, (batch, n)).astype(np.float32).copy()).to(gpu_device)
    for mod in mods(n):                                  # the identity path and an interleaver, both fadings
        llr, t = mix(batch, n, mod, gpu_device, amp=tab, codeword=rows_t, want_targets=True)
        assert t.shape == (batch, n) and t.dtype == torch.float32
        assert same_bits(t, want_rows), mod              # exactly 0.0f / 1.0f: the bit patterns 0 and 0x3f800000
        assert same_bits(llr, mix(batch, n, mod, gpu_device, amp=tab, codeword=rows_t)), mod       # the LLRs do not care
        _, t = mix(batch, n, mod, gpu_device, amp=tab, codeword=one, want_targets=True)
        assert same_bits(t, want_one), mod
        _, t = mix(batch, n, mod, gpu_device, amp=tab, want_targets=True)
        assert (t.view(torch.int32) == 0).all(), mod     # the all-zero word: +0.0


@pytest.mark.parametrize("n", NS)
def test_hard_decisions_at_amp_8_are_the_targets(n, gpu_device):
    """|z| <= 6.76 < 8 = half the spacing between neighbouring points: without fading every symbol stays in its own cell"""
    from modulation import Modulation
    batch = 67
    rows_t, _ = rows_for(n, batch, gpu_device)
    pos = np.random.default_rng(n).permutation(n)
    for scheme, m in SCHEMES:
        for p in (None, pos):
            llr, t = mix(batch, n, Modulation(scheme, None, p), gpu_device, amp=[8.0, 8.0, 8.0], codeword=rows_t,
                         want_targets=True)
            assert (llr != 0).all() and torch.equal((llr < 0).float(), t), (scheme, p is not None)


@pytest.mark.parametrize("n", [7, 1998])
def test_nothing_is_written_past_either_block(n, gpu_device):
    """llr and targets inside larger buffers at bases 0, 1, 2 and 3 floats past an aligned address, independently: the words
    before and after stay untouched and each block holds what a plain call returns.  n = 1998 with m = 6 puts every row of the
    batch at another store alignment; n = 7 ends every row in a partial symbol."""
    import _native
    from modulation import Modulation
    lib = _native.load()
    batch, guard, fill, K = 5, 64, 0x7fc0dead, 3
    rows_t, _ = rows_for(n, batch, gpu_device)
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    tab = torch.from_numpy(table(K)).to(gpu_device)
    pos = np.random.default_rng(n + 1).permutation(n)
    for scheme in ("qam16", "qam64", "qam256"):
        for p in (None, pos):
            mod = Modulation(scheme, "rayleigh", p)
            want_llr, want_t = mix(batch, n, mod, gpu_device, amp=tab, codeword=rows_t, want_targets=True)
            want_llr, want_t = want_llr.view(torch.int32).reshape(-1), want_t.view(torch.int32).reshape(-1)
            desc, keep = mod.native(0.0, n, gpu_device)
            for skew in (0, 1, 2, 3):
                for tskew in (0, 1, 2, 3):
                    buf = torch.full((guard + skew + batch * n + guard,), fill, dtype=torch.int32, device=gpu_device)
                    tbuf = torch.full((guard + tskew + batch * n + guard,), fill, dtype=torch.int32, device=gpu_device)
                    _native.check(lib.ldpc_channel_sym_mix(C.c_void_p(buf.data_ptr() + 4 * (guard + skew)), batch, n, SEED,
                                                           STREAM, FIRST, C.byref(desc), C.c_void_p(tab.data_ptr()), K,
                                                           C.c_void_p(rows_t.data_ptr()), (n + 7) // 8,
                                                           C.c_void_p(tbuf.data_ptr() + 4 * (guard + tskew)), stream),
                                  "ldpc_channel_sym_mix")
                    lo, tlo = guard + skew, guard + tskew
                    assert (buf[:lo] == fill).all() and (buf[lo + batch * n:] == fill).all(), (scheme, skew, tskew)
                    assert (tbuf[:tlo] == fill).all() and (tbuf[tlo + batch * n:] == fill).all(), (scheme, skew, tskew)
                    assert torch.equal(buf[lo:lo + batch * n], want_llr), (scheme, skew, tskew)
                    assert torch.equal(tbuf[tlo:tlo + batch * n], want_t), (scheme, skew, tskew)


def test_a_frame_gets_the_same_llrs_and_targets_in_any_block(gpu_device):
    from modulation import Modulation
    tab = table(13)
    for n in (96, 1998, 7):
        rows_t, _ = rows_for(n, 67, gpu_device)
        pos = np.random.default_rng(n + 2).permutation(n)
        for scheme, m in SCHEMES:
            for fading, p in ((None, None), ("rayleigh", pos)):
                mod = Modulation(scheme, fading, p)
                whole, wt = mix(67, n, mod, gpu_device, amp=tab, codeword=rows_t, want_targets=True)
                part, pt = mix(10, n, mod, gpu_device, amp=tab, codeword=rows_t[10:20].contiguous(), first=FIRST + 10,
                               want_targets=True)
                assert same_bits(whole[10:20], part) and same_bits(wt[10:20], pt), (n, scheme, fading)
                assert not same_bits(whole[0:10], part)


def test_what_the_entry_point_refuses(gpu_device):
    import _native
    lib = _native.load()
    buf = torch.empty(512, dtype=torch.float32, device=gpu_device)
    tab = torch.ones(16, dtype=torch.float32, device=gpu_device)
    p, off = C.c_void_p(buf.data_ptr()), lambda k: C.c_void_p(buf.data_ptr() + k)
    tp = C.c_void_p(tab.data_ptr())
    mod = C.byref(_native.ModulationDesc(bits_per_symbol=4, fading=0, amp=-1.0))              # mod->amp is ignored
    call = lambda llr, batch, md=mod, t=tp, k=13, stride=0, targets=None: lib.ldpc_channel_sym_mix(
        llr, batch, 8, 0, 0, 0, md, t, k, None, stride, targets, None)
    assert call(p, 1, k=0) == -1 and b"n_points" in lib.ldpc_last_error()
    assert call(p, 1, k=4097) == -1 and b"n_points" in lib.ldpc_last_error()
    assert call(p, 1, t=None) == -1 and b"amp_tab" in lib.ldpc_last_error()
    assert call(p, 1, stride=2) == -1 and b"codeword_stride" in lib.ldpc_last_error()
    assert call(p, 1, targets=off(1024 + 2)) == -1 and b"targets" in lib.ldpc_last_error()
    assert call(p, 1, md=C.byref(_native.ModulationDesc(bits_per_symbol=3, amp=1.0))) == -1
    assert b"bits_per_symbol" in lib.ldpc_last_error()
    assert call(p, 1, md=C.byref(_native.ModulationDesc(bits_per_symbol=4, fading=2))) == -1
    assert call(p, 1, md=None) == -1 and b"mod" in lib.ldpc_last_error()
    assert call(None, 1) == -1 and b"NULL llr" in lib.ldpc_last_error()
    assert call(off(2), 1) == -1 and b"4-byte" in lib.ldpc_last_error()
    assert call(p, 2 ** 31) == -1 and b"2^31" in lib.ldpc_last_error()
    assert lib.ldpc_channel_sym_mix(p, 2, 8, 0, 0, 2 ** 64 - 1, mod, tp, 13, None, 0, None, None) == -1
    assert b"wraps" in lib.ldpc_last_error()
    # the order: scalars, then batch == 0 is OK whatever the pointers are, then the pointers
    assert call(None, 0, t=None) == 0 and call(off(2), 0, targets=off(6)) == 0
    assert call(off(2), 0, k=0) == -1
    assert call(off(4), 1, targets=off(1024 + 4)) == 0                                  # skewed outputs are fine
    torch.cuda.synchronize()
    assert lib.ldpc_abi_version() == 1
