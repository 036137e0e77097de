"""
The counter-based AWGN channel kernel (ldpc_channel_awgn, ldpc_debug_philox) against the numpy restatement of the stream
definition (tests/philox_reference.py).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15
# |z_gpu - z_ref| with u and theta exact in fp32 and log / sqrt / sin / cos of the restatement in float64: r <= 6.76; theta's
# product rounding plus 2 ulp in sin / cos give <= 3.6e-7 in the trigonometric factor; r's own error is <= 1.2e-6; together
# about 4e-6, and the bound allows 2.4 times that
Z_TOL = 1e-5


def device_words(count, seed, stream_id, first_frame, qpf, dev):
    import _native
    out = torch.empty((count, 4), dtype=torch.int32, device=dev)
    _native.check(_native.load().ldpc_debug_philox(C.c_void_p(out.data_ptr()), count, seed, stream_id, first_frame, qpf,
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ldpc_debug_philox")
    return out.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("first_frame,frames,qpf", [(0, 5, 7), (2 ** 32 - 2, 4, 3), (2 ** 63 + 12345, 3, 500)])
def test_philox_words_equal_the_restatement(first_frame, frames, qpf, gpu_device):
    """frames 2^32 - 2 .. 2^32 + 1 cross into the high counter word"""
    got = device_words(frames * qpf, SEED, 0xfeedbeef, first_frame, qpf, gpu_device)
    want = ref.stream_words(frames, qpf, SEED, 0xfeedbeef, first_frame).reshape(-1, 4)
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("n", [1, 7, 96, 1998])
@pytest.mark.parametrize("batch", [1, 3, 67])
def test_awgn_llr_against_the_restatement(batch, n, gpu_device):
    import engine
    first = 2 ** 32 - 30                                          # the 67-frame draws cross the high counter word
    z_ref = ref.awgn_normals(batch, n, SEED, 4500, first)
    # scale 1, shift 0: fmaf(z, 1, 0) is z itself
    z = engine.awgn_llr(batch, n, seed=SEED, stream_id=4500, first_frame=first, scale=1.0, shift=0.0, device=gpu_device)
    assert z.shape == (batch, n) and z.dtype == torch.float32
    z = z.cpu().numpy()
    err = np.abs(z.astype(np.float64) - z_ref).max()
    print(f"batch {batch} n {n}: max |dz| = {err:.3e}")
    assert err <= Z_TOL
    # the LLR is fmaf(z, scale, shift) of a z within that band: fmaf is monotone in z, so it lies between the correctly
    # rounded images of the band's ends (formed in float64, whose own rounding is below a quarter ulp of the fp32 result:
    # the ends are moved outward by one fp32 step to cover it)
    scale, shift = engine.awgn_scale_shift(2.5)
    fs, fh = np.float64(np.float32(scale)), np.float64(np.float32(shift))
    llr = engine.awgn_llr(batch, n, seed=SEED, stream_id=4500, first_frame=first, snr_db=2.5, device=gpu_device).cpu().numpy()
    lo = np.nextafter(((z_ref - Z_TOL) * fs + fh).astype(np.float32), np.float32(-np.inf))
    hi = np.nextafter(((z_ref + Z_TOL) * fs + fh).astype(np.float32), np.float32(np.inf))
    assert ((llr >= lo) & (llr <= hi)).all()
    # ... and exactly fmaf of the z the kernel itself formed: the 48-bit product is exact in extended precision and the sum
    # carries 64 bits, so the one rounding to fp32 that matters is the last
    ext = z.astype(np.longdouble) * np.longdouble(fs) + np.longdouble(fh)
    np.testing.assert_array_equal(llr, ext.astype(np.float32))


def test_a_frame_gets_the_same_noise_in_any_block(gpu_device):
    import engine
    kw = dict(seed=SEED, stream_id=3000, snr_db=3.0, device=gpu_device)
    for n in (96, 1998, 7):
        whole = engine.awgn_llr(67, n, first_frame=0, **kw).cpu().numpy()
        part = engine.awgn_llr(10, n, first_frame=10, **kw).cpu().numpy()
        assert np.array_equal(whole[10:20], part)
        assert not np.array_equal(whole[0:10], part)


def test_a_codeword_mirrors_the_all_zero_draw_exactly(gpu_device):
    import engine
    rng = np.random.default_rng(1)
    for n in (7, 96, 1998):
        c = (rng.random(n) < 0.5).astype(np.uint8)
        kw = dict(seed=SEED, stream_id=1, first_frame=5, snr_db=1.0, device=gpu_device)
        zero = engine.awgn_llr(13, n, **kw).cpu().numpy()
        sent = engine.awgn_llr(13, n, codeword=c, **kw).cpu().numpy()
        assert np.array_equal(sent, zero * (1.0 - 2.0 * c.astype(np.float32))[None, :])
        assert (zero != 0).all()
        # the "reference" convention (bit 0 -> negative mean) is -shift
        scale, shift = engine.awgn_scale_shift(1.0)
        neg = engine.awgn_llr(13, n, seed=SEED, stream_id=1, first_frame=5, scale=scale, shift=-shift,
                              device=gpu_device).cpu().numpy()
        assert neg.mean() < 0 < zero.mean()


def test_stream_id_and_seed_select_different_streams(gpu_device):
    import engine
    base = engine.awgn_llr(4, 96, seed=1, stream_id=2, snr_db=3.0, device=gpu_device).cpu().numpy()
    again = engine.awgn_llr(4, 96, seed=1, stream_id=2, snr_db=3.0, device=gpu_device).cpu().numpy()
    assert np.array_equal(base, again)
    for kw in (dict(seed=1, stream_id=3), dict(seed=2, stream_id=2), dict(seed=1 + 2 ** 32, stream_id=2)):
        other = engine.awgn_llr(4, 96, snr_db=3.0, device=gpu_device, **kw).cpu().numpy()
        for r in range(4):
            assert not np.array_equal(base[r], other[r])
    import torch_ops  # noqa: F401  (registers torch.ops.ldpc.*)
    op = torch.ops.ldpc.awgn_llr(4, 96, 1, 2, 0, *engine.awgn_scale_shift(3.0), None, gpu_device)
    assert np.array_equal(op.cpu().numpy(), base)


@pytest.mark.parametrize("n", [1, 7, 96, 1998])
def test_nothing_is_written_past_the_block(n, gpu_device):
    """a block inside a larger buffer at a base that is only 4-byte aligned: the bytes before and after stay untouched"""
    import _native
    lib = _native.load()
    batch, guard = 5, 64
    for skew in (0, 1, 2, 3):                                     # base offset in floats: every store-width path
        buf = torch.full((guard + skew + batch * n + guard,), float("nan"), dtype=torch.float32, device=gpu_device)
        raw = buf.view(torch.int32)
        raw.fill_(0x7fc0dead)
        base = buf.data_ptr() + 4 * (guard + skew)
        _native.check(lib.ldpc_channel_awgn(C.c_void_p(base), batch, n, SEED, 9, 100, 1.0, 0.0, None,
                                            C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)), "ldpc_channel_awgn")
        host = raw.cpu().numpy()
        lo = guard + skew
        assert (host[:lo] == 0x7fc0dead).all() and (host[lo + batch * n:] == 0x7fc0dead).all()
        want = ref.awgn_normals(batch, n, SEED, 9, 100)
        got = host[lo:lo + batch * n].view(np.float32).reshape(batch, n)
        assert np.abs(got.astype(np.float64) - want).max() <= Z_TOL


def test_what_the_channel_entry_point_refuses(gpu_device):
    import _native
    lib = _native.load()
    buf = torch.empty(64, dtype=torch.float32, device=gpu_device)
    p = C.c_void_p(buf.data_ptr())
    assert lib.ldpc_channel_awgn(p, -1, 8, 0, 0, 0, 1.0, 0.0, None, None) == -1 and b"batch" in lib.ldpc_last_error()
    assert lib.ldpc_channel_awgn(p, 1, 0, 0, 0, 0, 1.0, 0.0, None, None) == -1 and b"n < 1" in lib.ldpc_last_error()
    assert lib.ldpc_channel_awgn(None, 1, 8, 0, 0, 0, 1.0, 0.0, None, None) == -1 and b"NULL" in lib.ldpc_last_error()
    assert lib.ldpc_channel_awgn(C.c_void_p(buf.data_ptr() + 2), 1, 8, 0, 0, 0, 1.0, 0.0, None, None) == -1
    assert lib.ldpc_channel_awgn(p, 0, 8, 0, 0, 0, 1.0, 0.0, None, None) == 0          # an empty block is no error
    assert lib.ldpc_debug_philox(None, 4, 0, 0, 0, 1, None) == -1
    assert lib.ldpc_debug_philox(p, 4, 0, 0, 0, 0, None) == -1
    import engine
    with pytest.raises(ValueError):
        engine.awgn_llr(2, 8, seed=0, device=gpu_device)                               # neither snr_db nor (scale, shift)
    with pytest.raises(ValueError):
        engine.awgn_llr(2, 8, seed=0, snr_db=1.0, scale=1.0, shift=1.0, device=gpu_device)
    with pytest.raises(ValueError):
        engine.awgn_llr(2, 8, seed=0, snr_db=1.0, codeword=np.zeros(9), device=gpu_device)
