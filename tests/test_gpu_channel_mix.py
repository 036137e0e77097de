"""
The mixed-SNR channel kernel (ldpc_channel_awgn_mix, engine.awgn_llr_mix, torch.ops.ldpc.awgn_llr_mix): frame f is drawn
at point f % K of a table.  The yardstick is the single-point channel ldpc_channel_awgn, which tests/test_gpu_sim_channel.py
pins against the numpy restatement tests/philox_reference.py: rows of a mixed block equal, bit for bit, the same rows of a
single-point block at that point's (scale, shift).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0x9e3779b97f4a7c15
Z_TOL = 1e-5            # tests/test_gpu_sim_channel.py derives it for these normals; scale 1, shift 0 leaves them as they are
FIRSTS = (0, 2 ** 32 - 30, 2 ** 63 + 12345)      # 67 frames from 2^32 - 30 cross into the high counter word


def tables(K):
    """distinct scales and shifts per point, some shifts negative (the reference's literal channel)"""
    k = np.arange(K, dtype=np.float64)
    return 0.75 + 0.37 * k, (1.5 + 0.61 * k) * np.where(k % 2 == 0, 1.0, -1.0)


def stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


@pytest.mark.parametrize("n", [1, 7, 96, 1998])
@pytest.mark.parametrize("batch", [1, 67])
def test_rows_equal_the_single_point_channel(batch, n, gpu_device):
    import engine
    for K in (1, 3, 13):
        scale, shift = tables(K)
        for first in FIRSTS:
            kw = dict(seed=SEED, stream_id=77, first_frame=first, device=gpu_device)
            mix = engine.awgn_llr_mix(batch, n, scale=scale, shift=shift, **kw)
            assert mix.shape == (batch, n) and mix.dtype == torch.float32
            mix = mix.cpu().numpy()
            point = np.array([(first + b) % K for b in range(batch)])
            np.testing.assert_array_equal(engine.mix_points(first, batch, K).numpy(), point)
            for p in sorted(set(point.tolist())):
                one = engine.awgn_llr(batch, n, scale=float(np.float32(scale[p])), shift=float(np.float32(shift[p])), **kw)
                rows = point == p
                assert np.array_equal(mix[rows], one.cpu().numpy()[rows]), (K, first, p)
            if K == 1:
                assert (point == 0).all()                         # ... which made the comparison above the whole block


def test_snr_tables_are_the_single_point_conversion(gpu_device):
    import engine
    grid = engine.snr_grid((0.0, 6.0), 0.5)
    for convention in ("decoder", "reference"):
        mix = engine.awgn_llr_mix(26, 96, seed=3, first_frame=5, snr_db=grid, llr_convention=convention, device=gpu_device)
        for b in (0, 7, 8, 25):
            scale, shift = engine.awgn_scale_shift(grid[(5 + b) % 13], convention)
            one = engine.awgn_llr(1, 96, seed=3, first_frame=5 + b, scale=scale, shift=shift, device=gpu_device)
            assert torch.equal(mix[b:b + 1], one)
        assert (float(mix.mean()) > 0) == (convention == "decoder")
    st, ht = engine.awgn_mix_tables(grid, device=gpu_device)
    assert st.dtype == torch.float32 and st.shape == (13,) and ht.shape == (13,)
    again = engine.awgn_llr_mix(26, 96, seed=3, first_frame=5, scale=st, shift=ht, device=gpu_device)
    assert torch.equal(again, engine.awgn_llr_mix(26, 96, seed=3, first_frame=5, snr_db=grid, device=gpu_device))


@pytest.mark.parametrize("n", [7, 1998])
def test_normals_against_the_restatement(n, gpu_device):
    import engine
    first, batch = 2 ** 32 - 30, 67
    z = engine.awgn_llr_mix(batch, n, seed=SEED, stream_id=4500, first_frame=first, scale=np.ones(13), shift=np.zeros(13),
                            device=gpu_device).cpu().numpy()
    err = np.abs(z.astype(np.float64) - ref.awgn_normals(batch, n, SEED, 4500, first)).max()
    print(f"n {n}: max |dz| = {err:.3e}")
    assert err <= Z_TOL


@pytest.mark.parametrize("K", [3, 13])
def test_a_frame_gets_the_same_noise_and_point_in_any_block(K, gpu_device):
    import engine
    scale, shift = tables(K)
    kw = dict(seed=SEED, stream_id=3000, scale=scale, shift=shift, device=gpu_device)
    for n in (96, 1998, 7):
        whole = engine.awgn_llr_mix(67, n, first_frame=5, **kw).cpu().numpy()
        part = engine.awgn_llr_mix(10, n, first_frame=15, **kw).cpu().numpy()
        assert np.array_equal(whole[10:20], part)
        assert not np.array_equal(whole[0:10], part)


def test_a_codeword_mirrors_the_all_zero_draw_exactly(gpu_device):
    import engine
    rng = np.random.default_rng(1)
    scale, shift = tables(3)
    for n in (7, 96, 1998):
        c = (rng.random(n) < 0.5).astype(np.uint8)
        kw = dict(seed=SEED, stream_id=1, first_frame=5, scale=scale, shift=shift, device=gpu_device)
        zero = engine.awgn_llr_mix(13, n, **kw).cpu().numpy()
        sent = engine.awgn_llr_mix(13, n, codeword=c, **kw).cpu().numpy()
        assert c.any() and np.array_equal(sent, zero * (1.0 - 2.0 * c.astype(np.float32))[None, :])
        assert (zero != 0).all()
        packed = engine.pack_codeword(c, n, gpu_device)
        assert np.array_equal(engine.awgn_llr_mix(13, n, codeword=packed, **kw).cpu().numpy(), sent)


@pytest.mark.parametrize("n", [1, 7, 1998])
def test_nothing_is_written_past_the_block(n, gpu_device):
    """a block inside a larger buffer at a base that is only 4-byte aligned: the words before and after stay untouched, and the
    block is what an aligned draw gives"""
    import _native
    import engine
    lib = _native.load()
    batch, guard, K = 5, 64, 3
    scale, shift = tables(K)
    st, ht = (torch.from_numpy(t.astype(np.float32)).to(gpu_device) for t in (scale, shift))
    want = engine.awgn_llr_mix(batch, n, seed=SEED, stream_id=9, first_frame=100, scale=st, shift=ht, device=gpu_device)
    want = want.cpu().numpy().view(np.int32).reshape(-1)
    for skew in (0, 1, 2, 3):                                     # base offset in floats: every store-width path
        buf = torch.empty((guard + skew + batch * n + guard,), dtype=torch.float32, device=gpu_device)
        raw = buf.view(torch.int32)
        raw.fill_(0x7fc0dead)
        base = buf.data_ptr() + 4 * (guard + skew)
        _native.check(lib.ldpc_channel_awgn_mix(C.c_void_p(base), batch, n, SEED, 9, 100, C.c_void_p(st.data_ptr()),
                                                C.c_void_p(ht.data_ptr()), K, None, stream(gpu_device)), "ldpc_channel_awgn_mix")
        host = raw.cpu().numpy()
        lo = guard + skew
        assert (host[:lo] == 0x7fc0dead).all() and (host[lo + batch * n:] == 0x7fc0dead).all()
        assert np.array_equal(host[lo:lo + batch * n], want)


def test_the_operator_equals_the_host_function(gpu_device):
    import engine
    import torch_ops  # noqa: F401  (registers torch.ops.ldpc.*)
    st, ht = engine.awgn_mix_tables(engine.snr_grid((1.0, 4.0), 0.5), device=gpu_device)
    cw = engine.pack_codeword(np.arange(96) % 3 == 0, 96, gpu_device)
    for codeword in (None, cw):
        op = torch.ops.ldpc.awgn_llr_mix(20, 96, 11, 2, 1000, st, ht, codeword, gpu_device)
        want = engine.awgn_llr_mix(20, 96, seed=11, stream_id=2, first_frame=1000, scale=st, shift=ht, codeword=codeword,
                                   device=gpu_device)
        assert torch.equal(op, want)
        torch.library.opcheck(torch.ops.ldpc.awgn_llr_mix, (20, 96, 11, 2, 1000, st, ht, codeword, gpu_device),
                              test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))


def test_what_the_entry_point_refuses(gpu_device):
    import _native
    lib = _native.load()
    buf = torch.empty(64, dtype=torch.float32, device=gpu_device)
    buf.view(torch.int32).fill_(0x7fc0dead)
    tab = torch.ones(8, dtype=torch.float32, device=gpu_device)
    p, t = C.c_void_p(buf.data_ptr()), C.c_void_p(tab.data_ptr())
    p2, t2 = C.c_void_p(buf.data_ptr() + 2), C.c_void_p(tab.data_ptr() + 2)

    def refused(word, llr, batch, n, first, st, ht, K):
        assert lib.ldpc_channel_awgn_mix(llr, batch, n, 0, 0, first, st, ht, K, None, None) == -1
        assert word in lib.ldpc_last_error(), lib.ldpc_last_error()

    refused(b"batch < 0", p, -1, 8, 0, t, t, 1)
    refused(b"batch >", p, 2 ** 31, 8, 0, t, t, 1)
    refused(b"n < 1", p, 1, 0, 0, t, t, 1)
    refused(b"n_points", p, 1, 8, 0, t, t, 0)
    refused(b"n_points", p, 1, 8, 0, t, t, 4097)
    refused(b"first_frame", p, 4, 8, 2 ** 64 - 3, t, t, 1)
    # the order of the checks: the earlier one names itself
    refused(b"batch < 0", None, -1, 0, 0, None, None, 0)
    refused(b"batch >", None, 2 ** 31, 0, 0, None, None, 0)
    refused(b"n < 1", None, 4, 0, 2 ** 64 - 1, None, None, 0)
    refused(b"n_points", None, 4, 8, 2 ** 64 - 1, None, None, 0)
    refused(b"first_frame", None, 4, 8, 2 ** 64 - 1, None, None, 1)
    refused(b"n_points", None, 0, 8, 0, None, None, 0)                                     # ... before the empty block returns
    # an empty block is no error and touches no pointer, at any first frame
    assert lib.ldpc_channel_awgn_mix(None, 0, 8, 0, 0, 2 ** 64 - 1, None, None, 1, None, None) == 0
    refused(b"NULL llr", None, 1, 8, 0, t, t, 1)
    refused(b"llr", p2, 1, 8, 0, t, t, 1)
    refused(b"scale_tab", p, 1, 8, 0, None, t, 1)
    refused(b"shift_tab", p, 1, 8, 0, t, None, 1)
    refused(b"scale_tab", p, 1, 8, 0, t2, t, 1)
    refused(b"shift_tab", p, 1, 8, 0, t, t2, 1)
    torch.cuda.synchronize(gpu_device)
    assert (buf.view(torch.int32) == 0x7fc0dead).all()                                     # no refusal wrote anything
    # the last frames of the 64-bit index are drawn: 2^64 - 4 .. 2^64 - 1 do not wrap
    assert lib.ldpc_channel_awgn_mix(p, 4, 8, 0, 0, 2 ** 64 - 4, t, t, 1, None, stream(gpu_device)) == 0
    import engine
    top = engine.awgn_llr(4, 8, seed=0, first_frame=2 ** 64 - 4, scale=1.0, shift=1.0, device=gpu_device)
    assert torch.equal(buf[:32].view(4, 8), top) and (buf.view(torch.int32)[32:] == 0x7fc0dead).all()


def test_what_the_host_function_refuses(gpu_device):
    import engine
    kw = dict(seed=0, device=gpu_device)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, **kw)                                                    # neither snr_db nor tables
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, scale=[1.0], **kw)                                       # a scale without a shift
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, snr_db=[1.0], scale=[1.0], shift=[1.0], **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, scale=[1.0, 2.0], shift=[1.0], **kw)                     # unequal lengths
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, snr_db=[], **kw)                                         # no point
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, snr_db=np.zeros(4097), **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, snr_db=[[1.0, 2.0]], **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, snr_db=[1.0], llr_convention="other", **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(-1, 8, snr_db=[1.0], **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 0, snr_db=[1.0], **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2 ** 31, 8, snr_db=[1.0], **kw)
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, snr_db=[1.0], codeword=np.zeros(9), **kw)
    with pytest.raises(ValueError, match="first_frame"):
        engine.awgn_llr_mix(4, 8, snr_db=[1.0], first_frame=2 ** 64 - 3, **kw)             # the native refusal, as ValueError
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, scale=torch.ones(2), shift=torch.ones(2), **kw)          # tables on the host
    with pytest.raises(ValueError):
        engine.awgn_llr_mix(2, 8, scale=torch.ones(2, dtype=torch.float64, device=gpu_device),
                            shift=torch.ones(2, dtype=torch.float64, device=gpu_device), **kw)
    assert engine.awgn_llr_mix(0, 8, snr_db=[1.0, 2.0], **kw).shape == (0, 8)
