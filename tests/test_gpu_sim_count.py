"""
The device-side error counters (ldpc_sim_count) against the restated in-order fold of tests/philox_reference.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_reference as ref

pytestmark = pytest.mark.gpu


def count(state, packed, iters, n, max_frames, max_errors, cw, dev):
    """one ldpc_sim_count through the raw entry point (no engine needed) -> the state as python ints"""
    import _native
    st = torch.tensor(state, dtype=torch.int64, device=dev)
    p = torch.from_numpy(np.ascontiguousarray(packed)).to(dev)
    it = torch.from_numpy(np.ascontiguousarray(iters, dtype=np.int32)).to(dev)
    c = None if cw is None else torch.from_numpy(cw).to(dev)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    _native.check(_native.load().ldpc_sim_count(ptr(st), ptr(p), ptr(it), p.shape[0], n, ptr(c), max_frames, max_errors,
                                                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ldpc_sim_count")
    return st.tolist()


def synthetic(rng, B, n, p_err, garbage=True):
    """packed rows uint8 [B, ceil(n/8)]: a share p_err of the frames has a few wrong bits (bit n-1 among them now and then);
    the pad bits of the last byte hold garbage"""
    bits = np.zeros((B, n), dtype=np.uint8)
    bad = rng.random(B) < p_err
    for b in np.nonzero(bad)[0]:
        k = int(rng.integers(1, min(n, 40) + 1))
        bits[b, rng.choice(n, size=k, replace=False)] = 1
        if rng.random() < 0.3:
            bits[b, n - 1] = 1
    pad = (rng.random((B, (-n) % 8)) < 0.5 if garbage else np.zeros((B, (-n) % 8))).astype(np.uint8)
    return np.packbits(np.concatenate([bits, pad], axis=1), axis=1, bitorder="little"), bits


@pytest.mark.parametrize("with_codeword", [False, True])
@pytest.mark.parametrize("n", [7, 96, 1998])
@pytest.mark.parametrize("B", [1, 64, 1025])
def test_one_block_against_the_restated_fold(B, n, with_codeword, gpu_device):
    rng = np.random.default_rng(B * 10007 + n)
    cw_bits = (rng.random(n) < 0.5).astype(np.uint8) if with_codeword else np.zeros(n, np.uint8)
    cw_pad = np.concatenate([cw_bits, np.ones((-n) % 8, np.uint8)])                 # garbage in the codeword's pad bits too
    cw = np.packbits(cw_pad, bitorder="little") if with_codeword else None
    for p_err in (0.0, 0.1, 1.0):
        packed, err_bits = synthetic(rng, B, n, p_err)
        if with_codeword:
            packed = packed ^ cw[None, :]
        iters = rng.integers(1, 11, B)
        wrong = ref.wrong_bits(packed, n, cw)
        np.testing.assert_array_equal(wrong, err_bits.sum(axis=1))
        n_err = int((wrong > 0).sum())
        # no limit in reach; the frame limit mid-block; the error limit mid-block and on the very last erroneous frame
        limits = [(10 ** 6, 10 ** 6), (max(1, B // 2), 10 ** 6), (B, 10 ** 6)]
        if n_err:
            limits += [(10 ** 6, max(1, n_err // 2)), (10 ** 6, n_err), (10 ** 6, n_err + 1), (max(1, B - 1), n_err)]
        for max_frames, max_errors in limits:
            state = [0] * 8
            got = count(state, packed, iters, n, max_frames, max_errors, cw, gpu_device)
            assert got == ref.sim_fold(state, wrong, iters, max_frames, max_errors), (p_err, max_frames, max_errors)


def test_error_limit_on_the_very_last_frame_of_a_block(gpu_device):
    n, B = 1998, 1025
    rng = np.random.default_rng(3)
    packed, _ = synthetic(rng, B, n, 0.0)
    packed[[5, 700, B - 1], 249] |= 0x20                                             # bit 1997: the last bit of the codeword
    iters = rng.integers(1, 11, B)
    wrong = ref.wrong_bits(packed, n)
    assert list(np.nonzero(wrong)[0]) == [5, 700, B - 1]
    for start, max_errors, frames in (([0] * 8, 3, B), ([40, 7, 90, 300, 0, 2, 0, 0], 10, 40 + B), ([0] * 8, 2, 701)):
        got = count(start, packed, iters, n, 10 ** 6, max_errors, None, gpu_device)
        assert got == ref.sim_fold(start, wrong, iters, 10 ** 6, max_errors)
        assert got[0] == frames and got[4] == 1


def test_point_already_done_and_zero_limits(gpu_device):
    n, B = 96, 64
    rng = np.random.default_rng(4)
    packed, _ = synthetic(rng, B, n, 0.5)
    iters = rng.integers(1, 11, B)
    wrong = ref.wrong_bits(packed, n)
    for state, max_frames, max_errors in (([14, 5, 27, 70, 1, 2, 0, 0], 1000, 50),      # done: only blocks_seen moves
                                          ([100, 0, 0, 300, 0, 1, 0, 0], 100, 5),         # limits met, flag not yet set
                                          ([30, 5, 9, 300, 0, 1, 0, 0], 100, 5),
                                          ([0] * 8, 100, 0),                              # max_errors = 0
                                          ([0] * 8, 0, 10)):
        got = count(state, packed, iters, n, max_frames, max_errors, None, gpu_device)
        assert got == ref.sim_fold(state, wrong, iters, max_frames, max_errors)
        assert got[:4] == state[:4] and got[4] == 1 and got[5] == state[5] + 1


@pytest.mark.parametrize("n", [7, 1998])
def test_state_carried_over_launches(n, gpu_device):
    """three blocks folded into one state on the device, then a launch after `done`"""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    rng = np.random.default_rng(n)
    blocks = [synthetic(rng, B, n, 0.05)[0] for B in (1025, 64, 1025)]
    iters = [rng.integers(1, 11, len(b)).astype(np.int32) for b in blocks]
    total_err = sum(int((ref.wrong_bits(b, n) > 0).sum()) for b in blocks)
    first_two = sum(int((ref.wrong_bits(b, n) > 0).sum()) for b in blocks[:2])
    assert total_err > first_two + 2
    eng = BasicMinSumDecoder(codes.load_code("small_96_48", 10), 0.7)._engine(torch.float32, gpu_device)
    eng_n = eng.graph.n
    for max_frames, max_errors in ((10 ** 6, 10 ** 6), (1025 + 64 + 500, 10 ** 6), (10 ** 6, first_two + 2)):
        state = torch.zeros(8, dtype=torch.int64, device=gpu_device)
        want = [0] * 8
        ptr = lambda t: C.c_void_p(t.data_ptr())
        for b, it in list(zip(blocks, iters)) + [(blocks[0], iters[0])]:
            pb, pi = torch.from_numpy(b).to(gpu_device), torch.from_numpy(it).to(gpu_device)
            if n == eng_n:
                eng.sim_count(state, pb, pi, max_frames=max_frames, max_errors=max_errors)
            else:
                import _native
                _native.check(eng._lib.ldpc_sim_count(ptr(state), ptr(pb), ptr(pi), len(b), n, None, max_frames, max_errors,
                                                      C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)),
                              "ldpc_sim_count")
            want = ref.sim_fold(want, ref.wrong_bits(b, n), it, max_frames, max_errors)
        assert state.tolist() == want
        if max_errors < 10 ** 6 or max_frames < 10 ** 6:
            assert want[4] == 1


def test_engine_sim_count_with_a_codeword(gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    eng = BasicMinSumDecoder(codes.load_code("small_96_48", 10), 0.7)._engine(torch.float32, gpu_device)
    n = eng.graph.n
    rng = np.random.default_rng(8)
    c = (rng.random(n) < 0.5).astype(np.uint8)
    cw = np.packbits(c, bitorder="little")
    packed, _ = synthetic(rng, 300, n, 0.2)
    packed = packed ^ cw[None, :]
    iters = rng.integers(1, 11, 300).astype(np.int32)
    state = torch.zeros(8, dtype=torch.int64, device=gpu_device)
    out = eng.sim_count(state, torch.from_numpy(packed).to(gpu_device), torch.from_numpy(iters).to(gpu_device),
                        max_frames=250, max_errors=10 ** 6, codeword=c)
    assert out is state and state.tolist() == ref.sim_fold([0] * 8, ref.wrong_bits(packed, n, cw), iters, 250, 10 ** 6)
    with pytest.raises(ValueError):
        eng.sim_count(state.to(torch.int32), torch.from_numpy(packed).to(gpu_device), torch.from_numpy(iters).to(gpu_device),
                      max_frames=1, max_errors=1)
    with pytest.raises(ValueError):
        eng.sim_count(state, torch.from_numpy(packed[:, :-1].copy()).to(gpu_device), torch.from_numpy(iters).to(gpu_device),
                      max_frames=1, max_errors=1)


def test_what_the_counter_entry_point_refuses(gpu_device):
    import _native
    lib = _native.load()
    st = torch.zeros(8, dtype=torch.int64, device=gpu_device)
    pk = torch.zeros((4, 12), dtype=torch.uint8, device=gpu_device)
    it = torch.ones(4, dtype=torch.int32, device=gpu_device)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.ldpc_sim_count(p(st), p(pk), p(it), -1, 96, None, 10, 10, None) == -1 and b"batch" in lib.ldpc_last_error()
    assert lib.ldpc_sim_count(p(st), p(pk), p(it), 4, 0, None, 10, 10, None) == -1 and b"n < 1" in lib.ldpc_last_error()
    assert lib.ldpc_sim_count(None, p(pk), p(it), 4, 96, None, 10, 10, None) == -1 and b"NULL" in lib.ldpc_last_error()
    assert lib.ldpc_sim_count(p(st), None, p(it), 4, 96, None, 10, 10, None) == -1
    assert lib.ldpc_sim_count(p(st), p(pk), None, 4, 96, None, 10, 10, None) == -1
    torch.cuda.synchronize()
    assert st.tolist() == [0] * 8                                  # a refused call launches nothing
