"""
The diagnostic error counters (ldpc_sim_count_diag) against the numpy restatement of tests/sim_diag_reference.py: the state
and the whole diag buffer, array_equal, on synthetic blocks -- random packed rows with garbage pad bits, random iterations in
0..T, random success flags that have nothing to do with the wrong bits.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_reference as ref
import sim_diag_reference as dref

pytestmark = pytest.mark.gpu

BIG = 10 ** 6
GUARD = 0x5A5A5A5A5A5A5A5A
GUARD_WORDS = 8


def synthetic(rng, B, n, T, p_err, cw):
    """(packed uint8 [B, ceil(n/8)] with garbage pad bits, XORed with the packed codeword; iterations; success)"""
    bits = np.zeros((B, n), dtype=np.uint8)
    for b in np.nonzero(rng.random(B) < p_err)[0]:
        bits[b, rng.choice(n, size=int(rng.integers(1, min(n, 40) + 1)), replace=False)] = 1
        if rng.random() < 0.3:
            bits[b, n - 1] = 1
    pad = (rng.random((B, (-n) % 8)) < 0.5).astype(np.uint8)
    packed = np.packbits(np.concatenate([bits, pad], axis=1), axis=1, bitorder="little")
    if cw is not None:
        packed = packed ^ cw[None, :]
    return packed, rng.integers(0, T + 1, B).astype(np.int32), rng.integers(0, 2, B).astype(np.uint8)


def make_codeword(rng, n, with_codeword):
    if not with_codeword:
        return None
    bits = np.concatenate([(rng.random(n) < 0.5).astype(np.uint8), np.ones((-n) % 8, np.uint8)])   # garbage pad bits too
    return np.packbits(bits, bitorder="little")


class Device:
    """the inputs of one block on the device, and ldpc_sim_count_diag / ldpc_sim_count through the raw entry points"""

    def __init__(self, dev, packed, iters, success, n, cw):
        import _native
        self.nat, self.lib, self.dev, self.n, self.B = _native, _native.load(), dev, n, len(iters)
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.packed, self.iters, self.success, self.cw = up(packed), up(iters), up(success), up(cw)
        self.scratch_bytes = int(self.lib.ldpc_sim_count_diag_scratch_bytes(self.B))
        assert self.scratch_bytes >= 4 * self.B and self.lib.ldpc_sim_count_diag_scratch_bytes(0) == 0

    def diag(self, state, diag, T, capture, first_frame, max_frames, max_errors):
        """-> (state, diag) as lists of python ints; guards round diag and scratch and the spare word are checked"""
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        words = len(diag)
        assert words == self.lib.ldpc_sim_diag_words(T, capture)
        st = torch.tensor(state, dtype=torch.int64, device=self.dev)
        buf = torch.full((words + 2 * GUARD_WORDS,), GUARD, dtype=torch.int64, device=self.dev)
        buf[GUARD_WORDS:GUARD_WORDS + words] = torch.tensor(diag, dtype=torch.int64, device=self.dev)
        dg = buf[GUARD_WORDS:GUARD_WORDS + words]
        sc = torch.full((self.scratch_bytes + 512,), 0xA5, dtype=torch.uint8, device=self.dev)      # dirty scratch
        stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        self.nat.check(self.lib.ldpc_sim_count_diag(p(st), p(dg), T, capture, p(self.packed), p(self.iters), p(self.success),
                                                    self.B, self.n, p(self.cw), first_frame & (2 ** 64 - 1), max_frames,
                                                    max_errors, C.c_void_p(sc.data_ptr() + 256), self.scratch_bytes, stream),
                       "ldpc_sim_count_diag")
        out = buf.tolist()
        assert out[:GUARD_WORDS] == [GUARD] * GUARD_WORDS and out[-GUARD_WORDS:] == [GUARD] * GUARD_WORDS
        assert bool((sc[:256] == 0xA5).all()) and bool((sc[256 + self.scratch_bytes:] == 0xA5).all())
        got = out[GUARD_WORDS:-GUARD_WORDS]
        assert got[2] == 0 and got[3] == 0                                                      # the unordered spare word
        return st.tolist(), got

    def plain(self, state, max_frames, max_errors):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        st = torch.tensor(state, dtype=torch.int64, device=self.dev)
        self.nat.check(self.lib.ldpc_sim_count(p(st), p(self.packed), p(self.iters), self.B, self.n, p(self.cw), max_frames,
                                               max_errors, C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)),
                       "ldpc_sim_count")
        return st.tolist()


def check(d, wrong, iters, success, state, diag, T, capture, first, max_frames, max_errors, note=()):
    want_state, want_diag = dref.sim_fold_diag(state, diag, wrong, iters, success, first, T, capture, max_frames, max_errors)
    got_state, got_diag = d.diag(state, diag, T, capture, first, max_frames, max_errors)
    assert got_state == want_state, (note, T, capture, max_frames, max_errors)
    assert np.array_equal(got_diag, want_diag), (note, T, capture, max_frames, max_errors)
    assert d.plain(state, max_frames, max_errors) == got_state                                # the plain counter agrees
    return got_state, got_diag


@pytest.mark.parametrize("with_codeword", [False, True])
@pytest.mark.parametrize("n", [7, 96])
@pytest.mark.parametrize("B", [1, 64, 65, 1025, 2049])
def test_one_block_against_the_restatement(B, n, with_codeword, gpu_device):
    rng = np.random.default_rng(B * 10007 + n * 3 + with_codeword)
    cw = make_codeword(rng, n, with_codeword)
    for p_err, Ts in ((0.1, (1, 10, 300)), (0.0, (10,)), (1.0, (10,))):
        for T in Ts:
            packed, iters, success = synthetic(rng, B, n, T, p_err, cw)
            wrong = ref.wrong_bits(packed, n, cw)
            n_err = int((wrong > 0).sum())
            d = Device(gpu_device, packed, iters, success, n, cw)
            # no limit in reach; the frame limit mid-block and on the last frame; max_errors = 0; the error limit mid-block,
            # on the last erroneous frame, one past it, and together with a frame limit
            limits = [(BIG, BIG), (max(1, B // 2), BIG), (B, BIG), (BIG, 0)]
            if n_err:
                limits += [(BIG, max(1, n_err // 2)), (BIG, n_err), (BIG, n_err + 1), (max(1, B - 1), n_err)]
            for capture in (0, 1, 5, n_err + 3):
                for max_frames, max_errors in limits:
                    first = int(rng.integers(0, 2 ** 33))
                    check(d, wrong, iters, success, [0] * 8, [0] * dref.diag_words(T, capture), T, capture, first, max_frames,
                          max_errors, (p_err,))


def test_stop_frames_first_last_and_inside_a_later_fold_tile(gpu_device):
    n, B, T = 96, 2049, 10
    rng = np.random.default_rng(5)
    packed, iters, success = synthetic(rng, B, n, T, 0.0, None)
    packed[[0, 1500, B - 1], 11] |= 0x80                               # bit 95 of frames 0, 1500 (second fold tile) and 2048
    success[[0, 1500, B - 1]] = (1, 0, 1)
    wrong = ref.wrong_bits(packed, n)
    assert list(np.nonzero(wrong)[0]) == [0, 1500, B - 1]
    d = Device(gpu_device, packed, iters, success, n, None)
    for max_errors, frames in ((1, 1), (2, 1501), (3, B), (4, B)):
        for capture in (0, 1, 2, 8):
            st, dg = check(d, wrong, iters, success, [0] * 8, [0] * dref.diag_words(T, capture), T, capture, 7, BIG, max_errors)
            assert st[0] == frames and st[4] == int(max_errors <= 3) and dg[1] == min(capture, max_errors, 3)
            assert dg[0] == (1, 1, 2, 2)[max_errors - 1] and sum(dg[4:4 + T + 1]) == frames
    # a state with errors already counted: the limit is reached by this block's second error
    start = [40, 7, 90, 300, 0, 2, 0, 0]
    diag0 = [3, 2, 0, 0] + [4] * (T + 1) + [11, 1, 2, 0, 13, 5, 10, 1] + [0] * 8
    st, dg = check(d, wrong, iters, success, start, diag0, T, 4, 2 ** 40, BIG, 9)
    assert st[0] == 40 + 1501 and st[1] == 9 and dg[1] == 4 and dg[23:27] == [2 ** 40, 1, int(iters[0]), 1]


def test_capture_fills_inside_a_block_before_the_stop_frame(gpu_device):
    n, B, T = 96, 1025, 10
    rng = np.random.default_rng(6)
    packed, iters, success = synthetic(rng, B, n, T, 0.05, None)
    wrong = ref.wrong_bits(packed, n)
    n_err = int((wrong > 0).sum())
    assert n_err > 12
    d = Device(gpu_device, packed, iters, success, n, None)
    for capture in (3, 5):
        for max_errors in (capture + 4, n_err - 1, BIG):
            st, dg = check(d, wrong, iters, success, [0] * 8, [0] * dref.diag_words(T, capture), T, capture, 0, BIG, max_errors)
            assert dg[1] == capture and st[1] == min(max_errors, n_err)
            assert dg[4 + T + 1:4 + T + 1 + 4 * capture:4] == list(np.nonzero(wrong)[0][:capture])


@pytest.mark.parametrize("limits", [(BIG, BIG), (1025 + 64 + 500, BIG), (BIG, None)])
def test_state_and_diag_carried_over_launches(limits, gpu_device):
    """three blocks into one state and one diag buffer, the block_first_frame of each its own (one above 2^32, one that wraps
    past 2^64), then a launch after `done` (nothing but blocks_seen moves) and an empty block"""
    n, T, capture = 96, 10, 6
    rng = np.random.default_rng(16)
    blocks = [synthetic(rng, B, n, T, 0.004, None) for B in (1025, 64, 1025)]
    errs = [int((ref.wrong_bits(b[0], n) > 0).sum()) for b in blocks]
    assert errs[0] < capture < errs[0] + errs[1] + errs[2] - 2 and errs[2] > 2      # the capture fills in the last block
    max_frames, max_errors = limits
    if max_errors is None:
        max_errors = errs[0] + errs[1] + 2
    firsts = (0, 2 ** 32 + 5, 2 ** 64 - 100)
    state, diag = [0] * 8, [0] * dref.diag_words(T, capture)
    for (packed, iters, success), first in zip(blocks, firsts):
        d = Device(gpu_device, packed, iters, success, n, None)
        state, diag = check(d, ref.wrong_bits(packed, n), iters, success, state, diag, T, capture, first, max_frames, max_errors)
    limited = limits != (BIG, BIG)
    assert state[4] == int(limited) and state[5] == 3
    if limited:                                                         # a launch after `done`
        before = (list(state), list(diag))
        state, diag = check(d, ref.wrong_bits(packed, n), iters, success, state, diag, T, capture, 77, max_frames, max_errors)
        assert state[:5] == before[0][:5] and state[5] == 4 and diag == before[1]
    # batch = 0: the flag and blocks_seen are all that can move, NULL block pointers are accepted
    import _native
    lib = _native.load()
    st = torch.tensor(state, dtype=torch.int64, device=gpu_device)
    dg = torch.tensor(diag, dtype=torch.int64, device=gpu_device)
    p = lambda t: C.c_void_p(t.data_ptr())
    for with_diag in (True, False):
        _native.check(lib.ldpc_sim_count_diag(p(st), p(dg) if with_diag else None, T, capture, None, None, None, 0, n, None, 0,
                                              max_frames, max_errors, None, 0, None), "ldpc_sim_count_diag")
        state = ref.sim_fold(state, [], [], max_frames, max_errors)
        assert st.tolist() == state and dg.tolist() == diag


def test_what_the_diagnostic_counter_refuses(gpu_device):
    import _native
    lib = _native.load()
    T, capture, n, B = 10, 2, 96, 4
    assert lib.ldpc_sim_diag_words(T, capture) == 4 + T + 1 + 4 * capture and lib.ldpc_sim_diag_words(0, 0) == 5
    assert lib.ldpc_sim_diag_words(-1, 0) == 0 and lib.ldpc_sim_diag_words(3, -1) == 0
    st = torch.zeros(8, dtype=torch.int64, device=gpu_device)
    dg = torch.zeros(lib.ldpc_sim_diag_words(T, capture) + 1, dtype=torch.int64, device=gpu_device)
    pk = torch.zeros((B, 12), dtype=torch.uint8, device=gpu_device)
    it = torch.ones(B, dtype=torch.int32, device=gpu_device)
    su = torch.ones(B, dtype=torch.uint8, device=gpu_device)
    need = lib.ldpc_sim_count_diag_scratch_bytes(B)
    sc = torch.zeros(need, dtype=torch.uint8, device=gpu_device)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(state=p(st), diag=p(dg), T=T, capture=capture, packed=p(pk), iters=p(it), success=p(su), batch=B, n=n,
             scratch=p(sc), scratch_bytes=need):
        return lib.ldpc_sim_count_diag(state, diag, T, capture, packed, iters, success, batch, n, None, 0, 10, 10, scratch,
                                       scratch_bytes, None)
    assert call(T=-1) == -1 and b"T < 0" in lib.ldpc_last_error()
    assert call(capture=-1) == -1 and b"capture" in lib.ldpc_last_error()
    assert call(batch=-1) == -1 and call(n=0) == -1 and call(state=None) == -1
    assert call(success=None) == -1 and b"NULL" in lib.ldpc_last_error()
    assert call(diag=None) == -1 and call(scratch=None) == -1 and call(packed=None) == -1 and call(iters=None) == -1
    assert call(diag=C.c_void_p(dg.data_ptr() + 4)) == -1 and b"aligned" in lib.ldpc_last_error()
    assert call(scratch_bytes=need - 1) == -4 and b"scratch" in lib.ldpc_last_error()
    torch.cuda.synchronize()
    assert st.tolist() == [0] * 8 and not dg.any()                 # a refused call launches nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert st.tolist()[:2] == [B, 0] and dg.tolist()[4 + 1] == B
