"""
GPU tests (-m gpu) of rate matching (ldpc_rate_match of include/ldpc_hip.h): the rate-matched channel
kernels against RateMatching.where / the numpy rule on the plain draw as int32 bit patterns, the masked counters against the
numpy fold of tests/rate_matching_reference.py, the one-call Monte-Carlo against the written-out loop, the simulator on both
engines, the ordering shortened < plain < punctured found with the CPU oracle, and stream training through a profile.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import philox_reference as ref
import rate_matching_reference as rmref
import sim_diag_reference as dref

pytestmark = pytest.mark.gpu

LEAD = 4                                 # guard words before a block: the block itself starts 16-byte aligned at skew 0
GUARD = 0x7FC0DEAD                       # int32 pattern around every output block: a store outside the block changes it
T = 10
COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done")
# small_96_48: eight degree-3 information bits no two of which share a check, and the eight degree-8 information bits
PUNCTURED = [0, 2, 3, 6, 9, 10, 14, 19]
SHORTENED = [1, 4, 5, 21, 26, 30, 32, 33]


def lib():
    import _native
    return _native.load()


def dev_bytes(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)


def pack(mask, garbage=False):
    """bool [n] -> packed bytes; garbage: the pad bits of the last byte set"""
    p = np.packbits(np.asarray(mask, dtype=np.uint8), bitorder="little")
    n = len(mask)
    if garbage and n % 8:
        p[-1] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    return p


class Profile:
    """a raw ldpc_rate_match over masks given as bool [n] (or None = NULL pointer); keeps its device buffers alive"""

    def __init__(self, dev, punctured=None, shortened=None, count=None, short_llr=0.0, garbage=False, null=False):
        import _native
        self.punctured, self.shortened, self.count, self.short_llr, self.null = punctured, shortened, count, short_llr, null
        self.bufs = [None if m is None else dev_bytes(pack(m, garbage), dev) for m in (punctured, shortened, count)]
        ptr = lambda t: None if t is None else t.data_ptr()
        self.struct = _native.RateMatch(punctured_packed=ptr(self.bufs[0]), shortened_packed=ptr(self.bufs[1]),
                                        count_packed=ptr(self.bufs[2]), short_llr=float(short_llr))

    @property
    def arg(self):
        return None if self.null else C.byref(self.struct)

    def expect(self, plain, codeword):
        """the channel rule on the plain draw (numpy float32 [B, n]); a bit in both masks is shortened"""
        if self.null:
            return plain
        p = self.punctured
        if p is not None and self.shortened is not None:
            p = p & ~self.shortened
        return rmref.apply(plain, p, self.shortened, self.short_llr, codeword)


def channel_profiles(n, dev, rng):
    Q = (n + 3) // 4
    j = np.arange(n)
    quads = np.where((j // 4) % 2 == 0, True, j % 4 == 1)               # whole quads off next to partly transmitted ones
    tail = j >= 4 * (Q - 1)
    r = rng.integers(0, 3, n)
    out = {
        "rm NULL": Profile(dev, null=True),
        "all masks NULL": Profile(dev),
        "all punctured": Profile(dev, punctured=np.ones(n, bool)),
        "all shortened": Profile(dev, shortened=np.ones(n, bool), short_llr=17.5),
        "whole and partial quads": Profile(dev, punctured=quads & (j % 3 != 0), shortened=quads & (j % 3 == 0), short_llr=9.0),
        "tail quad punctured": Profile(dev, punctured=tail),
        "tail quad shortened": Profile(dev, shortened=tail, short_llr=30.0),
        "random": Profile(dev, punctured=r == 1, shortened=r == 2, short_llr=12.25),
        "pad garbage": Profile(dev, punctured=r == 1, shortened=r == 2, short_llr=12.25, garbage=True),
        "bit in both": Profile(dev, punctured=r >= 1, shortened=r == 2, short_llr=8.0),
    }
    return out


def draw(dev, batch, n, cw_dev, profile, skew, *, mix=None, plain=False, seed=77, stream_id=5, first_frame=123456789012):
    """the block through ldpc_channel_awgn[_mix][_rm] into a guarded buffer, the base pointer `skew` elements past a
    16-byte boundary -> int32 [batch, n]"""
    L = lib()
    lead = LEAD + skew
    buf = torch.full((lead + batch * n + 1,), GUARD, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 16 == 0
    ptr = C.c_void_p(buf.data_ptr() + 4 * lead)
    cw = None if cw_dev is None else C.c_void_p(cw_dev.data_ptr())
    if mix is None:
        args = (ptr, batch, n, seed, stream_id, first_frame, 2.5, 3.125, cw)
        rc = L.ldpc_channel_awgn(*args, None) if plain else L.ldpc_channel_awgn_rm(*args, profile.arg, None)
    else:
        args = (ptr, batch, n, seed, stream_id, first_frame, C.c_void_p(mix[0].data_ptr()), C.c_void_p(mix[1].data_ptr()),
                mix[0].numel(), cw)
        rc = L.ldpc_channel_awgn_mix(*args, None) if plain else L.ldpc_channel_awgn_mix_rm(*args, profile.arg, None)
    assert rc == 0, L.ldpc_last_error()
    host = buf.cpu().numpy()
    assert (host[:lead] == GUARD).all() and host[-1] == GUARD, "a store outside the block"
    return host[lead:lead + batch * n].reshape(batch, n)


# ---------------------------------------------------------------------------------------------------- 1. channel
# batches that cross a workgroup boundary of 256 quads, mid-row where a row has more than one quad
SHAPES = [(1, 300), (3, 259), (4, 300), (5, 131), (7, 150), (8, 130), (9, 90), (13, 70), (96, 23), (1998, 3)]


@pytest.mark.parametrize("n,batch", SHAPES)
def test_channel(n, batch, gpu_device):
    assert batch * ((n + 3) // 4) > 256
    rng = np.random.default_rng(n)
    codeword = rng.integers(0, 2, n)
    profiles = channel_profiles(n, gpu_device, rng)
    tabs = {1: ([2.5], [3.125]), 3: ([2.5, 1.75, 4.0], [3.125, 1.5, 8.0])}
    mixes = {None: None}
    for K, (a, b) in tabs.items():
        mixes[K] = (torch.tensor(a, dtype=torch.float32, device=gpu_device), torch.tensor(b, dtype=torch.float32, device=gpu_device))
    for cw in (None, codeword):
        cw_dev = dev_bytes(None if cw is None else pack(cw), gpu_device)
        for K, mix in mixes.items():
            plain = draw(gpu_device, batch, n, cw_dev, None, 0, mix=mix, plain=True)
            plain_f = plain.view(np.float32)
            assert np.isfinite(plain_f).all() and (plain != GUARD).all()
            if K == 1:                                                   # one point is the plain channel, bit for bit
                assert np.array_equal(plain, draw(gpu_device, batch, n, cw_dev, None, 0, plain=True))
            for name, prof in profiles.items():
                want = prof.expect(plain_f, cw).view(np.int32)
                for skew in (0, 1, 2):                                   # 16-, 4- and 8-byte aligned base pointers
                    got = draw(gpu_device, batch, n, cw_dev, prof, skew, mix=mix)
                    assert np.array_equal(got, want), (name, K, skew, cw is not None)
    # what the profiles are: a punctured bit is +0.0 (int32 0) under a codeword bit of one, too
    got = draw(gpu_device, batch, n, dev_bytes(pack(np.ones(n, int)), gpu_device), profiles["all punctured"], 0)
    assert not got.any()
    got = draw(gpu_device, batch, n, dev_bytes(pack(codeword), gpu_device), profiles["all shortened"], 0).view(np.float32)
    assert np.array_equal(got, np.broadcast_to(np.float32(17.5) * (1 - 2 * codeword), (batch, n)).astype(np.float32))


def test_channel_through_the_engine_functions(gpu_device):
    import engine
    from rate_matching import RateMatching
    n, B = 1998, 5
    rng = np.random.default_rng(3)
    sel = rng.permutation(n)
    c = rng.integers(0, 2, n)
    rm = RateMatching(n, punctured=sel[:200], shortened=sel[200:260], short_llr=25.0)
    kw = dict(seed=4, stream_id=2, first_frame=2 ** 40 + 7, codeword=c, device=gpu_device)
    plain = engine.awgn_llr(B, n, snr_db=2.0, **kw)
    got = engine.awgn_llr(B, n, snr_db=2.0, rate_matching=rm, **kw)
    assert torch.equal(got.view(torch.int32), rm.where(plain, c).view(torch.int32))
    assert torch.equal(engine.awgn_llr(B, n, snr_db=2.0, rate_matching=None, **kw).view(torch.int32), plain.view(torch.int32))
    grid = [1.0, 2.0, 3.5]
    plain = engine.awgn_llr_mix(B, n, snr_db=grid, **kw)
    got = engine.awgn_llr_mix(B, n, snr_db=grid, rate_matching=rm, **kw)
    assert torch.equal(got.view(torch.int32), rm.where(plain, c).view(torch.int32))
    assert (got[:, torch.from_numpy(sel[:200]).to(gpu_device)].view(torch.int32) == 0).all()
    # expand of the transmitted columns is the same block
    tx = plain[:, torch.from_numpy(rm.transmitted).to(gpu_device)]
    assert torch.equal(rm.expand(tx, c).view(torch.int32), got.view(torch.int32))
    with pytest.raises(ValueError, match="RateMatching"):
        engine.awgn_llr(B, n, snr_db=2.0, rate_matching=RateMatching(n + 1), **kw)
    bad = Profile(gpu_device, shortened=np.ones(8, bool), short_llr=0.0)
    out = torch.zeros(8, dtype=torch.float32, device=gpu_device)
    assert lib().ldpc_channel_awgn_rm(C.c_void_p(out.data_ptr()), 1, 8, 0, 0, 0, 1.0, 1.0, None, bad.arg, None) == -1
    assert b"short_llr" in lib().ldpc_last_error() and not out.any().item()


# ---------------------------------------------------------------------------------------------------- 2. counters
def count_block(dev, state, diag, packed, iters, success, n, cw, prof, first_frame, capture, max_frames, max_errors, plain=False):
    """one block through ldpc_sim_count[_rm] (diag None) or ldpc_sim_count_diag[_rm]; state / diag: device tensors, updated"""
    L = lib()
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    B = packed.shape[0]
    pk, it, su = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (packed, iters.astype(np.int32), success.astype(np.uint8)))
    cwd = dev_bytes(cw, dev)
    if diag is None:
        args = (p(state), p(pk), p(it), B, n, p(cwd), max_frames, max_errors)
        rc = L.ldpc_sim_count(*args, None) if plain else L.ldpc_sim_count_rm(*args, prof.arg, None)
    else:
        scratch = torch.empty(max(int(L.ldpc_sim_count_diag_scratch_bytes(B)), 4), dtype=torch.uint8, device=dev)
        args = (p(state), p(diag), T, capture, p(pk), p(it), p(su), B, n, p(cwd), first_frame, max_frames, max_errors,
                p(scratch), scratch.numel())
        rc = L.ldpc_sim_count_diag(*args, None) if plain else L.ldpc_sim_count_diag_rm(*args, prof.arg, None)
    assert rc == 0, L.ldpc_last_error()
    torch.cuda.synchronize(dev)


def crafted_blocks(n, B, kind, rng, count):
    """two blocks of B frames: (packed [B, rb] with garbage in the pad bits, iterations, success), and the codeword's bytes"""
    rb = (n + 7) // 8
    cw = rng.integers(0, 2, n)
    blocks = []
    for _ in range(2):
        err = np.zeros((B, n), dtype=np.uint8)
        rows = rng.random(B) < 0.2
        inside = rng.random((B, n)) < 0.3
        if kind == "outside":
            err[rows] = (inside & ~count[None, :])[rows]
        elif kind == "inside":
            err[rows] = (inside & count[None, :])[rows]
        else:                                                            # rows with errors outside only, inside only, or both
            where = rng.integers(0, 3, B)
            err[rows] = (inside & np.where(where[:, None] == 0, ~count[None, :], np.where(where[:, None] == 1, count[None, :], True)))[rows]
        bits = err ^ cw[None, :].astype(np.uint8)
        packed = np.packbits(bits, axis=1, bitorder="little")
        if n % 8:
            packed[:, -1] |= (rng.integers(0, 256, B).astype(np.uint8) << (n % 8)).astype(np.uint8)
        assert packed.shape == (B, rb)
        blocks.append((packed, rng.integers(1, T + 1, B), (rng.random(B) < 0.5).astype(np.uint8)))
    return blocks, pack(cw)


@pytest.mark.parametrize("n", [13, 96])
@pytest.mark.parametrize("kind", ["outside", "inside", "mixed"])
def test_counters(n, kind, gpu_device):
    rng = np.random.default_rng(100 + n)
    B, capture = 2500, 6                                                 # more than two 1024-frame steps of the fold
    count = rng.random(n) < 0.5
    count[:2] = [True, False]
    prof = Profile(gpu_device, count=count, garbage=True)
    count_packed = pack(count, garbage=True)
    blocks, cw = crafted_blocks(n, B, kind, rng, count)
    wrong = [rmref.wrong_bits(b[0], n, cw, count_packed) for b in blocks]
    all_wrong = [ref.wrong_bits(b[0], n, cw) for b in blocks]
    if kind == "outside":
        assert not wrong[0].any() and all_wrong[0].any()
    else:
        assert wrong[0].any() and (kind == "inside") == bool(np.array_equal(wrong[0], all_wrong[0]))
    errs0 = int((wrong[0] > 0).sum())
    # no limit inside the blocks; the error limit inside the first block (mid-tile) and inside the second; the frame limit
    limits = [(10 ** 6, 10 ** 6), (10 ** 6, max(errs0 // 2, 1)), (10 ** 6, errs0 + 3), (B + 1100, 10 ** 6), (1500, 10 ** 6)]
    for max_frames, max_errors in limits:
        state = torch.zeros(8, dtype=torch.int64, device=gpu_device)
        dstate = torch.zeros(8, dtype=torch.int64, device=gpu_device)
        diag = torch.zeros(dref.diag_words(T, capture), dtype=torch.int64, device=gpu_device)
        want, dwant = [0] * 8, [0] * dref.diag_words(T, capture)
        for k, (packed, iters, success) in enumerate(blocks):
            first = 1000 + k * B
            count_block(gpu_device, state, None, packed, iters, success, n, cw, prof, first, capture, max_frames, max_errors)
            count_block(gpu_device, dstate, diag, packed, iters, success, n, cw, prof, first, capture, max_frames, max_errors)
            prev = want
            want = rmref.sim_fold(prev, packed, iters, n, max_frames, max_errors, cw, count_packed)
            w2, dwant = rmref.sim_fold_diag(prev, dwant, packed, iters, success, first, n, T, capture, max_frames, max_errors,
                                            cw, count_packed)
            assert w2 == want
            assert state.tolist() == want, (max_frames, max_errors, k)
            assert dstate.tolist() == want and diag.tolist() == dwant, (max_frames, max_errors, k)
        if kind != "outside" and max_errors < 10 ** 6:
            assert want[1] == max_errors and want[4] == 1                # the stop rule did hit
    # without a count mask the _rm calls give the plain counters' words exactly
    for prof0 in (Profile(gpu_device, null=True), Profile(gpu_device), Profile(gpu_device, punctured=count, shortened=~count, short_llr=5.0)):
        for max_frames, max_errors in limits[:3]:
            pair = []
            for plain in (True, False):
                state = torch.zeros(8, dtype=torch.int64, device=gpu_device)
                dstate = torch.zeros(8, dtype=torch.int64, device=gpu_device)
                diag = torch.zeros(dref.diag_words(T, capture), dtype=torch.int64, device=gpu_device)
                for k, (packed, iters, success) in enumerate(blocks):
                    count_block(gpu_device, state, None, packed, iters, success, n, cw, prof0, k * B, capture, max_frames, max_errors, plain)
                    count_block(gpu_device, dstate, diag, packed, iters, success, n, cw, prof0, k * B, capture, max_frames, max_errors, plain)
                pair.append((state.tolist(), dstate.tolist(), diag.tolist()))
            assert pair[0] == pair[1] and pair[0][0] == pair[0][1]


# ---------------------------------------------------------------------------------------------------- 3. one call
def small_code():
    import codes
    code = codes.load_code("small_96_48", T)
    g = code.tanner_graph()
    c = codes.staircase_encode(g, np.random.default_rng(22).integers(0, 2, g.n - g.m))
    assert c.any() and not g.syndrome(c).any()
    return code, g, c.astype(np.int64)


def no_check_sees_two(g, punctured):
    mask = np.zeros(g.n, dtype=np.int64)
    mask[punctured] = 1
    return int(np.add.reduceat(mask[g.var_idx], g.check_ptr[:-1]).max()) <= 1


def written_out(eng, rm, c, snr_db, seed, max_frames, max_errors, capture, block):
    """the loop ldpc_simulate_rm runs, one engine call per step -> what DecodeEngine.simulate(diagnostics=True) returns"""
    import engine
    state = torch.zeros(8, dtype=torch.int64, device=eng.device)
    diag = eng.sim_diag_buffer(capture)
    for first in range(0, max_frames, block):
        frames = min(block, max_frames - first)
        llr = engine.awgn_llr(frames, eng.graph.n, seed=seed, stream_id=int(round(snr_db * 1000)), first_frame=first, snr_db=snr_db,
                              codeword=c, device=eng.device, rate_matching=rm)
        res = eng.decode(llr, early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
        eng.sim_count(state, res.packed_bits, res.iterations, max_frames=max_frames, max_errors=max_errors, codeword=c,
                      success=res.success, diag=diag, first_frame=first, capture=capture, rate_matching=rm)
    out = dict(zip(engine.SIM_COUNTERS, state.tolist()))
    out.update(engine.parse_sim_diag(diag.cpu().numpy(), T, capture))
    return out


def same_diag(got, want):
    assert {k: got[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}
    assert got["undetected_errors"] == want["undetected_errors"] and got["captured"] == want["captured"]
    assert np.array_equal(got["iteration_histogram"], want["iteration_histogram"])
    assert np.array_equal(got["error_frames"], want["error_frames"])


@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_one_call_equals_the_written_out_loop(mode, gpu_device):
    import _native
    from ldpc_decoder import BasicMinSumDecoder
    from rate_matching import RateMatching
    from simulation_framework import _engine_of
    code, g, c = small_code()
    assert no_check_sees_two(g, PUNCTURED)
    rm = RateMatching(g.n, punctured=PUNCTURED, shortened=SHORTENED[:3], count=np.arange(g.n) < g.n - g.m, short_llr=20.0)
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), gpu_device)
    eng.set_mode(mode)
    try:
        assert eng.info()["engine"] == ("resident" if mode == "auto" else "stream")
        snr_db, seed = 2.0, 22
        for max_frames, max_errors in ((1500, 10 ** 6), (3000, 150)):
            kw = dict(seed=seed, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, codeword=c, max_frames=max_frames,
                      max_errors=max_errors)
            want = written_out(eng, rm, c, snr_db, seed, max_frames, max_errors, 7, 400)
            assert want["frame_errors"] >= 100 and want["done"] == 1 and want["captured"] == 7
            if max_errors == 150:
                assert want["frame_errors"] == 150 and want["frames"] < max_frames
            plain = eng.simulate(rate_matching=rm, **kw)
            assert {k: plain[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}
            for block, poll in ((400, 4), (64, 1), (257, 3), (4096, 2)):     # block and poll_blocks change blocks_seen alone
                same_diag(eng.simulate(rate_matching=rm, diagnostics=True, capture=7, block=block, poll_blocks=poll, **kw), want)
                got = eng.simulate(rate_matching=rm, block=block, poll_blocks=poll, **kw)
                assert {k: got[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}
            # the profile matters: the plain point counts differently
            assert {k: eng.simulate(**kw)[k] for k in COUNTERS} != {k: want[k] for k in COUNTERS}
        # rm == NULL through the native _rm calls is ldpc_simulate / ldpc_simulate_diag exactly, blocks_seen included
        L = lib()
        cw = torch.from_numpy(pack(c)).to(gpu_device)
        desc = _native.SimDesc(seed=seed, stream_id=2000, first_frame=5, scale=2.5, shift=3.125, codeword_packed=cw.data_ptr(),
                               max_frames=2000, max_errors=120, block=300, poll_blocks=2)
        need = int(L.ldpc_simulate_diag_workspace_bytes(eng.handle, 300, 4))
        ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
        wp = C.c_void_p(ws.data_ptr())
        outs = [np.zeros(8, dtype=np.int64) for _ in range(4)]
        words = [np.zeros(int(L.ldpc_sim_diag_words(T, 4)), dtype=np.int64) for _ in range(2)]
        assert L.ldpc_simulate(eng.handle, C.byref(desc), _native.ptr(outs[0]), wp, need, None) == 0
        assert L.ldpc_simulate_rm(eng.handle, C.byref(desc), None, _native.ptr(outs[1]), wp, need, None) == 0
        assert L.ldpc_simulate_diag(eng.handle, C.byref(desc), 4, _native.ptr(outs[2]), _native.ptr(words[0]), wp, need, None) == 0
        assert L.ldpc_simulate_diag_rm(eng.handle, C.byref(desc), None, 4, _native.ptr(outs[3]), _native.ptr(words[1]), wp, need, None) == 0
        assert outs[0][1] >= 20 and np.array_equal(outs[0], outs[1]) and np.array_equal(outs[2], outs[3])
        assert np.array_equal(words[0], words[1]) and np.array_equal(outs[0][:5], outs[2][:5])
        bad = Profile(gpu_device, shortened=np.ones(g.n, bool), short_llr=float("inf"))
        assert L.ldpc_simulate_rm(eng.handle, C.byref(desc), bad.arg, _native.ptr(outs[1]), wp, need, None) == -1
        assert b"short_llr" in L.ldpc_last_error()
    finally:
        eng.set_mode("auto")


# ---------------------------------------------------------------------------------------------------- 4. simulator
def run_simulator(dec, code, snr_db, tmp_path, **kw):
    from simulation_framework import LDPSimulator, SimulationConfig
    cfg = SimulationConfig(snr_range=(snr_db, snr_db), snr_step=1.0, seed=22, channel="device", results_dir=str(tmp_path),
                           save_results=False, **kw)
    sim = LDPSimulator(cfg)
    with torch.no_grad():
        r = sim.simulate_decoder(dec, code, "d")
    return sim, r


def test_simulator_on_both_engines_and_replay(gpu_device, tmp_path):
    from ldpc_decoder import BasicMinSumDecoder
    from rate_matching import RateMatching
    from simulation_framework import _engine_of
    code, g, c = small_code()
    k = g.n - g.m
    rm = RateMatching(g.n, punctured=PUNCTURED, shortened=SHORTENED[:3], count=np.arange(g.n) < k, short_llr=20.0)
    dec = BasicMinSumDecoder(code, 0.7)
    eng = _engine_of(dec, gpu_device)
    kw = dict(max_frames=2500, max_errors=200, batch_frames=300, rate_matching=rm, codeword=c, capture_errors=10 ** 4,
              stage_min_block=64)
    results = {}
    try:
        for mode in ("auto", "stream"):
            eng.set_mode(mode)
            assert eng.info()["engine"] == ("resident" if mode == "auto" else "stream")
            with warnings.catch_warnings():
                warnings.filterwarnings("error", message="punctured")    # a codeword is given: no warning
                sim, r = run_simulator(dec, code, 2.0, tmp_path, **kw)
            results[mode] = r
            rec = r.error_frames[0]
            assert r.total_errors[0] == 200 == len(rec) and r.total_frames[0] < 2500
            assert r.bit_error_rates[0] == rec["wrong_bits"].sum() / (r.total_frames[0] * k)     # per counted bit
            out = sim.replay_errors(dec, code, 2.0, rec["frame"])
            llr = out["llr"]
            assert (llr[:, PUNCTURED].view(torch.int32) == 0).all()
            assert torch.equal(llr[:, SHORTENED[:3]], torch.tensor(20.0 * (1 - 2 * c[SHORTENED[:3]]), dtype=torch.float32,
                                                                  device=llr.device).expand(len(rec), 3))
            wrong = ((out["bits"].cpu().numpy() != c[None, :]) & rm.count[None, :]).sum(axis=1)
            assert np.array_equal(wrong, rec["wrong_bits"]) and (wrong > 0).all()
            assert np.array_equal(out["iterations"].cpu().numpy(), rec["iterations"])
            assert np.array_equal(out["success"].cpu().numpy().astype(np.int64), rec["undetected"])
    finally:
        eng.set_mode("auto")
    a, b = results["auto"], results["stream"]
    for key in ("total_frames", "total_errors", "frame_error_rates", "bit_error_rates", "average_iterations", "undetected_errors",
                "iteration_histograms"):
        assert getattr(a, key) == getattr(b, key), key
    assert np.array_equal(a.error_frames[0], b.error_frames[0])


def test_the_all_zero_codeword_warning(gpu_device, tmp_path):
    from ldpc_decoder import BasicMinSumDecoder
    from rate_matching import RateMatching
    from simulation_framework import LDPSimulator, SimulationConfig
    code, g, c = small_code()
    dec = BasicMinSumDecoder(code, 0.7)
    kw = dict(max_frames=64, max_errors=10, batch_frames=64)
    with pytest.warns(UserWarning, match="punctured") as caught:
        cfg = SimulationConfig(snr_range=(2.0, 3.0), snr_step=1.0, channel="device", results_dir=str(tmp_path), save_results=False,
                               rate_matching=RateMatching(g.n, punctured=PUNCTURED), **kw)
        with torch.no_grad():
            LDPSimulator(cfg).simulate_decoder(dec, code, "d")
    assert len([w for w in caught if "punctured" in str(w.message)]) == 1            # once per run, not once per point
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="punctured")
        run_simulator(dec, code, 2.0, tmp_path, rate_matching=RateMatching(g.n, punctured=PUNCTURED), codeword=c, **kw)
        run_simulator(dec, code, 2.0, tmp_path, rate_matching=RateMatching(g.n, shortened=SHORTENED, short_llr=20.0), **kw)
        run_simulator(dec, code, 2.0, tmp_path, **kw)


# ---------------------------------------------------------------------------------------------------- 5. behaviour
# Found on the CPU: oracle/ (basic_minsum, factor 0.7, T = 10, float32) on rate_matching_reference.plain_llr + apply, seed 22,
# stream 2000, 2.0 dB, frames 0 .. 1999, the staircase_encode'd codeword of default_rng(22): frame errors over all n bits
ORACLE_FRAME_ERRORS = {"shortened": 539, "plain": 665, "punctured": 1093}


def test_shortening_helps_and_puncturing_hurts(gpu_device):
    import engine
    from ldpc_decoder import BasicMinSumDecoder
    from rate_matching import RateMatching
    from simulation_framework import _engine_of
    code, g, c = small_code()
    k = g.n - g.m
    assert all(g.dv[j] == 3 and j < k for j in PUNCTURED) and no_check_sees_two(g, PUNCTURED) and len(PUNCTURED) == 8
    assert all(j < k for j in SHORTENED) and len(SHORTENED) == 8
    o = ORACLE_FRAME_ERRORS
    assert o["shortened"] < o["plain"] < o["punctured"]
    profiles = {"shortened": RateMatching(g.n, shortened=SHORTENED, short_llr=20.0), "plain": None,
                "punctured": RateMatching(g.n, punctured=PUNCTURED)}
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), gpu_device)
    frames, snr_db = 2000, 2.0
    got = {}
    for name, rm in profiles.items():
        kw = dict(seed=22, stream_id=2000, snr_db=snr_db, codeword=c, rate_matching=rm)
        res = eng.simulate(max_frames=frames, max_errors=10 ** 6, block=512, **kw)
        # the counters are the restated fold of the GPU's own decisions on the GPU's own draw
        llr = engine.awgn_llr(frames, g.n, device=gpu_device, **kw)
        dec = eng.decode(llr, early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
        want = rmref.sim_fold([0] * 8, dec.packed_bits.cpu().numpy(), dec.iterations.cpu().numpy(), g.n, frames, 10 ** 6, pack(c),
                              None if rm is None else rm.packed("cpu")[2])
        assert [res[k_] for k_ in COUNTERS] == want[:5]
        got[name] = res["frame_errors"]
    print("frame errors, GPU:", got, "oracle:", o)
    assert got["shortened"] < got["plain"] < got["punctured"]


# ---------------------------------------------------------------------------------------------------- 6. training
def trainer_with(rm, **kw):
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    from training_framework import PosteriorJointTrainer, TrainingConfig
    code = codes.load_code("small_96_48", max_iterations=5)
    model = Neural2DMinSumDecoder(code, 2, 5)
    with torch.no_grad():
        for p in model.parameters():
            p.fill_(0.3)
    base = dict(batch_size=64, num_epochs=2, learning_rate=0.05, snr_range=(1.0, 4.0), snr_step=0.5, device="cuda", seed=9)
    base.update(kw)
    cfg = TrainingConfig(**base)
    trainer = PosteriorJointTrainer(model, cfg) if rm is None else PosteriorJointTrainer(model, cfg, rate_matching=rm)
    return code, model, trainer


def test_train_stream_draws_through_the_profile(gpu_device):
    import engine
    from rate_matching import RateMatching
    rm = RateMatching(96, punctured=PUNCTURED, shortened=SHORTENED[:4], short_llr=20.0)
    fed = []
    runs = {}
    for name, profile in (("rm", rm), ("rm again", rm), ("none", None)):
        code, model, trainer = trainer_with(profile)
        hook = model.register_forward_pre_hook(lambda mod, args: fed.append(args[0].detach().clone())) if name == "rm" else None
        runs[name] = trainer.train_stream(code, 3, val_frames=70)
        if hook is not None:
            hook.remove()
    grid = engine.snr_grid((1.0, 4.0), 0.5)
    # per epoch: three training steps, then the validation blocks of 64 and 6 frames of stream 1
    assert len(fed) == 2 * (3 + 2)
    for epoch in range(2):
        for s in range(3):
            step = epoch * 3 + s
            want = engine.awgn_llr_mix(64, 96, seed=9, stream_id=0, first_frame=step * 64, snr_db=grid, device=gpu_device,
                                       rate_matching=rm)
            assert torch.equal(fed[epoch * 5 + s].view(torch.int32), want.view(torch.int32))
            assert (want[:, PUNCTURED].view(torch.int32) == 0).all() and (want[:, SHORTENED[:4]] == 20.0).all()
        for v, (first, frames) in enumerate(((0, 64), (64, 6))):
            want = engine.awgn_llr_mix(frames, 96, seed=9, stream_id=1, first_frame=first, snr_db=grid, device=gpu_device,
                                       rate_matching=rm)
            assert torch.equal(fed[epoch * 5 + 3 + v].view(torch.int32), want.view(torch.int32))
    assert runs["rm"] == runs["rm again"]
    assert runs["rm"]["train_losses"] != runs["none"]["train_losses"] and runs["rm"]["val_losses"] != runs["none"]["val_losses"]
    # `train` does not look at the profile
    hist = []
    for profile in (rm, None):
        torch.manual_seed(5)
        code, model, trainer = trainer_with(profile, num_epochs=1)
        hist.append(trainer.train(code, 128, 64))
    assert hist[0] == hist[1]
    with pytest.raises(ValueError, match="RateMatching"):
        trainer_with(np.zeros(96, bool))
