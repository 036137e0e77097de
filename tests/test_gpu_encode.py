"""
GPU tests (-m gpu) of Monte-Carlo on random codewords: ldpc_encode_random / ldpc_encode against the numpy restatement of the
information-bit stream (tests/encode_reference.py) and codes.Encoder.encode, the per-frame channel against single-frame calls
of the one-codeword channel as bit patterns, the counters on codeword rows against the numpy fold, the one-call point
(ldpc_simulate_enc) against the written-out loop on both engines, replay of recorded frames, and the punctured all-zero trap.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import encode_reference as eref
import philox_reference as ref

pytestmark = pytest.mark.gpu

T = 10
SEED, STREAM, FIRST = (0x9E37 << 32) | 0x1234567, 3500, 2 ** 40 + 7
COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done")
GUARD = 0xA5


def encoder_of(kind):
    """the cases: toy matrices (dense rows, scattered positions), the committed staircase codes (16200: more
    information words than lanes, 141 ballot words), a staircase code with m = 129
    (a one-bit last ballot word) and the eliminated form of a staircase code (dense rows, no accumulation)"""
    import codes
    if kind in ("toy", "reversed", "permuted", "deficient"):
        return codes.Encoder.from_graph(eref.toy_graph(kind))
    if kind == "m129":
        return codes.Encoder.from_graph(codes.generate_ira_code(200, 129, {3: 71}, seed=129))
    if kind == "small eliminated":
        return codes.Encoder.from_graph(codes.load_graph("small_96_48"), method="eliminate")
    return codes.Encoder.from_graph(codes.load_graph(kind))


@pytest.mark.parametrize("kind", ["toy", "reversed", "permuted", "deficient", "small_96_48", "small eliminated", "m129",
                                  "ira_1998_1512", "dvbs2_like_16200_7200"])
def test_encode_random_is_the_stream_through_the_host_encoder(kind, gpu_device):
    import engine
    e = encoder_of(kind)
    if kind == "ira_1998_1512":
        assert e.k % 32 == 8 and (e.n - e.k) % 64 != 0 and (e.n + 7) // 8 == 250 and e.accumulate and e.systematic
    if kind == "m129":
        assert e.n - e.k == 129 and e.accumulate
    if kind == "permuted":
        assert not e.systematic
    kw = dict(seed=SEED, stream_id=STREAM, device=gpu_device)
    want_info = eref.info_bits(67, e.k, SEED, STREAM, FIRST)
    want = eref.pack_rows(e.encode(want_info))                       # pad bits of the last byte are 0
    for batch in (1, 5, 67):
        cw, info = engine.encode_random(e, batch, first_frame=FIRST, want_info=True, **kw)
        assert cw.shape == (batch, (e.n + 7) // 8) and info.shape == (batch, (e.k + 7) // 8)
        assert np.array_equal(info.cpu().numpy(), eref.pack_rows(want_info[:batch]))
        assert np.array_equal(cw.cpu().numpy(), want[:batch])
        assert torch.equal(engine.encode_random(e, batch, first_frame=FIRST, **kw), cw)      # without the information rows
    # a frame's codeword does not depend on the block it is drawn in
    parts = [engine.encode_random(e, 30, first_frame=FIRST, **kw), engine.encode_random(e, 37, first_frame=FIRST + 30, **kw)]
    assert np.array_equal(torch.cat(parts).cpu().numpy(), want)
    # ldpc_encode of the given bits; the pad bits of an information row are ignored
    rows = eref.pack_rows(want_info)
    if e.k % 8:
        rows[:, -1] |= np.uint8((0xFF << (e.k % 8)) & 0xFF)
    got = engine.encode(e, torch.from_numpy(rows).to(gpu_device))
    assert np.array_equal(got.cpu().numpy(), want)
    assert engine.encode_random(e, 0, first_frame=FIRST, **kw).shape == (0, (e.n + 7) // 8)


@pytest.mark.parametrize("kind", ["permuted", "small_96_48", "ira_1998_1512"])
def test_encoder_stores_stay_inside_rows_at_every_alignment(kind, gpu_device):
    import _native
    from engine import _NativeEncoder
    e = encoder_of(kind)
    ne = _NativeEncoder.get(e, gpu_device)
    L = _native.load()
    B, nb, kb = 5, (e.n + 7) // 8, (e.k + 7) // 8
    want_info = eref.info_bits(B, e.k, SEED, STREAM, FIRST)
    want = eref.pack_rows(e.encode(want_info))
    for skew in range(4):
        bufs = [torch.full((16 + skew + B * w + 16,), GUARD, dtype=torch.uint8, device=gpu_device) for w in (nb, kb)]
        assert all(b.data_ptr() % 16 == 0 for b in bufs)
        ptrs = [C.c_void_p(b.data_ptr() + 16 + skew) for b in bufs]
        assert L.ldpc_encode_random(ne.handle, B, SEED, STREAM, FIRST, ptrs[0], ptrs[1], None) == 0, L.ldpc_last_error()
        for buf, rows in zip(bufs, (want, eref.pack_rows(want_info))):
            host = buf.cpu().numpy()
            lo, hi = 16 + skew, 16 + skew + rows.size
            assert (host[:lo] == GUARD).all() and (host[hi:] == GUARD).all(), (kind, skew)
            assert np.array_equal(host[lo:hi].reshape(rows.shape), rows), (kind, skew)


@pytest.mark.parametrize("n", [1998, 7])
@pytest.mark.parametrize("profile", [False, True])
def test_channel_with_codeword_rows_equals_single_frame_calls(n, profile, gpu_device):
    import engine
    from rate_matching import RateMatching
    B = 13
    rng = np.random.default_rng(n)
    rows = eref.pack_rows(rng.integers(0, 2, (B, n)))
    rows_dev = torch.from_numpy(rows).to(gpu_device)
    rm = None
    if profile:
        pick = rng.permutation(n)
        rm = RateMatching(n, punctured=np.sort(pick[:max(2, n // 5)]), shortened=np.sort(pick[max(2, n // 5):max(4, n // 3)]),
                          short_llr=18.5)
    kw = dict(seed=SEED, stream_id=STREAM, snr_db=2.5, device=gpu_device, rate_matching=rm)
    got = engine.awgn_llr(B, n, first_frame=FIRST, codeword=rows_dev, **kw)
    one = [engine.awgn_llr(1, n, first_frame=FIRST + b, codeword=rows_dev[b].contiguous(), **kw) for b in range(B)]
    assert torch.equal(got.view(torch.int32), torch.cat(one).view(torch.int32))
    zero = engine.awgn_llr(B, n, first_frame=FIRST, **kw)
    assert not torch.equal(got.view(torch.int32), zero.view(torch.int32))                # the rows are read
    with pytest.raises(ValueError):
        engine.awgn_llr(B + 1, n, first_frame=FIRST, codeword=rows_dev, **kw)


def small_engine(gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code("small_96_48", T)
    dec = BasicMinSumDecoder(code, 0.7)
    return code, dec, _engine_of(dec, gpu_device)


def test_sim_count_with_codeword_rows(gpu_device):
    code, _, eng = small_engine(gpu_device)
    n, B = code.n, 300
    rng = np.random.default_rng(8)
    rows = eref.pack_rows(rng.integers(0, 2, (B, n)))
    flips = (rng.random((B, n)) < 0.004).astype(np.uint8)                                # about a third of the frames in error
    packed = rows ^ eref.pack_rows(flips)
    iters = rng.integers(1, T + 1, B).astype(np.int32)
    wrong = ref.wrong_bits(packed ^ rows, n)
    assert np.array_equal(wrong, flips.sum(axis=1)) and 50 < (wrong > 0).sum() < 250
    pd, idv, rd = (torch.from_numpy(a).to(gpu_device) for a in (packed, iters, rows))
    for max_frames, max_errors in ((10 ** 6, 10 ** 6), (450, 10 ** 6), (10 ** 6, 77)):
        state = torch.zeros(8, dtype=torch.int64, device=gpu_device)
        want = [0] * 8
        for _ in range(2):
            eng.sim_count(state, pd, idv, max_frames=max_frames, max_errors=max_errors, codeword=rd)
            want = ref.sim_fold(want, wrong, iters, max_frames, max_errors)
            assert state.tolist() == want
        assert np.array_equal(pd.cpu().numpy(), packed)                                  # the caller's decisions are untouched
    with pytest.raises(ValueError):
        eng.sim_count(torch.zeros(8, dtype=torch.int64, device=gpu_device), pd, idv, max_frames=9, max_errors=9, codeword=rd[:-1])


def written_out(eng, rm, snr_db, max_frames, max_errors, capture, block):
    """the loop ldpc_simulate_enc runs, one engine call per step -> what DecodeEngine.simulate(diagnostics=True) returns"""
    import engine
    state = torch.zeros(8, dtype=torch.int64, device=eng.device)
    diag = eng.sim_diag_buffer(capture)
    kw = dict(seed=SEED, stream_id=STREAM, device=eng.device)
    for first in range(0, max_frames, block):
        frames = min(block, max_frames - first)
        cw = engine.encode_random(eng.encoder(), frames, first_frame=first, **kw)
        llr = engine.awgn_llr(frames, eng.graph.n, first_frame=first, snr_db=snr_db, codeword=cw, rate_matching=rm, **kw)
        res = eng.decode(llr, early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
        eng.sim_count(state, res.packed_bits, res.iterations, max_frames=max_frames, max_errors=max_errors, codeword=cw,
                      success=res.success, diag=diag, first_frame=first, capture=capture, rate_matching=rm)
    out = dict(zip(engine.SIM_COUNTERS, state.tolist()))
    out.update(engine.parse_sim_diag(diag.cpu().numpy(), T, capture))
    return out


def same_diag(got, want):
    assert {k: got[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}
    assert got["undetected_errors"] == want["undetected_errors"] and got["captured"] == want["captured"]
    assert np.array_equal(got["iteration_histogram"], want["iteration_histogram"])
    assert np.array_equal(got["error_frames"], want["error_frames"])


def point_case(name, gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code(name, T)
    dec = BasicMinSumDecoder(code, 0.7)
    eng = _engine_of(dec, gpu_device)
    mode, snr_db = ("auto", 4.75) if name == "ira_1998_1512" else ("stream", 2.0)
    return code, dec, eng, mode, snr_db


@pytest.mark.parametrize("name", ["ira_1998_1512", "small_96_48"])
def test_one_call_equals_the_written_out_loop(name, gpu_device):
    from rate_matching import RateMatching
    code, dec, eng, mode, snr_db = point_case(name, gpu_device)
    k = code.n - code.tanner_graph().m
    profiles = (None, RateMatching(code.n, punctured=[1, 6, 13], count=np.arange(code.n) < k))
    eng.set_mode(mode)
    try:
        assert eng.info()["engine"] == ("resident" if mode == "auto" else "stream")
        for rm in profiles:
            for max_frames, max_errors in ((900, 10 ** 6), (2000, 25)):
                want = written_out(eng, rm, snr_db, max_frames, max_errors, 6, 333)
                assert want["frame_errors"] >= 25 and want["done"] == 1 and want["captured"] == 6, want
                if max_errors == 25:
                    assert want["frame_errors"] == 25 and want["frames"] < max_frames
                kw = dict(seed=SEED, stream_id=STREAM, snr_db=snr_db, codeword="random", max_frames=max_frames,
                          max_errors=max_errors, rate_matching=rm)
                for block, poll in ((333, 4), (100, 5)):                     # block and poll_blocks change blocks_seen alone
                    same_diag(eng.simulate(diagnostics=True, capture=6, block=block, poll_blocks=poll, **kw), want)
                    got = eng.simulate(block=block, poll_blocks=poll, **kw)
                    assert {c: got[c] for c in COUNTERS} == {c: want[c] for c in COUNTERS}
        with pytest.raises(ValueError):
            eng.simulate(seed=1, snr_db=2.0, max_frames=10, max_errors=10, codeword="zero")
    finally:
        eng.set_mode("auto")


@pytest.mark.parametrize("name", ["ira_1998_1512", "small_96_48"])
def test_simulator_with_random_codewords_and_replay(name, gpu_device, tmp_path):
    from rate_matching import RateMatching
    from simulation_framework import LDPSimulator, SimulationConfig
    code, dec, eng, mode, snr_db = point_case(name, gpu_device)
    k = code.n - code.tanner_graph().m
    rm = RateMatching(code.n, punctured=[1, 6, 13], count=np.arange(code.n) < k)
    eng.set_mode(mode)
    try:
        cfg = SimulationConfig(snr_range=(snr_db, snr_db), snr_step=1.0, seed=SEED, channel="device", codeword="random",
                               results_dir=str(tmp_path), save_results=False, max_frames=1500, max_errors=30, batch_frames=256,
                               rate_matching=rm, capture_errors=100, stage_min_block=64)
        sim = LDPSimulator(cfg)
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="punctured")            # random codewords: the trap is closed, no warning
            with torch.no_grad():
                r = sim.simulate_decoder(dec, code, "d")
        rec = r.error_frames[0]
        assert r.total_errors[0] == 30 == len(rec) and r.total_frames[0] < 1500
        # the driver's point is DecodeEngine.simulate's, whichever engine runs it
        want = eng.simulate(seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, codeword="random", max_frames=1500,
                            max_errors=30, rate_matching=rm, diagnostics=True, capture=100, block=999)
        assert (r.total_frames[0], r.total_errors[0], r.undetected_errors[0]) == (want["frames"], 30, want["undetected_errors"])
        assert np.array_equal(rec, want["error_frames"])
        out = sim.replay_errors(dec, code, snr_db, rec["frame"])
        sent = eref.unpack_rows(out["codewords"].cpu().numpy(), code.n)
        assert sent.any(axis=1).all() and not code.tanner_graph().syndrome(sent).any()
        wrong = ((out["bits"].cpu().numpy() != sent) & rm.count[None, :]).sum(axis=1)
        assert np.array_equal(wrong, rec["wrong_bits"]) and (wrong > 0).all()
        assert np.array_equal(out["iterations"].cpu().numpy(), rec["iterations"])
        assert (out["llr"][:, [1, 6, 13]].view(torch.int32) == 0).all()
    finally:
        eng.set_mode("auto")


@pytest.mark.parametrize("mode", ["auto", "stream"])
def test_every_bit_punctured_counts_the_codeword_weight(mode, gpu_device):
    """the trap, with no tolerance: nothing is sent, every decision is 0 and satisfies H.  Against the all-zero codeword that
    counts as 300 correct frames; against a random codeword every set bit is an error, and an undetected one"""
    import engine
    from rate_matching import RateMatching
    code, _, eng = small_engine(gpu_device)
    rm = RateMatching(code.n, punctured=np.arange(code.n))
    eng.set_mode(mode)
    try:
        assert eng.info()["engine"] == ("resident" if mode == "auto" else "stream")
        kw = dict(seed=SEED, stream_id=STREAM, snr_db=3.0, max_frames=300, max_errors=10 ** 6, rate_matching=rm, diagnostics=True,
                  block=128)
        zero = eng.simulate(**kw)
        assert zero["frames"] == 300 and zero["frame_errors"] == 0 and zero["bit_errors"] == 0
        got = eng.simulate(codeword="random", **kw)
        sent = eref.unpack_rows(engine.encode_random(eng.encoder(), 300, seed=SEED, stream_id=STREAM, device=gpu_device).cpu().numpy(),
                                code.n)
        weight = sent.sum(axis=1)
        assert got["frames"] == 300 and got["frame_errors"] == int((weight > 0).sum()) > 0
        assert got["bit_errors"] == int(weight.sum()) and got["undetected_errors"] == got["frame_errors"]
    finally:
        eng.set_mode("auto")
