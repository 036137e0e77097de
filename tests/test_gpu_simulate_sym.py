"""
GPU tests (-m gpu) of one SNR point on the symbol channel: the one-call point (ldpc_simulate_sym) against the same loop written
out in Python from encode_random, sym_llr, decode and sim_count, its independence of block and poll_blocks, LDPSimulator with a
modulation on both engines, replay of recorded frames, and the refusals.
"""
import numpy as np
import pytest
import torch

import encode_reference as eref

pytestmark = pytest.mark.gpu

T = 10
SEED, STREAM = (0x9E37 << 32) | 0x1234567, 3500
COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done")
FRAMES = 4096
# Es/N0 per (code, scheme, fading) at which the written-out loop counts between 10 and 200 frame errors in 4096 frames
# (BasicMinSum 0.7, T = 10, random codewords); the counts are in the docstring of test_one_call_equals_the_written_out_loop
SNR_DB = {
    ("small_96_48", "qpsk", None): 4.0,
    ("small_96_48", "qam16", None): 9.5,
    ("small_96_48", "qam16", "rayleigh"): 14.0,
    ("ira_1998_1512", "qpsk", None): 5.5,
    ("ira_1998_1512", "qam16", None): 11.5,
    ("ira_1998_1512", "qam16", "rayleigh"): 17.0,
}


def written_out(eng, mod, snr_db, max_frames, max_errors, capture, block):
    """the loop ldpc_simulate_sym runs, one engine call per step -> what DecodeEngine.simulate(diagnostics=True) returns"""
    import engine
    state = torch.zeros(8, dtype=torch.int64, device=eng.device)
    diag = eng.sim_diag_buffer(capture)
    kw = dict(seed=SEED, stream_id=STREAM, device=eng.device)
    for first in range(0, max_frames, block):
        frames = min(block, max_frames - first)
        cw = engine.encode_random(eng.encoder(), frames, first_frame=first, **kw)
        llr = engine.sym_llr(frames, eng.graph.n, first_frame=first, modulation=mod, snr_db=snr_db, codeword=cw, **kw)
        res = eng.decode(llr, early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
        eng.sim_count(state, res.packed_bits, res.iterations, max_frames=max_frames, max_errors=max_errors, codeword=cw,
                      success=res.success, diag=diag, first_frame=first, capture=capture)
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
    return code, dec, eng, "auto" if name == "ira_1998_1512" else "stream"


@pytest.mark.parametrize("scheme,fading", [("qam16", None), ("qam16", "rayleigh"), ("qpsk", None)])
@pytest.mark.parametrize("name", ["small_96_48", "ira_1998_1512"])
def test_one_call_equals_the_written_out_loop(name, scheme, fading, gpu_device):
    """All eight state words but blocks_seen, and the whole diag buffer, of the native point equal the written-out loop's.
    Frame errors of the written-out loop in 4096 frames at SNR_DB (a condition on the inputs, asserted below):
    small_96_48: 16-QAM 9.5 dB 76, 16-QAM Rayleigh 14.0 dB 73, QPSK 4.0 dB 66;
    ira_1998_1512: 16-QAM 11.5 dB 71, 16-QAM Rayleigh 17.0 dB 37, QPSK 5.5 dB 39."""
    from modulation import Modulation
    code, dec, eng, mode = point_case(name, gpu_device)
    # the QPSK points run through a random interleaver (no fading: the law of the point is the identity run's)
    pos = np.random.default_rng(code.n).permutation(code.n) if scheme == "qpsk" else None
    mod, snr_db = Modulation(scheme, fading, pos), SNR_DB[(name, scheme, fading)]
    eng.set_mode(mode)
    try:
        assert eng.info()["engine"] == ("resident" if mode == "auto" else "stream")
        want = written_out(eng, mod, snr_db, FRAMES, 10 ** 6, 8, FRAMES)
        print(f"{name} {scheme} {fading} at {snr_db} dB: {want['frame_errors']} frame errors in {want['frames']} frames")
        assert want["frames"] == FRAMES and 10 <= want["frame_errors"] <= 200 and want["done"] == 1 and want["captured"] == 8
        kw = dict(seed=SEED, stream_id=STREAM, snr_db=snr_db, codeword="random", modulation=mod, max_frames=FRAMES)
        got = eng.simulate(diagnostics=True, capture=8, max_errors=10 ** 6, block=FRAMES, poll_blocks=1, **kw)
        same_diag(got, want)
        assert got["blocks_seen"] == want["blocks_seen"] == 1
        assert got["detected_errors"] == got["frame_errors"] - got["undetected_errors"]
        # a point that stops on its error limit, cut into blocks in three ways
        stop = written_out(eng, mod, snr_db, FRAMES, 9, 4, 333)
        assert stop["frame_errors"] == 9 and stop["frames"] < FRAMES
        for block, poll in ((1, 64), (100, 5), (4096, 1)):          # block and poll_blocks change blocks_seen alone
            same_diag(eng.simulate(diagnostics=True, capture=4, max_errors=9, block=block, poll_blocks=poll, **kw), stop)
            plain = eng.simulate(max_errors=9, block=block, poll_blocks=poll, **kw)
            assert {c: plain[c] for c in COUNTERS} == {c: stop[c] for c in COUNTERS}
    finally:
        eng.set_mode("auto")


def test_one_codeword_for_every_frame_and_amp(gpu_device):
    """e == NULL: the descriptor's codeword on the channel and in the counters; QPSK is symmetric, so the all-zero word and a
    codeword give the same kind of point, and amp = Modulation.amp(snr_db) is the same point as snr_db"""
    import engine
    from modulation import Modulation
    code, dec, eng, mode = point_case("small_96_48", gpu_device)
    mod, snr_db = Modulation("qpsk"), SNR_DB[("small_96_48", "qpsk", None)]
    word = eref.unpack_rows(engine.encode_random(eng.encoder(), 1, seed=5, device=gpu_device).cpu().numpy(), code.n)[0]
    assert word.any()
    kw = dict(seed=SEED, stream_id=STREAM, modulation=mod, max_frames=1000, max_errors=10 ** 6, block=256)
    for cw in (None, word):
        got = eng.simulate(snr_db=snr_db, codeword=cw, **kw)
        state = torch.zeros(8, dtype=torch.int64, device=eng.device)
        for first in range(0, 1000, 256):
            frames = min(256, 1000 - first)
            llr = engine.sym_llr(frames, code.n, seed=SEED, stream_id=STREAM, first_frame=first, modulation=mod, snr_db=snr_db,
                                 codeword=cw, device=gpu_device)
            res = eng.decode(llr, early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
            eng.sim_count(state, res.packed_bits, res.iterations, max_frames=1000, max_errors=10 ** 6, codeword=cw)
        want = dict(zip(engine.SIM_COUNTERS, state.tolist()))
        assert {c: got[c] for c in COUNTERS} == {c: want[c] for c in COUNTERS} and got["frame_errors"] > 0
        assert eng.simulate(amp=mod.amp(snr_db), codeword=cw, **kw) == got


def test_simulator_with_a_modulation_on_both_engines_and_replay(gpu_device, tmp_path):
    from modulation import Modulation
    from simulation_framework import LDPSimulator, SimulationConfig
    name = "ira_1998_1512"
    code, dec, eng, _ = point_case(name, gpu_device)
    mod = Modulation("qam16", "rayleigh")
    snr_db = SNR_DB[(name, "qam16", "rayleigh")] - 0.5            # about 1.3 % of the frames fail: 6 errors well inside 1500
    cfg = SimulationConfig(snr_range=(snr_db, snr_db), snr_step=1.0, seed=SEED, channel="device", codeword="random",
                           results_dir=str(tmp_path), save_results=False, max_frames=1500, max_errors=6, batch_frames=256,
                           modulation=mod, capture_errors=100, stage_min_block=64)
    sim = LDPSimulator(cfg)
    results = {}
    try:
        for mode in ("auto", "stream"):
            eng.set_mode(mode)
            assert eng.info()["engine"] == ("resident" if mode == "auto" else "stream")
            with torch.no_grad():
                results[mode] = sim.simulate_decoder(dec, code, mode)
        a, b = results["auto"], results["stream"]
        assert (a.total_frames, a.total_errors, a.bit_error_rates, a.average_iterations, a.undetected_errors) == \
               (b.total_frames, b.total_errors, b.bit_error_rates, b.average_iterations, b.undetected_errors)
        assert np.array_equal(a.error_frames[0], b.error_frames[0]) and a.iteration_histograms == b.iteration_histograms
        rec = a.error_frames[0]
        assert a.total_errors[0] == 6 == len(rec) and a.total_frames[0] < 1500
        # the driver's point is DecodeEngine.simulate's
        want = eng.simulate(seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, codeword="random", modulation=mod,
                            max_frames=1500, max_errors=6, diagnostics=True, capture=100, block=999)
        assert (a.total_frames[0], a.undetected_errors[0]) == (want["frames"], want["undetected_errors"])
        assert np.array_equal(rec, want["error_frames"])
        out = sim.replay_errors(dec, code, snr_db, rec["frame"])
        sent = eref.unpack_rows(out["codewords"].cpu().numpy(), code.n)
        assert sent.any(axis=1).all() and not code.tanner_graph().syndrome(sent).any()
        wrong = (out["bits"].cpu().numpy() != sent).sum(axis=1)
        assert np.array_equal(wrong, rec["wrong_bits"]) and (wrong > 0).all()
        assert np.array_equal(out["iterations"].cpu().numpy(), rec["iterations"])
    finally:
        eng.set_mode("auto")


def test_what_the_point_refuses(gpu_device):
    from modulation import Modulation
    from rate_matching import RateMatching
    from simulation_framework import SimulationConfig
    code, dec, eng, _ = point_case("small_96_48", gpu_device)
    q16 = Modulation("qam16")
    ok = dict(seed=1, snr_db=9.0, max_frames=10, max_errors=10, block=64, codeword="random", modulation=q16)
    assert eng.simulate(**ok)["frames"] == 10
    with pytest.raises(ValueError, match="rate matching"):
        eng.simulate(rate_matching=RateMatching(code.n, punctured=[1]), **ok)
    with pytest.raises(ValueError, match="rate_matching"):
        SimulationConfig(channel="device", codeword="random", modulation=q16, rate_matching=RateMatching(code.n, punctured=[1]))
    with pytest.raises(ValueError, match='codeword="random"'):
        SimulationConfig(channel="device", modulation=q16)
    with pytest.raises(NotImplementedError, match="float64"):
        dec._engine(torch.float64, gpu_device).simulate(**ok)
    with pytest.raises(ValueError):
        eng.simulate(**dict(ok, snr_db=None))                                          # neither snr_db nor amp
    with pytest.raises(ValueError):
        eng.simulate(scale=1.0, shift=1.0, **ok)
    with pytest.raises(ValueError):
        eng.simulate(**dict(ok, modulation="qam16"))
    with pytest.raises(ValueError, match="block"):
        eng.simulate(**dict(ok, block=0))
    with pytest.raises(ValueError, match="codeword"):
        eng.simulate(**dict(ok, codeword="zero"))
    with pytest.raises(ValueError):
        eng.simulate(**dict(ok, modulation=Modulation("qam16", interleaver=[1, 0])))     # a permutation of 2 on n = 96
    with pytest.raises(ValueError):
        eng.simulate(seed=1, snr_db=2.0, amp=1.0, max_frames=10, max_errors=10)          # amp without a modulation
