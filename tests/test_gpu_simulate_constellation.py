"""
GPU tests (-m gpu) of one SNR point on the constellation channel: the one-call point (ldpc_simulate_con) against the same loop
written out in Python from encode_random, sym_llr, decode and sim_count, its independence of block and poll_blocks, replay of
recorded frames through LDPSimulator, and stream training on 8-PSK.  small_96_48, BasicMinSum 0.7, T = 10, random codewords;
8-PSK over AWGN and 16-APSK (4 + 12) over Rayleigh fading through a random interleaver.
"""
import numpy as np
import pytest
import torch

import encode_reference as eref

pytestmark = pytest.mark.gpu

T = 10
NAME = "small_96_48"
SEED, STREAM = (0x9E37 << 32) | 0x7654321, 3700
COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done")
FRAMES = 2048
# Es/N0 per channel at which the written-out loop sees at least 20 frame errors and at least 20 error-free frames in 2048
# frames; the counts are in the docstring of test_one_call_equals_the_written_out_loop
SNR_DB = {"psk8": 7.0, "apsk16_rayleigh": 14.0}
KINDS = tuple(SNR_DB)


def channel(kind, n, demapper="maxlog"):
    from modulation import Constellation
    if kind == "psk8":
        return Constellation.psk(8, demapper=demapper)
    pos = np.random.default_rng(n).permutation(n)
    return Constellation.apsk((4, 12), (1.0, 2.6), fading="rayleigh", interleaver=pos, demapper=demapper)


def written_out(eng, mod, snr_db, max_frames, max_errors, capture, block):
    """the loop ldpc_simulate_con runs, one engine call per step -> what DecodeEngine.simulate(diagnostics=True) returns"""
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


def point_case(gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code(NAME, T)
    dec = BasicMinSumDecoder(code, 0.7)
    return code, dec, _engine_of(dec, gpu_device)


@pytest.mark.parametrize("demapper", ["maxlog", "exact"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_call_equals_the_written_out_loop(kind, demapper, gpu_device):
    """All eight state words but blocks_seen, and the whole diag buffer (stop histogram and captured records), of the native
    point equal the written-out loop's, and the point does not depend on block and poll_blocks.
    Frame errors of the written-out loop in 2048 frames at SNR_DB (a condition on the inputs, not what is tested):
    8-PSK 7.0 dB: 75 under max-log, 74 under exact; 16-APSK Rayleigh interleaved 14.0 dB: 235 under max-log, 224 under exact --
    at least 20 frame errors and at least 20 error-free frames each."""
    code, dec, eng = point_case(gpu_device)
    mod, snr_db = channel(kind, code.n, demapper), SNR_DB[kind]
    want = written_out(eng, mod, snr_db, FRAMES, 10 ** 6, 8, FRAMES)
    print(f"{kind} {demapper} at {snr_db} dB: {want['frame_errors']} frame errors in {want['frames']} frames")
    assert want["frames"] == FRAMES and want["done"] == 1 and want["captured"] == 8
    kw = dict(seed=SEED, stream_id=STREAM, snr_db=snr_db, codeword="random", modulation=mod, max_frames=FRAMES)
    got = eng.simulate(diagnostics=True, capture=8, max_errors=10 ** 6, block=FRAMES, poll_blocks=1, **kw)
    same_diag(got, want)
    assert got["blocks_seen"] == want["blocks_seen"] == 1
    assert got["detected_errors"] == got["frame_errors"] - got["undetected_errors"]
    same_diag(eng.simulate(diagnostics=True, capture=8, max_errors=10 ** 6, block=FRAMES, amp=mod.amp(snr_db),
                           **dict(kw, snr_db=None)), got)
    # a point that stops on its error limit, cut into blocks in three ways
    stop = written_out(eng, mod, snr_db, FRAMES, 9, 4, 333)
    assert stop["frame_errors"] == 9 and stop["frames"] < FRAMES
    for block, poll in ((1, 64), (100, 5), (2048, 1)):              # block and poll_blocks change blocks_seen alone
        same_diag(eng.simulate(diagnostics=True, capture=4, max_errors=9, block=block, poll_blocks=poll, **kw), stop)
        plain = eng.simulate(max_errors=9, block=block, poll_blocks=poll, **kw)
        assert {c: plain[c] for c in COUNTERS} == {c: stop[c] for c in COUNTERS}


def test_one_codeword_for_every_frame(gpu_device):
    """e == NULL: the descriptor's codeword on the channel and in the counters"""
    import engine
    code, dec, eng = point_case(gpu_device)
    mod, snr_db = channel("psk8", code.n), SNR_DB["psk8"]
    word = eref.unpack_rows(engine.encode_random(eng.encoder(), 1, seed=5, device=gpu_device).cpu().numpy(), code.n)[0]
    assert word.any()
    kw = dict(seed=SEED, stream_id=STREAM, modulation=mod, max_frames=600, max_errors=10 ** 6, block=256)
    got = eng.simulate(snr_db=snr_db, codeword=word, **kw)
    state = torch.zeros(8, dtype=torch.int64, device=eng.device)
    for first in range(0, 600, 256):
        frames = min(256, 600 - first)
        llr = engine.sym_llr(frames, code.n, seed=SEED, stream_id=STREAM, first_frame=first, modulation=mod, snr_db=snr_db,
                             codeword=word, device=gpu_device)
        res = eng.decode(llr, early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
        eng.sim_count(state, res.packed_bits, res.iterations, max_frames=600, max_errors=10 ** 6, codeword=word)
    want = dict(zip(engine.SIM_COUNTERS, state.tolist()))
    assert {c: got[c] for c in COUNTERS} == {c: want[c] for c in COUNTERS} and got["frame_errors"] > 0


@pytest.mark.parametrize("kind", KINDS)
def test_simulator_replays_a_captured_frame_bit_for_bit(kind, gpu_device, tmp_path):
    from simulation_framework import LDPSimulator, SimulationConfig
    code, dec, eng = point_case(gpu_device)
    mod, snr_db = channel(kind, code.n), SNR_DB[kind]
    cfg = SimulationConfig(snr_range=(snr_db, snr_db), snr_step=1.0, seed=SEED, channel="device", codeword="random",
                           results_dir=str(tmp_path), save_results=False, max_frames=1500, max_errors=6, batch_frames=256,
                           modulation=mod, capture_errors=100, stage_min_block=64)
    sim = LDPSimulator(cfg)
    with torch.no_grad():
        res = sim.simulate_decoder(dec, code, kind)
    rec = res.error_frames[0]
    assert res.total_errors[0] == 6 == len(rec) and res.total_frames[0] < 1500
    # the driver's point is DecodeEngine.simulate's
    want = eng.simulate(seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, codeword="random", modulation=mod,
                        max_frames=1500, max_errors=6, diagnostics=True, capture=100, block=999)
    assert (res.total_frames[0], res.undetected_errors[0]) == (want["frames"], want["undetected_errors"])
    assert np.array_equal(rec, want["error_frames"])
    out = sim.replay_errors(dec, code, snr_db, rec["frame"])
    sent = eref.unpack_rows(out["codewords"].cpu().numpy(), code.n)
    assert sent.any(axis=1).all() and not code.tanner_graph().syndrome(sent).any()
    wrong = (out["bits"].cpu().numpy() != sent).sum(axis=1)
    assert np.array_equal(wrong, rec["wrong_bits"]) and (wrong > 0).all()
    assert np.array_equal(out["iterations"].cpu().numpy(), rec["iterations"])
    # the redrawn LLRs are the frame's own: the block draw that holds it gives the same row
    import engine
    f = int(rec["frame"][0])
    cw = engine.encode_random(eng.encoder(), f + 1, seed=SEED, stream_id=int(round(snr_db * 1000)), device=gpu_device)
    block = engine.sym_llr(f + 1, code.n, seed=SEED, stream_id=int(round(snr_db * 1000)), modulation=mod, snr_db=snr_db,
                           codeword=cw, device=gpu_device)
    assert torch.equal(block[f].view(torch.int32), out["llr"][0].view(torch.int32))


def test_what_the_point_refuses(gpu_device):
    from rate_matching import RateMatching
    code, dec, eng = point_case(gpu_device)
    psk8 = channel("psk8", code.n)
    ok = dict(seed=1, snr_db=6.0, max_frames=10, max_errors=10, block=64, codeword="random", modulation=psk8)
    assert eng.simulate(**ok)["frames"] == 10
    with pytest.raises(ValueError, match="rate matching"):
        eng.simulate(rate_matching=RateMatching(code.n, punctured=[1]), **ok)
    with pytest.raises(NotImplementedError, match="float64"):
        dec._engine(torch.float64, gpu_device).simulate(**ok)
    with pytest.raises(ValueError):
        eng.simulate(**dict(ok, snr_db=None))                                          # neither snr_db nor amp
    with pytest.raises(ValueError):
        eng.simulate(scale=1.0, shift=1.0, **ok)
    with pytest.raises(ValueError, match="block"):
        eng.simulate(**dict(ok, block=0))
    with pytest.raises(ValueError):
        from modulation import Constellation
        eng.simulate(**dict(ok, modulation=Constellation.psk(8, interleaver=[1, 0])))   # a permutation of 2 on n = 96


def test_stream_training_on_8psk_is_finite_and_reproducible(gpu_device):
    """a few steps of PosteriorJointTrainer(..., modulation=Constellation.psk(8), codeword="random").train_stream: the losses
    are finite, the first step's loss is the loss of the block drawn by hand from (seed, step), and a second trainer with the
    same seed gives the same losses and parameters bit for bit"""
    import codes
    import engine
    from modulation import Constellation
    from neural_2d_decoder import Neural2DMinSumDecoder
    from training_framework import PosteriorJointTrainer, TrainingConfig, stream_first_frame
    B, grid = 64, [4.0, 6.0, 8.0]

    def run():
        code = codes.load_code(NAME, max_iterations=3)
        model = Neural2DMinSumDecoder(code, 2, 3)
        with torch.no_grad():
            for p in model.parameters():
                p.fill_(0.3)
        cfg = TrainingConfig(batch_size=B, num_epochs=3, learning_rate=0.05, snr_range=(4.0, 8.0), snr_step=2.0, device="cuda",
                             seed=9, joint_posterior_loss=True)
        trainer = PosteriorJointTrainer(model, cfg, modulation=Constellation.psk(8), codeword="random")
        hist = trainer.train_stream(code, 1)
        return code, model, hist

    code, model, hist = run()
    assert len(hist["train_losses"]) == 3 and np.isfinite(hist["train_losses"]).all() and hist["snr_points"] == grid
    assert np.isfinite(np.asarray(hist["train_iteration_losses"])).all()
    _, again, hist2 = run()
    assert hist2["train_losses"] == hist["train_losses"] and hist2["train_iteration_losses"] == hist["train_iteration_losses"]
    assert all(torch.equal(a, b) for a, b in zip(model.parameters(), again.parameters()))
    # step 0 by hand
    fresh = Neural2DMinSumDecoder(code, 2, 3)
    with torch.no_grad():
        for p in fresh.parameters():
            p.fill_(0.3)
    fresh.to(gpu_device)
    enc = codes.Encoder.from_graph(code.tanner_graph())
    first = stream_first_frame(0, B)
    cw = engine.encode_random(enc, B, seed=9, stream_id=0, first_frame=first, device=gpu_device)
    llr, targets = engine.sym_llr_mix(B, code.n, seed=9, stream_id=0, first_frame=first, modulation=Constellation.psk(8),
                                      snr_db=grid, codeword=cw, device=gpu_device, want_targets=True)
    assert set(np.unique(targets.cpu().numpy())) == {0.0, 1.0}
    loss, _, _, _ = fresh.joint_posterior_loss(llr, targets)
    assert float(loss.item()) == hist["train_losses"][0]
