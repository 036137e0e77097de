"""
GPU tests (-m gpu) of the exact demapper on the paths that draw from the symbol channel: one SNR point in one call
(ldpc_simulate_sym_dm) against the loop written out in Python on both engines, LDPSimulator with replay of recorded frames, and
one train_stream step of PosteriorJointTrainer.  A Modulation(..., demapper="exact") is all a caller passes.
"""
import numpy as np
import pytest
import torch

import encode_reference as eref

pytestmark = pytest.mark.gpu

T = 10
SEED, STREAM = (0x9E37 << 32) | 0x7654321, 3700
COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done")
FRAMES = 2048
# Es/N0 of tests/test_gpu_simulate_sym.py for 16-QAM on the two codes (BasicMinSum 0.7, T = 10, random codewords): about 2 % of
# the frames fail under max-log there, and the exact rule moves that little
SNR_DB = {"small_96_48": 9.5, "ira_1998_1512": 11.5}


def point_case(name, gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code(name, T)
    dec = BasicMinSumDecoder(code, 0.7)
    return code, dec, _engine_of(dec, gpu_device)


def written_out(eng, mod, snr_db, max_frames, max_errors, capture, block):
    """the loop ldpc_simulate_sym_dm runs, one engine call per step: encode_random -> sym_llr -> decode -> counters"""
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


@pytest.mark.parametrize("name", ["small_96_48", "ira_1998_1512"])
def test_one_call_with_the_exact_demapper_equals_the_written_out_loop(name, gpu_device):
    from modulation import Modulation
    code, dec, eng = point_case(name, gpu_device)
    snr_db = SNR_DB[name]
    pos = np.random.default_rng(code.n).permutation(code.n)
    engines = set()
    try:
        for mode in ("auto", "stream"):
            eng.set_mode(mode)
            engines.add(eng.info()["engine"])
            for fading, p in ((None, None), ("rayleigh", pos)):
                mod = Modulation("qam16", fading, p, demapper="exact")
                db = snr_db + (5.0 if fading else 0.0)
                want = written_out(eng, mod, db, FRAMES, 10 ** 6, 8, 512)
                kw = dict(seed=SEED, stream_id=STREAM, snr_db=db, codeword="random", modulation=mod, max_frames=FRAMES)
                got = eng.simulate(diagnostics=True, capture=8, max_errors=10 ** 6, block=FRAMES, poll_blocks=1, **kw)
                same_diag(got, want)
                ml = eng.simulate(diagnostics=True, capture=8, max_errors=10 ** 6, block=FRAMES, poll_blocks=1,
                                  **dict(kw, modulation=Modulation("qam16", fading, p)))
                print(f"{name} {eng.info()['engine']} 16-QAM {fading} at {db} dB, {FRAMES} frames: {got['frame_errors']} frame "
                      f"errors / {got['bit_errors']} bit errors exact, {ml['frame_errors']} / {ml['bit_errors']} max-log")
                assert got["frames"] == FRAMES and got["frame_errors"] > 0 and got["done"] == 1
                assert (got["bit_errors"], got["iterations"]) != (ml["bit_errors"], ml["iterations"])   # it is another demapper
                # a point that stops on its error limit, cut into blocks in two ways, without diagnostics too
                stop = written_out(eng, mod, db, FRAMES, 3, 2, 333)
                assert stop["frame_errors"] == 3
                for block, poll in ((100, 5), (4096, 1)):
                    same_diag(eng.simulate(diagnostics=True, capture=2, max_errors=3, block=block, poll_blocks=poll, **kw), stop)
                    plain = eng.simulate(max_errors=3, block=block, poll_blocks=poll, **kw)
                    assert {c: plain[c] for c in COUNTERS} == {c: stop[c] for c in COUNTERS}
        assert "stream" in engines and (name != "ira_1998_1512" or "resident" in engines)
    finally:
        eng.set_mode("auto")


def test_simulator_replays_a_recorded_frame_with_its_exact_llrs(gpu_device, tmp_path):
    import engine
    from modulation import Modulation
    from simulation_framework import LDPSimulator, SimulationConfig
    name = "ira_1998_1512"
    code, dec, eng = point_case(name, gpu_device)
    mod = Modulation("qam64", "rayleigh", demapper="exact")
    snr_db = 20.5
    cfg = SimulationConfig(snr_range=(snr_db, snr_db), snr_step=1.0, seed=SEED, channel="device", codeword="random",
                           results_dir=str(tmp_path), save_results=False, max_frames=1500, max_errors=4, batch_frames=256,
                           modulation=mod, capture_errors=100, stage_min_block=64)
    sim = LDPSimulator(cfg)
    results = {}
    try:
        for mode in ("auto", "stream"):
            eng.set_mode(mode)
            with torch.no_grad():
                results[mode] = sim.simulate_decoder(dec, code, mode)
        a, b = results["auto"], results["stream"]
        assert (a.total_frames, a.total_errors, a.bit_error_rates, a.undetected_errors) == \
               (b.total_frames, b.total_errors, b.bit_error_rates, b.undetected_errors)
        assert np.array_equal(a.error_frames[0], b.error_frames[0])
        rec = a.error_frames[0]
        print(f"64-QAM Rayleigh exact at {snr_db} dB: {a.total_errors[0]} frame errors in {a.total_frames[0]} frames")
        assert len(rec) == a.total_errors[0] and len(rec) >= 1
        out = sim.replay_errors(dec, code, snr_db, rec["frame"])
        sid = int(round(snr_db * 1000))
        for i, f in enumerate(int(f) for f in rec["frame"]):
            cw = engine.encode_random(eng.encoder(), 1, seed=SEED, stream_id=sid, first_frame=f, device=gpu_device)
            llr, samples = engine.sym_llr(1, code.n, seed=SEED, stream_id=sid, first_frame=f, modulation=mod, snr_db=snr_db,
                                          codeword=cw, device=gpu_device, want_received=True)
            assert torch.equal(out["llr"][i:i + 1].view(torch.int32), llr.view(torch.int32))
            assert torch.equal(engine.demap(samples, code.n, modulation=mod).view(torch.int32), llr.view(torch.int32))
            assert not torch.equal(engine.demap(samples, code.n, modulation=mod, demapper="maxlog"), llr)
        sent = eref.unpack_rows(out["codewords"].cpu().numpy(), code.n)
        wrong = (out["bits"].cpu().numpy() != sent).sum(axis=1)
        assert np.array_equal(wrong, rec["wrong_bits"]) and (wrong > 0).all()
        assert np.array_equal(out["iterations"].cpu().numpy(), rec["iterations"])
    finally:
        eng.set_mode("auto")


B, TT = 64, 3
GRID = [6.0, 8.0, 10.0]


def fresh_model():
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    code = codes.load_code("small_96_48", max_iterations=TT)
    model = Neural2DMinSumDecoder(code, 2, TT)
    with torch.no_grad():
        for p in model.parameters():
            p.fill_(0.3)
    return code, model


def one_step(mod, gpu_device):
    """-> (the loss of one train_stream step of a fresh trainer, the loss of the same step written out from sym_llr_mix)"""
    import codes
    import engine
    from training_framework import PosteriorJointTrainer, TrainingConfig, stream_first_frame
    cfg = dict(batch_size=B, num_epochs=1, learning_rate=0.05, snr_range=(6.0, 10.0), snr_step=2.0, device="cuda", seed=9,
               joint_posterior_loss=True)
    code, model = fresh_model()
    hist = PosteriorJointTrainer(model, TrainingConfig(**cfg), modulation=mod, codeword="random").train_stream(code, 1)
    _, ref = fresh_model()
    ref.to(gpu_device)
    ref.train(True)
    first = stream_first_frame(0, B)
    cw = engine.encode_random(codes.Encoder.from_graph(code.tanner_graph()), B, seed=9, stream_id=0, first_frame=first,
                              device=gpu_device)
    llr, targets = engine.sym_llr_mix(B, code.n, seed=9, stream_id=0, first_frame=first, modulation=mod, snr_db=GRID,
                                      codeword=cw, device=gpu_device, want_targets=True)
    loss = ref.joint_posterior_loss(llr, targets)[0]
    assert len(hist["train_losses"]) == 1 and hist["snr_points"] == GRID
    return hist["train_losses"][0], float(loss.item()), llr


def test_one_training_step_draws_the_exact_llrs(gpu_device):
    """the trainer with an exact 16-QAM modulation draws what sym_llr_mix gives under that modulation (its loss is the
    written-out step's, ==), the loss differs from the max-log trainer's on the same seed, and the max-log trainer's is what
    the plain entry point ldpc_channel_sym_mix gives: today's"""
    import _native
    import ctypes as C
    import codes
    import engine
    from modulation import Modulation
    from training_framework import stream_first_frame
    exact, exact_loop, exact_llr = one_step(Modulation("qam16", "rayleigh", demapper="exact"), gpu_device)
    maxlog, maxlog_loop, maxlog_llr = one_step(Modulation("qam16", "rayleigh"), gpu_device)
    print(f"one step, 16-QAM Rayleigh, 6 / 8 / 10 dB: loss {exact!r} exact, {maxlog!r} max-log")
    assert exact == exact_loop and maxlog == maxlog_loop and np.isfinite([exact, maxlog]).all()
    assert exact != maxlog and not torch.equal(exact_llr, maxlog_llr)
    # today's draw: the entry point without a demapper argument, called directly
    code, _ = fresh_model()
    mod = Modulation("qam16", "rayleigh")
    first = stream_first_frame(0, B)
    cw = engine.encode_random(codes.Encoder.from_graph(code.tanner_graph()), B, seed=9, stream_id=0, first_frame=first,
                              device=gpu_device)
    tab = torch.from_numpy(mod.amp_table(GRID)).to(gpu_device)
    desc, keep = mod.native(0.0, code.n, gpu_device)
    out = torch.empty((B, code.n), dtype=torch.float32, device=gpu_device)
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    _native.check(_native.load().ldpc_channel_sym_mix(C.c_void_p(out.data_ptr()), B, code.n, 9, 0, first, C.byref(desc),
                                                      C.c_void_p(tab.data_ptr()), 3, C.c_void_p(cw.data_ptr()),
                                                      (code.n + 7) // 8, None, stream), "ldpc_channel_sym_mix")
    assert torch.equal(out.view(torch.int32), maxlog_llr.view(torch.int32))
