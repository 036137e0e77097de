"""
Monte-Carlo diagnostics end to end (ldpc_simulate_diag, DecodeEngine.simulate(diagnostics=True), LDPSimulator(channel="device",
diagnostics=True)) against a Python fold over the same frames -- engine.awgn_llr -> decode by the CPU oracle -> the restated
counters of tests/sim_diag_reference.py -- on small_96_48, T = 10, in three regimes that have detected AND undetected frame
errors; and LDPSimulator.replay_errors on what was captured.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sim_diag_reference as dref
from test_gpu_simulate import QP, null_space_vector

pytestmark = pytest.mark.gpu

SEED, T = 9, 10
# family, snr, max_frames, max_errors: at 2.0 dB the error limit stops the point mid-run
REGIMES = {"basic-3.0": ("basic", 3.0, 2500, 1000), "basic-2.0": ("basic", 2.0, 3000, 200), "rcq-3.0": ("rcq", 3.0, 2500, 1000)}
COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done")


def make_decoder(family, code, oracle_mod):
    """(host decoder, oracle decode of a float32 LLR block -> (bits, iterations, success))"""
    from ldpc_decoder import BasicMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    g = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)
    if family == "basic":
        dec = BasicMinSumDecoder(code, 0.7)
        cpu = lambda x: oracle_mod.basic_minsum(og, x, 0.7, T, dtype=np.float32)
    else:
        dec = RCQMinSumDecoder(code, 3, 8, QP, T)
        cpu = lambda x: oracle_mod.rcq(og, x, 3, QP, T)

    def oracle_decode(x):
        out = cpu(x)
        return out[0], out[2], out[3]
    return dec, oracle_decode


def engine_decode(eng):
    def run(x):
        res = eng.decode(torch.from_numpy(x).to(eng.device), early_stop=True, want_posterior=False)
        return res.bits.cpu().numpy(), res.iterations.cpu().numpy(), res.success.cpu().numpy()
    return run


def decoded_frames(decode, n, dev, snr_db, frames, codeword=None):
    """(wrong bits, iterations, success) of frames 0 .. frames - 1 of the point's stream"""
    import engine
    x = engine.awgn_llr(frames, n, seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, codeword=codeword,
                        device=dev).cpu().numpy()
    bits, iters, success = decode(x)
    wrong = (bits != 0) ^ (np.asarray(codeword) != 0)[None, :] if codeword is not None else (bits != 0)
    return wrong.sum(axis=1), np.asarray(iters), np.asarray(success).astype(np.uint8)


def fold(frames, capture, max_frames, max_errors, block=500):
    """the point block by block through the restatement -> what DecodeEngine.simulate(diagnostics=True) must return"""
    import engine
    wrong, iters, success = frames
    state, diag = [0] * 8, [0] * dref.diag_words(T, capture)
    for a in range(0, max_frames, block):
        b = min(a + block, max_frames)
        state, diag = dref.sim_fold_diag(state, diag, wrong[a:b], iters[a:b], success[a:b], a, T, capture, max_frames, max_errors)
    want = dict(zip(COUNTERS, state[:5]))
    want.update(engine.parse_sim_diag(diag, T, capture))
    want["detected_errors"] = want["frame_errors"] - want["undetected_errors"]
    return want


def same(got, want):
    assert {k: got[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}
    for k in ("undetected_errors", "detected_errors", "captured"):
        assert got[k] == want[k], k
    assert got["iteration_histogram"].dtype == np.int64 and got["iteration_histogram"].shape == (T + 1,)
    assert np.array_equal(got["iteration_histogram"], want["iteration_histogram"])
    assert got["error_frames"].dtype == want["error_frames"].dtype and np.array_equal(got["error_frames"], want["error_frames"])


_ORACLE = {}


def oracle_frames(name, code, dev, oracle_mod):
    """every frame of a regime decoded by the oracle, once for the whole module"""
    if name not in _ORACLE:
        family, snr_db, max_frames, _ = REGIMES[name]
        _ORACLE[name] = decoded_frames(make_decoder(family, code, oracle_mod)[1], code.n, dev, snr_db, max_frames)
    return _ORACLE[name]


def native_point(eng, snr_db, max_frames, max_errors, **kw):
    return eng.simulate(seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, max_frames=max_frames,
                        max_errors=max_errors, **kw)


def driver_point(dec, code, snr_db, max_frames, max_errors, tmp_path, **kw):
    """one point through LDPSimulator.simulate_decoder -> the keys of DecodeEngine.simulate(diagnostics=True)"""
    from simulation_framework import LDPSimulator, SimulationConfig
    cfg = SimulationConfig(snr_range=(snr_db, snr_db), snr_step=1.0, max_frames=max_frames, max_errors=max_errors, seed=SEED,
                           channel="device", diagnostics=True, results_dir=str(tmp_path), save_results=False, **kw)
    sim = LDPSimulator(cfg)
    with torch.no_grad():
        r = sim.simulate_decoder(dec, code, "d")
    assert r.snr_values == [snr_db] and len(r.undetected_errors) == len(r.iteration_histograms) == len(r.error_frames) == 1
    frames, errs = r.total_frames[0], r.total_errors[0]
    return sim, {"frames": frames, "frame_errors": errs, "fer": r.frame_error_rates[0], "ber": r.bit_error_rates[0],
                 "avg_it": r.average_iterations[0], "undetected_errors": r.undetected_errors[0],
                 "iteration_histogram": r.iteration_histograms[0], "error_frames": r.error_frames[0]}


@pytest.mark.parametrize("name", list(REGIMES))
def test_diagnostics_equal_the_fold_over_the_oracle(name, gpu_device, oracle_mod, tmp_path):
    import codes
    from simulation_framework import _engine_of
    family, snr_db, max_frames, max_errors = REGIMES[name]
    code = codes.load_code("small_96_48", T)
    dec, _ = make_decoder(family, code, oracle_mod)
    eng = _engine_of(dec, gpu_device)
    frames = oracle_frames(name, code, gpu_device, oracle_mod)
    kw = dict(snr_db=snr_db, max_frames=max_frames, max_errors=max_errors)
    full = fold(frames, 10 ** 4, max_frames, max_errors)
    # the regime is one: detected and undetected errors, a spread of stop iterations, no failing frame with correct decisions
    print(name, {k: full[k] for k in COUNTERS}, "undetected", full["undetected_errors"], full["iteration_histogram"].tolist())
    assert full["undetected_errors"] >= 1 and full["detected_errors"] >= 1 and full["done"] == 1
    assert (full["iteration_histogram"] > 0).sum() >= 3 and full["captured"] == full["frame_errors"]
    assert not ((frames[0] == 0) & (frames[2] == 0)).any()
    if name == "basic-2.0":
        assert full["frame_errors"] == max_errors and full["frames"] < max_frames
    plain = native_point(eng, **kw)
    for capture in (0, 3, 10 ** 4):
        want = fold(frames, capture, max_frames, max_errors, block=333)
        assert want["captured"] == min(capture, want["frame_errors"])
        got = native_point(eng, diagnostics=True, capture=capture, **kw)
        same(got, want)
        assert {k: got[k] for k in COUNTERS} == {k: plain[k] for k in COUNTERS}          # the plain path counts the same
    # nothing depends on the block size or on how often the host looks
    for capture, blocks in ((10 ** 4, (64, 257, 4096)), (3, (64, 4096))):
        want = fold(frames, capture, max_frames, max_errors)
        for block in blocks:
            for poll in (1, 7):
                same(native_point(eng, diagnostics=True, capture=capture, block=block, poll_blocks=poll, **kw), want)
    # both engines, the native call and the driver (the streaming engine with and without the staged early stop)
    want = fold(frames, 5, max_frames, max_errors)
    for mode in ("auto", "stream"):
        eng.set_mode(mode)
        if mode == "stream":
            assert eng.info()["engine"] == "stream"
        same(native_point(eng, diagnostics=True, capture=5, block=300, poll_blocks=2, **kw), want)
        for staged in (False, True):
            _, got = driver_point(dec, code, snr_db, max_frames, max_errors, tmp_path, capture_errors=5, batch_frames=200,
                                  staged_early_stop=staged, stage_min_block=64)
            assert (got["frames"], got["frame_errors"]) == (want["frames"], want["frame_errors"])
            assert got["fer"] == want["frame_errors"] / want["frames"] and got["avg_it"] == want["iterations"] / want["frames"]
            assert got["ber"] == want["bit_errors"] / (want["frames"] * code.n)
            assert got["undetected_errors"] == want["undetected_errors"]
            assert got["iteration_histogram"] == want["iteration_histogram"].tolist()
            assert np.array_equal(got["error_frames"], want["error_frames"])
    eng.set_mode("auto")


@pytest.mark.parametrize("name", list(REGIMES))
def test_nonzero_codeword(name, gpu_device, oracle_mod):
    import codes
    import engine
    from simulation_framework import _engine_of
    family, snr_db, max_frames, max_errors = REGIMES[name]
    code = codes.load_code("small_96_48", T)
    H = (np.asarray(code.H) != 0).astype(np.uint8)
    c = null_space_vector(H, np.random.default_rng(21))
    assert c.any() and not ((H @ c) & 1).any()
    dec, _ = make_decoder(family, code, oracle_mod)
    eng = _engine_of(dec, gpu_device)
    kw = dict(snr_db=snr_db, max_frames=max_frames, max_errors=max_errors)
    sent = decoded_frames(engine_decode(eng), code.n, gpu_device, snr_db, max_frames, codeword=c)
    want = fold(sent, 40, max_frames, max_errors)
    assert want["detected_errors"] >= 1 and (family != "basic" or want["undetected_errors"] >= 1)
    same(native_point(eng, diagnostics=True, capture=40, codeword=c, block=100, poll_blocks=5, **kw), want)
    if family != "basic":
        return
    # min-sum is sign symmetric: the mirrored LLRs give mirrored messages and posteriors exactly, so the diagnostics equal the
    # all-zero run's -- unless a posterior is exactly 0 somewhere (its decision does not mirror)
    x = engine.awgn_llr(want["frames"], code.n, seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, device=gpu_device)
    exact_zero = any(bool((eng.decode(x, early_stop=False, want_bits=False, max_iters=t).posterior == 0).any())
                     for t in range(1, T + 1))
    if not exact_zero:
        same(native_point(eng, diagnostics=True, capture=40, **kw), want)


@pytest.mark.parametrize("name", ["basic-2.0", "rcq-3.0"])
def test_replay_reproduces_every_captured_frame(name, gpu_device, oracle_mod, tmp_path):
    import codes
    family, snr_db, max_frames, max_errors = REGIMES[name]
    code = codes.load_code("small_96_48", T)
    dec, _ = make_decoder(family, code, oracle_mod)
    c = null_space_vector((np.asarray(code.H) != 0).astype(np.uint8), np.random.default_rng(21)) if family == "rcq" else None
    sim, got = driver_point(dec, code, snr_db, max_frames, max_errors, tmp_path, capture_errors=10 ** 4, batch_frames=512,
                            codeword=c)
    rec = got["error_frames"]
    assert len(rec) == got["frame_errors"] > 0 and rec["undetected"].sum() == got["undetected_errors"]
    assert c is not None or got["undetected_errors"] >= 1
    assert (np.diff(rec["frame"].astype(np.int64)) > 0).all() and int(rec["frame"][-1]) < got["frames"]
    out = sim.replay_errors(dec, code, snr_db, rec["frame"])
    assert out["frames"] == rec["frame"].tolist() and out["llr"].shape == out["posterior"].shape == (len(rec), code.n)
    sent = np.zeros(code.n, np.int64) if c is None else c.astype(np.int64)
    wrong = (out["bits"].cpu().numpy() != sent[None, :]).sum(axis=1)
    assert np.array_equal(wrong, rec["wrong_bits"]) and (wrong > 0).all()
    assert np.array_equal(out["iterations"].cpu().numpy(), rec["iterations"])
    assert np.array_equal(out["success"].cpu().numpy().astype(np.int64), rec["undetected"])
    # frames that were consumed and not captured replay as correct
    others = np.setdiff1d(np.arange(got["frames"]), rec["frame"].astype(np.int64))[:300]
    ok = sim.replay_errors(dec, code, snr_db, others)
    assert not (ok["bits"].cpu().numpy() != sent[None, :]).any() and bool(ok["success"].all())
    assert sim.replay_errors(dec, code, snr_db, [])["llr"].shape == (0, code.n)


def test_resident_point_on_the_1998_1512_code(gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code("ira_1998_1512", T)
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), gpu_device)
    assert eng.info()["engine"] == "resident"
    kw = dict(snr_db=3.0, max_frames=4096, max_errors=10 ** 9)
    plain = native_point(eng, block=1000, poll_blocks=2, **kw)
    for capture, block in ((20, 1000), (10 ** 4, 4096)):
        got = native_point(eng, diagnostics=True, capture=capture, block=block, poll_blocks=2, **kw)
        assert {k: got[k] for k in COUNTERS} == {k: plain[k] for k in COUNTERS} and got["frames"] == 4096
        hist, rec = got["iteration_histogram"], got["error_frames"]
        assert hist.sum() == got["frames"] and (np.arange(T + 1) * hist).sum() == got["iterations"] and hist[0] == 0
        assert got["captured"] == len(rec) == min(got["frame_errors"], capture) and got["frame_errors"] >= 1
        assert (np.diff(rec["frame"].astype(np.int64)) > 0).all() and int(rec["frame"].max()) < 4096
        assert (rec["wrong_bits"] > 0).all() and (rec["iterations"] >= 1).all() and (rec["iterations"] <= T).all()
        assert rec["undetected"].sum() <= got["undetected_errors"] <= got["frame_errors"]
        assert got["detected_errors"] == got["frame_errors"] - got["undetected_errors"]
        if capture >= got["frame_errors"]:
            assert rec["undetected"].sum() == got["undetected_errors"] and rec["wrong_bits"].sum() == got["bit_errors"]


def test_what_the_diagnostics_refuse(gpu_device, tmp_path):
    import _native
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import LDPSimulator, SimulationConfig
    lib = _native.load()
    code = codes.load_code("small_96_48", T)
    dec = BasicMinSumDecoder(code, 0.7)
    eng = dec._engine(torch.float32, gpu_device)
    ok = dict(seed=1, snr_db=3.0, max_frames=100, max_errors=10)
    with pytest.raises(NotImplementedError, match="float64"):
        dec._engine(torch.float64, gpu_device).simulate(diagnostics=True, **ok)
    with pytest.raises(ValueError, match="capture"):
        eng.simulate(capture=3, **ok)
    with pytest.raises(ValueError, match="capture"):
        eng.simulate(diagnostics=True, capture=-1, **ok)
    with pytest.raises(ValueError, match="block"):
        eng.simulate(diagnostics=True, block=0, **ok)
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(channel="torch", diagnostics=True)
    with pytest.raises(ValueError, match="device"):
        LDPSimulator(SimulationConfig(save_results=False)).replay_errors(dec, code, 3.0, [1])
    desc = _native.SimDesc(seed=1, stream_id=0, first_frame=0, scale=2.0, shift=2.0, codeword_packed=None, max_frames=10,
                           max_errors=10, block=64, poll_blocks=1)
    out, words = np.zeros(8, dtype=np.int64), np.zeros(lib.ldpc_sim_diag_words(T, 2), dtype=np.int64)
    need = lib.ldpc_simulate_diag_workspace_bytes(eng.handle, 64, 2)
    assert need > lib.ldpc_simulate_workspace_bytes(eng.handle, 64) and lib.ldpc_simulate_diag_workspace_bytes(eng.handle, 0, 2) == 0
    assert lib.ldpc_simulate_diag_workspace_bytes(eng.handle, 64, -1) == 0
    assert lib.ldpc_simulate_diag_workspace_bytes(eng.handle, 64, 3) >= need
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    p = C.c_void_p(ws.data_ptr())
    o, w = _native.ptr(out), _native.ptr(words)
    assert lib.ldpc_simulate_diag(None, C.byref(desc), 2, o, w, p, need, None) == -1
    assert lib.ldpc_simulate_diag(eng.handle, C.byref(desc), 2, o, None, p, need, None) == -1
    assert lib.ldpc_simulate_diag(eng.handle, C.byref(desc), -1, o, w, p, need, None) == -1 and b"capture" in lib.ldpc_last_error()
    assert lib.ldpc_simulate_diag(eng.handle, C.byref(desc), 2, o, w, None, need, None) == -1
    assert lib.ldpc_simulate_diag(eng.handle, C.byref(desc), 2, o, w, p, need - 1, None) == -4
    assert b"workspace" in lib.ldpc_last_error() and not out.any() and not words.any()
    assert lib.ldpc_simulate_diag(eng.handle, C.byref(desc), 2, o, w, p, need, None) == 0
    assert out[0] == 10 and out[4] == 1 and out[6] == 0 and out[7] == 0 and words[4:4 + T + 1].sum() == 10 and words[2] == 0
    # no frames asked for: nothing drawn, nothing binned, the point is done at once
    got = eng.simulate(seed=1, snr_db=3.0, max_frames=0, max_errors=10, diagnostics=True, capture=4)
    assert got["frames"] == 0 and got["done"] == 1 and not got["iteration_histogram"].any() and len(got["error_frames"]) == 0
