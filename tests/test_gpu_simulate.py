"""
One SNR point on the device (ldpc_simulate, DecodeEngine.simulate, LDPSimulator(channel="device")) against a Python fold over
the same frames -- engine.awgn_llr -> decode -> the restated stop rule of tests/philox_reference.py -- with the decode done by
the engine and by the CPU oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import philox_reference as ref

pytestmark = pytest.mark.gpu

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
# the three regimes of the oracle test of the torch channel (tests/test_simulation_framework.py): snr, max_frames, max_errors
REGIMES = ((3.0, 2500, 30), (1.0, 700, 1000), (5.0, 1500, 5))
SEED = 9
KEYS = ("frames", "frame_errors", "bit_errors", "iterations", "done")        # blocks_seen depends on the block size


def make_decoder(family, code, oracle_mod):
    """(host decoder, oracle decode of a float32 LLR block -> (bits, iterations))"""
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder
    g = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)
    if family == "basic":
        dec = BasicMinSumDecoder(code, 0.7)
        cpu = lambda x: oracle_mod.basic_minsum(og, x, 0.7, 10, dtype=np.float32)
    elif family == "rcq":
        dec = RCQMinSumDecoder(code, 3, 8, QP, 10)
        cpu = lambda x: oracle_mod.rcq(og, x, 3, QP, 10)
    else:
        dec = Neural2DMinSumDecoder(code, 2, 10)
        rng = np.random.default_rng(7)
        with torch.no_grad():
            for k in sorted(dec.beta_weights.keys()):
                dec.beta_weights[k].fill_(float(np.float32(rng.uniform(0.5, 1.0))))
            for k in sorted(dec.alpha_weights.keys()):
                dec.alpha_weights[k].fill_(float(np.float32(rng.uniform(0.8, 1.2))))
        beta = {k: float(v.item()) for k, v in dec.beta_weights.items()}
        alpha = {k: float(v.item()) for k, v in dec.alpha_weights.items()}
        cpu = lambda x: oracle_mod.neural2d(og, x, 2, 10, beta, alpha)

    def oracle_decode(x):
        out = cpu(x)
        return out[0], out[2]
    return dec, oracle_decode


def engine_decode(eng):
    def run(x):
        res = eng.decode(torch.from_numpy(x).to(eng.device), early_stop=True, want_posterior=False)
        return res.bits.cpu().numpy(), res.iterations.cpu().numpy()
    return run


def python_fold(decode, n, dev, *, snr_db, max_frames, max_errors, block, codeword=None, convention="decoder"):
    """the point frame by frame: draw block k at first_frame = k * block, decode, XOR the codeword, the restated stop rule"""
    import engine
    scale, shift = engine.awgn_scale_shift(snr_db, convention)
    sid = int(round(snr_db * 1000)) % (1 << 32)
    state, drawn = [0] * 8, 0
    while drawn < max_frames and not state[4]:
        frames = min(block, max_frames - drawn)
        x = engine.awgn_llr(frames, n, seed=SEED, stream_id=sid, first_frame=drawn, scale=scale, shift=shift,
                            codeword=codeword, device=dev).cpu().numpy()
        bits, iters = decode(x)
        wrong = (bits != 0) ^ (np.asarray(codeword) != 0)[None, :] if codeword is not None else (bits != 0)
        state = ref.sim_fold(state, wrong.sum(axis=1), iters, max_frames, max_errors)
        drawn += frames
    if not state[4]:
        state = ref.sim_fold(state, [], [], max_frames, max_errors)
    return dict(zip(KEYS, state[:5]))


def pick(c):
    return {k: c[k] for k in KEYS}


def native_point(eng, snr_db, max_frames, max_errors, **kw):
    return eng.simulate(seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, max_frames=max_frames,
                        max_errors=max_errors, **kw)


@pytest.mark.parametrize("family", ["basic", "rcq", "neural2d"])
def test_simulate_equals_the_fold_and_the_oracle(family, gpu_device, oracle_mod, tmp_path):
    import codes
    from simulation_framework import LDPSimulator, SimulationConfig, _engine_of
    code = codes.load_code("small_96_48", 10)
    dec, oracle_decode = make_decoder(family, code, oracle_mod)
    eng = _engine_of(dec, gpu_device)
    for snr_db, max_frames, max_errors in REGIMES:
        kw = dict(snr_db=snr_db, max_frames=max_frames, max_errors=max_errors)
        want = python_fold(oracle_decode, code.n, gpu_device, block=500, **kw)
        assert 0 < want["frame_errors"] < want["frames"] and want["done"] == 1          # 0 < FER < 1 on the restated result
        assert python_fold(engine_decode(eng), code.n, gpu_device, block=384, **kw) == want
        # the result does not depend on the block size or on how often the host looks
        for block in (64, 257, 4096):
            for poll in (1, 7):
                got = native_point(eng, block=block, poll_blocks=poll, **kw)
                assert pick(got) == want, (snr_db, block, poll)
                assert got["blocks_seen"] >= -(-want["frames"] // block)
        # the driver: resident engine -> the native call, streaming engine -> its own loop with the staged early stop
        for mode in ("auto", "stream"):
            eng.set_mode(mode)
            if mode == "stream":
                assert eng.info()["engine"] == "stream"
            assert pick(native_point(eng, block=300, poll_blocks=2, **kw)) == want
            for staged in (False, True):
                cfg = SimulationConfig(max_frames=max_frames, max_errors=max_errors, batch_frames=200, seed=SEED, channel="device",
                                       results_dir=str(tmp_path), save_results=False, staged_early_stop=staged, stage_min_block=64)
                with torch.no_grad():
                    fer, ber, avg_it, _t, frames, errs = LDPSimulator(cfg).simulate_single_snr(dec, code, snr_db, max_frames,
                                                                                               max_errors)
                assert (frames, errs) == (want["frames"], want["frame_errors"])
                assert fer == errs / frames and ber == want["bit_errors"] / (frames * code.n)
                assert avg_it == want["iterations"] / frames
        eng.set_mode("auto")


def test_engine_mode_from_the_environment(gpu_device, monkeypatch):
    """LDPC_ENGINE_MODE=stream (read when an engine is created) and the default give the same counters"""
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code("small_96_48", 10)
    auto = _engine_of(BasicMinSumDecoder(code, 0.7), gpu_device)
    monkeypatch.setenv("LDPC_ENGINE_MODE", "stream")
    stream = _engine_of(BasicMinSumDecoder(code, 0.7), gpu_device)
    assert stream is not auto and stream.info()["engine"] == "stream"
    for snr_db, max_frames, max_errors in REGIMES:
        a = native_point(auto, snr_db, max_frames, max_errors, block=512, poll_blocks=3)
        s = native_point(stream, snr_db, max_frames, max_errors, block=512, poll_blocks=3)
        assert pick(a) == pick(s) and 0 < a["frame_errors"] < a["frames"]


def null_space_vector(H, rng):
    """a nonzero codeword: a random combination of a GF(2) null-space basis of H (Gauss-Jordan elimination)"""
    A = (np.asarray(H) != 0).astype(np.uint8)
    m, n = A.shape
    pivots, r = [], 0
    for c in range(n):
        rows = np.nonzero(A[r:, c])[0]
        if rows.size == 0:
            continue
        A[[r, r + rows[0]]] = A[[r + rows[0], r]]
        for i in np.nonzero(A[:, c])[0]:
            if i != r:
                A[i] ^= A[r]
        pivots.append(c)
        r += 1
        if r == m:
            break
    free = [c for c in range(n) if c not in pivots]
    x = np.zeros(n, dtype=np.uint8)
    x[free] = rng.random(len(free)) < 0.5
    for i, c in enumerate(pivots):                                   # reduced rows: x[pivot] = sum of the row's free entries
        x[c] = (A[i, free] & x[free]).sum() & 1
    return x


def test_nonzero_codeword(gpu_device, oracle_mod, tmp_path):
    import codes
    from simulation_framework import LDPSimulator, SimulationConfig, _engine_of
    code = codes.load_code("small_96_48", 10)
    H = (np.asarray(code.H) != 0).astype(np.uint8)
    c = null_space_vector(H, np.random.default_rng(21))
    assert c.any() and not ((H @ c) & 1).any()
    for family in ("basic", "rcq", "neural2d"):
        dec, _ = make_decoder(family, code, oracle_mod)
        eng = _engine_of(dec, gpu_device)
        for snr_db, max_frames, max_errors in REGIMES:
            kw = dict(snr_db=snr_db, max_frames=max_frames, max_errors=max_errors)
            direct = python_fold(engine_decode(eng), code.n, gpu_device, block=333, codeword=c, **kw)
            cfg = SimulationConfig(max_frames=max_frames, max_errors=max_errors, batch_frames=256, seed=SEED, channel="device",
                                   codeword=c, results_dir=str(tmp_path), save_results=False)
            fer, ber, avg_it, _t, frames, errs = LDPSimulator(cfg).simulate_single_snr(dec, code, snr_db, max_frames, max_errors)
            assert (frames, errs) == (direct["frames"], direct["frame_errors"])
            assert ber == direct["bit_errors"] / (frames * code.n) and avg_it == direct["iterations"] / frames
            assert pick(native_point(eng, block=100, poll_blocks=5, codeword=c, **kw)) == direct
            if family != "basic":
                continue
            # min-sum is sign symmetric: the mirrored LLRs give mirrored messages and posteriors exactly, so the counters
            # equal the all-zero run -- unless a posterior is exactly 0 somewhere (its decision does not mirror)
            zero = python_fold(engine_decode(eng), code.n, gpu_device, block=333, **kw)
            import engine
            x = engine.awgn_llr(zero["frames"], code.n, seed=SEED, stream_id=int(round(snr_db * 1000)), snr_db=snr_db,
                                device=gpu_device)
            exact_zero = any(bool((eng.decode(x, early_stop=False, want_bits=False, max_iters=t).posterior == 0).any())
                             for t in range(1, 11))
            if not exact_zero:
                assert direct == zero


def test_reference_convention_gives_fer_one(gpu_device, tmp_path):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import LDPSimulator, SimulationConfig
    code = codes.load_code("small_96_48", 10)
    dec = BasicMinSumDecoder(code, 0.7)
    for block in (64, 1000):
        cfg = SimulationConfig(max_frames=200, max_errors=50, batch_frames=block, llr_convention="reference", channel="device",
                               save_results=False, results_dir=str(tmp_path))
        fer, _ber, _it, _t, frames, errs = LDPSimulator(cfg).simulate_single_snr(dec, code, 6.0, 200, 50)
        assert fer == 1.0 and (frames, errs) == (50, 50)


def test_resident_point_on_the_1998_1512_code(gpu_device):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    code = codes.load_code("ira_1998_1512", 10)
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), gpu_device)
    assert eng.info()["engine"] == "resident"
    kw = dict(snr_db=4.0, max_frames=4096, max_errors=10 ** 9)
    want = python_fold(engine_decode(eng), code.n, gpu_device, block=1024, **kw)
    assert want["frames"] == 4096 and want["iterations"] >= 4096
    for block, poll in ((4096, 1), (1000, 2), (65536, 4)):
        assert pick(native_point(eng, block=block, poll_blocks=poll, **kw)) == want
    # an error limit that falls inside a block: in the waterfall (whichever limit comes first) and well below it
    for snr_db in (4.0, 2.0):
        kw = dict(snr_db=snr_db, max_frames=4096, max_errors=37)
        want = python_fold(engine_decode(eng), code.n, gpu_device, block=1024, **kw)
        assert want["done"] == 1 and (want["frame_errors"] == 37 or want["frames"] == 4096)
        for block in (4096, 300):
            assert pick(native_point(eng, block=block, poll_blocks=3, **kw)) == want
    assert want["frame_errors"] == 37 and want["frames"] < 4096                         # 2 dB: the error limit it is


def test_what_simulate_refuses(gpu_device):
    import _native
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    lib = _native.load()
    dec = BasicMinSumDecoder(codes.load_code("small_96_48", 10), 0.7)
    eng = dec._engine(torch.float32, gpu_device)
    ok = dict(seed=1, snr_db=3.0, max_frames=100, max_errors=10)
    with pytest.raises(ValueError, match="block"):
        eng.simulate(block=0, **ok)
    with pytest.raises(ValueError, match="poll_blocks"):
        eng.simulate(poll_blocks=0, **ok)
    with pytest.raises(ValueError):
        eng.simulate(seed=1, max_frames=1, max_errors=1)                               # neither snr_db nor (scale, shift)
    with pytest.raises(NotImplementedError, match="float64"):
        dec._engine(torch.float64, gpu_device).simulate(**ok)
    desc = _native.SimDesc(seed=1, stream_id=0, first_frame=0, scale=2.0, shift=2.0, codeword_packed=None, max_frames=10,
                           max_errors=10, block=64, poll_blocks=1)
    out = np.zeros(8, dtype=np.int64)
    need = lib.ldpc_simulate_workspace_bytes(eng.handle, 64)
    assert need >= 64 * 96 * 4 and lib.ldpc_simulate_workspace_bytes(eng.handle, 0) == 0
    assert lib.ldpc_simulate_workspace_bytes(eng.handle, 128) > need
    ws = torch.empty(need, dtype=torch.uint8, device=gpu_device)
    p = C.c_void_p(ws.data_ptr())
    assert lib.ldpc_simulate(None, C.byref(desc), _native.ptr(out), p, need, None) == -1
    assert lib.ldpc_simulate(eng.handle, None, _native.ptr(out), p, need, None) == -1
    assert lib.ldpc_simulate(eng.handle, C.byref(desc), None, p, need, None) == -1
    assert lib.ldpc_simulate(eng.handle, C.byref(desc), _native.ptr(out), None, need, None) == -1
    assert lib.ldpc_simulate(eng.handle, C.byref(desc), _native.ptr(out), p, need - 1, None) == -4
    assert b"workspace" in lib.ldpc_last_error()
    assert not out.any()
    assert lib.ldpc_simulate(eng.handle, C.byref(desc), _native.ptr(out), p, need, None) == 0
    assert out[0] == 10 and out[4] == 1 and out[6] == 0 and out[7] == 0
    # no frames asked for: nothing drawn, the point is done at once
    assert pick(eng.simulate(seed=1, snr_db=3.0, max_frames=0, max_errors=10)) == dict(zip(KEYS, (0, 0, 0, 0, 1)))
    assert pick(eng.simulate(seed=1, snr_db=3.0, max_frames=50, max_errors=0)) == dict(zip(KEYS, (0, 0, 0, 0, 1)))
