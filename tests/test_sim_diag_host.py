"""
Host side of the Monte-Carlo diagnostics: the numpy restatement of ldpc_sim_count_diag (tests/sim_diag_reference.py) against
a block worked out by hand, against the plain fold and its own invariants; the configuration, the exports, parse_sim_diag and
the saved results.  No GPU.
"""
import json
import os

import numpy as np
import pytest

import philox_reference as ref
import sim_diag_reference as dref


def test_restatement_on_a_block_worked_out_by_hand():
    # frame            100  101  102  103  104  105  106  107
    wrong = [0, 2, 0, 1, 0, 3, 0, 4]              # 101 and 105 detected, 103 undetected; 107 lies behind the stop frame
    success = [1, 0, 1, 1, 1, 0, 1, 0]
    iters = [3, 10, 2, 4, 3, 10, 1, 10]
    T, capture = 10, 2
    state, diag = dref.sim_fold_diag([0] * 8, [0] * dref.diag_words(T, capture), wrong, iters, success, 100, T, capture,
                                     max_frames=1000, max_errors=3)
    assert state == [6, 3, 6, 32, 1, 1, 0, 0]     # frames 100..105: the third frame error is the stop frame
    hist = [0] * 11
    hist[2], hist[3], hist[4], hist[10] = 1, 2, 1, 2
    assert diag == [1, 2, 0, 0] + hist + [101, 2, 10, 0] + [103, 1, 4, 1]   # the third error is counted, not recorded
    # a launch after `done`: nothing but blocks_seen
    again, diag2 = dref.sim_fold_diag(state, diag, wrong, iters, success, 108, T, capture, 1000, 3)
    assert again == [6, 3, 6, 32, 1, 2, 0, 0] and diag2 == diag
    # the frame limit instead: four frames, one detected and one undetected error, both recorded
    state, diag = dref.sim_fold_diag([0] * 8, [0] * dref.diag_words(T, capture), wrong, iters, success, 2 ** 64 - 2, T, capture,
                                     max_frames=4, max_errors=3)
    assert state == [4, 2, 3, 19, 1, 1, 0, 0]
    assert diag[:4] == [1, 2, 0, 0] and diag[15:] == [-1, 2, 10, 0, 1, 1, 4, 1]   # frame indices wrap mod 2^64


def random_block(rng, B, T, p_err):
    wrong = np.where(rng.random(B) < p_err, rng.integers(1, 40, B), 0)
    return wrong, rng.integers(0, T + 1, B), rng.integers(0, 2, B)


@pytest.mark.parametrize("seed", range(6))
def test_state_equals_the_plain_fold_and_invariants(seed):
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 30))
    for capture in (0, 1, 5, 10 ** 4):
        for max_frames, max_errors in ((10 ** 6, 10 ** 6), (700, 10 ** 6), (10 ** 6, 17), (10 ** 6, 0), (900, 60)):
            state, plain = [0] * 8, [0] * 8
            diag = [0] * dref.diag_words(T, capture)
            first = int(rng.integers(0, 2 ** 40))
            for k in range(4):
                B = int(rng.integers(1, 400))
                wrong, iters, success = random_block(rng, B, T, 0.08)
                state, diag = dref.sim_fold_diag(state, diag, wrong, iters, success, first, T, capture, max_frames, max_errors)
                plain = ref.sim_fold(plain, wrong, iters, max_frames, max_errors)
                first += B
                assert state[:6] == plain[:6] and state[6:] == [0, 0]
                hist = np.array(diag[4:4 + T + 1])
                rec = np.array(diag[4 + T + 1:], dtype=np.int64).reshape(capture, 4)[:diag[1]]
                assert hist.sum() == state[0]
                assert (np.arange(T + 1) * hist).sum() == state[3]
                assert diag[1] == min(state[1], capture) and diag[2] == 0 and diag[3] == 0
                assert (np.diff(rec[:, 0]) > 0).all() and (rec[:, 1] > 0).all()
                assert rec[:, 3].sum() <= diag[0] <= state[1]
                if capture >= state[1]:
                    assert rec[:, 3].sum() == diag[0] and rec[:, 1].sum() == state[2]


def test_the_cut_into_blocks_does_not_matter():
    rng = np.random.default_rng(11)
    T, capture, N = 12, 7, 3000
    wrong, iters, success = random_block(rng, N, T, 0.02)
    results = []
    for block in (N, 64, 257, 1):
        state, diag = [0] * 8, [0] * dref.diag_words(T, capture)
        for a in range(0, N, block):
            state, diag = dref.sim_fold_diag(state, diag, wrong[a:a + block], iters[a:a + block], success[a:a + block], 5 + a, T,
                                             capture, 2500, 40)
        results.append((state[:5], diag))
    assert all(r == results[0] for r in results[1:]) and results[0][0][4] == 1 and results[0][1][1] == capture


def test_configuration():
    from simulation_framework import SimulationConfig
    assert SimulationConfig().diagnostics is False and SimulationConfig().capture_errors == 0
    cfg = SimulationConfig(channel="device", diagnostics=True, capture_errors=5, save_results=False)
    assert cfg.diagnostics and cfg.capture_errors == 5
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(diagnostics=True)
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(capture_errors=1)
    with pytest.raises(ValueError, match="device"):
        SimulationConfig(channel="torch", diagnostics=True, capture_errors=3)
    with pytest.raises(ValueError, match="capture_errors"):
        SimulationConfig(channel="device", capture_errors=-1)


def test_exports_and_prototypes():
    import _native
    new = ("ldpc_sim_diag_words", "ldpc_sim_count_diag_scratch_bytes", "ldpc_sim_count_diag",
           "ldpc_simulate_diag_workspace_bytes", "ldpc_simulate_diag")
    assert set(new) <= set(_native.PRODUCT_EXPORTS) and len(set(_native.PRODUCT_EXPORTS)) == len(_native.PRODUCT_EXPORTS)
    header = open(_native.HEADER).read()
    for name in new:
        assert name + "(" in header
    assert "#define LDPC_HIP_ABI_VERSION 1" in header
    sim = open(os.path.join(_native.CSRC, "ldpc_sim.hip")).read()
    for name in new:
        assert name + "(" in sim


def test_parse_sim_diag():
    import engine
    T, capture = 3, 4
    assert engine.sim_diag_words(T, capture) == dref.diag_words(T, capture) == 24
    words = [2, 3, 0, 0, 5, 6, 7, 8] + [10, 1, 3, 0] + [-1, 9, 2, 1] + [77, 4, 3, 1] + [0, 0, 0, 0]
    d = engine.parse_sim_diag(words, T, capture)
    assert d["undetected_errors"] == 2 and d["captured"] == 3
    assert d["iteration_histogram"].dtype == np.int64 and d["iteration_histogram"].tolist() == [5, 6, 7, 8]
    e = d["error_frames"]
    assert e.dtype.names == ("frame", "wrong_bits", "iterations", "undetected") and len(e) == 3
    assert e["frame"].tolist() == [10, 2 ** 64 - 1, 77] and e["wrong_bits"].tolist() == [1, 9, 4]
    assert e["iterations"].tolist() == [3, 2, 3] and e["undetected"].tolist() == [0, 1, 1]
    empty = engine.parse_sim_diag(np.zeros(4 + T + 1, dtype=np.int64), T, 0)
    assert empty["captured"] == 0 and len(empty["error_frames"]) == 0 and empty["iteration_histogram"].tolist() == [0] * 4
    with pytest.raises(ValueError):
        engine.parse_sim_diag(words[:-1], T, capture)
    with pytest.raises(ValueError):
        engine.parse_sim_diag([0, 5] + words[2:], T, capture)
    with pytest.raises(ValueError):
        engine.sim_diag_words(-1, 0)
    # the restatement's buffer parses to what it recorded
    state, diag = dref.sim_fold_diag([0] * 8, [0] * dref.diag_words(10, 2), [0, 2, 1], [3, 10, 4], [1, 0, 1], 100, 10, 2, 10, 10)
    d = engine.parse_sim_diag(diag, 10, 2)
    assert d["error_frames"].tolist() == [(101, 2, 10, 0), (102, 1, 4, 1)] and d["undetected_errors"] == 1


def parent_save(results, path):
    """what save_results wrote before the diagnostics existed, for the same result objects"""
    serializable = {name: {"decoder_name": r.decoder_name, "snr_values": r.snr_values,
                           "frame_error_rates": r.frame_error_rates, "bit_error_rates": r.bit_error_rates,
                           "average_iterations": r.average_iterations, "simulation_times": r.simulation_times,
                           "total_frames": r.total_frames, "total_errors": r.total_errors}
                    for name, r in results.items()}
    with open(path, "w") as f:
        json.dump(serializable, f, indent=2)


def test_saved_results(tmp_path):
    import engine
    from simulation_framework import LDPSimulator, SimulationConfig, SimulationResult
    sim = LDPSimulator(SimulationConfig(results_dir=str(tmp_path), save_results=True))
    plain = SimulationResult("Basic", [1.0, 2.0])
    plain.add_result(0, 0.5, 0.01, 7.5, 0.25, 200, 100)
    plain.add_result(1, 0.125, 0.001, 5.0, 0.5, 800, 100)
    assert plain.undetected_errors == [] and plain.iteration_histograms == [] and plain.error_frames == []
    sim.save_results({"Basic": plain}, "plain.json")
    parent_save({"Basic": plain}, tmp_path / "parent.json")
    assert (tmp_path / "plain.json").read_bytes() == (tmp_path / "parent.json").read_bytes()
    back = sim.load_results("plain.json")["Basic"]
    assert back.total_frames == [200, 800] and back.iteration_histograms == [] and back.error_frames == []

    rich = SimulationResult("RCQ", [1.0, 2.0])
    rich.add_result(0, 0.5, 0.01, 7.5, 0.25, 200, 100)
    rich.add_result(1, 0.125, 0.001, 5.0, 0.5, 800, 100)
    frames = np.array([(3, 2, 10, 0), (2 ** 40 + 1, 5, 4, 1)], dtype=engine.ERROR_FRAME_DTYPE)
    rich.add_diagnostics(1, 1, np.array([0, 700, 90, 10], dtype=np.int64), frames)
    assert rich.undetected_errors == [0, 1] and rich.iteration_histograms == [[], [0, 700, 90, 10]]
    sim.save_results({"RCQ": rich, "Basic": plain}, "rich.json")
    data = json.loads((tmp_path / "rich.json").read_text())
    assert "iteration_histograms" not in data["Basic"] and data["RCQ"]["undetected_errors"] == [0, 1]
    assert data["RCQ"]["error_frames"] == [[], [[3, 2, 10, 0], [2 ** 40 + 1, 5, 4, 1]]]
    back = sim.load_results("rich.json")
    assert back["Basic"].iteration_histograms == []
    r = back["RCQ"]
    assert r.undetected_errors == [0, 1] and r.iteration_histograms == [[], [0, 700, 90, 10]]
    assert len(r.error_frames[0]) == 0 and r.error_frames[1].dtype == engine.ERROR_FRAME_DTYPE
    assert np.array_equal(r.error_frames[1], frames) and r.frame_error_rates == rich.frame_error_rates
