#!/usr/bin/env python3
"""What the Monte-Carlo diagnostics cost: tools/time_simulator_device.py's workload -- the (1998,1512) code, Basic min-sum 0.7,
batch_frames=65536, 2e6 frames at four SNRs, channel="device" -- with diagnostics off (the plain counters) and with diagnostics
on at capture_errors=1000.  The two legs alternate, REPEATS times each after a warm-up of both, in one process; one JSON line
per leg with the median, the smallest and the largest time of every SNR point (the spread to hold a difference against)."""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: F401,E402  (package path)
import codes  # noqa: E402
from ldpc_decoder import BasicMinSumDecoder  # noqa: E402
from simulation_framework import LDPSimulator, SimulationConfig, _engine_of  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000_000
SNRS = (3.0, 4.5, 5.5, 6.5)

code = codes.load_code("ira_1998_1512", max_iterations=10)
dec = BasicMinSumDecoder(code, 0.7)
legs = {"off": LDPSimulator(SimulationConfig(save_results=False, batch_frames=65536, seed=1, channel="device")),
        "on": LDPSimulator(SimulationConfig(save_results=False, batch_frames=65536, seed=1, channel="device", diagnostics=True,
                                            capture_errors=1000))}
for sim in legs.values():                                            # warm-up: engine build, allocator, both workspaces
    sim.simulate_single_snr(dec, code, 5.0, 2 * 65536, 10 ** 9)
engine = _engine_of(dec, legs["off"].config.device).info()["engine"]
seconds = {leg: {snr: [] for snr in SNRS} for leg in legs}
counters = {leg: {} for leg in legs}
for _ in range(REPEATS):
    for leg, sim in legs.items():
        for snr in SNRS:
            fer, ber, avg_it, secs, frames, errs = sim.simulate_single_snr(dec, code, snr, FRAMES, 10 ** 9)   # ends in a synchronise
            seconds[leg][snr].append(secs)
            counters[leg][snr] = (frames, errs, ber, avg_it)
for snr in SNRS:                                                     # the diagnostics change no counter
    assert counters["on"][snr] == counters["off"][snr], (snr, counters["on"][snr], counters["off"][snr])
for leg in legs:
    points = []
    for snr in SNRS:
        t = sorted(seconds[leg][snr])
        frames, errs, _ber, avg_it = counters[leg][snr]
        med = statistics.median(t)
        points.append({"snr_db": snr, "frames": frames, "frame_errors": errs, "avg_iterations": avg_it, "median_s": med,
                       "min_s": t[0], "max_s": t[-1], "frames_per_s": frames / med})
    print(json.dumps({"leg": "diagnostics_" + leg, "engine": engine, "repeats": REPEATS,
                      "capture_errors": legs[leg].config.capture_errors, "points": points}))
