#!/usr/bin/env python3
"""Throughput of the Monte-Carlo driver with both channels: tools/time_simulator.py's workload -- the (1998,1512) code, Basic
min-sum 0.7, batch_frames=65536, 2e6 frames at four SNRs -- once with channel="torch" (torch.randn draw, host stop rule) and
once with channel="device" (counter-based AWGN kernel, device-side counters, one native call per point on the resident
engine).  One JSON line per (channel, SNR)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: F401,E402  (package path)
import codes  # noqa: E402
from ldpc_decoder import BasicMinSumDecoder  # noqa: E402
from simulation_framework import LDPSimulator, SimulationConfig, _engine_of  # noqa: E402

code = codes.load_code("ira_1998_1512", max_iterations=10)
dec = BasicMinSumDecoder(code, 0.7)
for channel in ("torch", "device"):
    sim = LDPSimulator(SimulationConfig(save_results=False, batch_frames=65536, seed=1, channel=channel))
    sim.simulate_single_snr(dec, code, 5.0, 65536, 10 ** 9)          # warm-up: engine build, allocator
    engine = _engine_of(dec, sim.config.device).info()["engine"]
    for snr in (3.0, 4.5, 5.5, 6.5):
        fer, ber, avg_it, secs, frames, errs = sim.simulate_single_snr(dec, code, snr, 2_000_000, 10 ** 9)
        print(json.dumps({"channel": channel, "engine": engine, "snr_db": snr, "frames": frames, "frames_per_s": frames / secs,
                          "fer": fer, "ber": ber, "avg_iterations": avg_it, "frame_errors": errs, "seconds": secs}))
