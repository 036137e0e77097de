#!/usr/bin/env python3
"""One frame-error-rate comparison of iterative demapping with decoder feedback: code ira_1998_1512,
BasicMinSumDecoder(0.7) with T = 10, set-partitioned 8-PSK against Gray 8-PSK, no interleaver, random codewords,
SimulationConfig(iterative_demapping=K) with K = 1 against K = 4, demapping_feedback_scale 1.0 and 0.5.

    python tools/fer_iterative_demapping.py [--frames 65536] [--out profiles/demap_prior_fer.jsonl]
First a coarse scan of the one-shot (K = 1) set-partitioned leg, 8192 frames per point in 0.5 dB steps, for the first Es/N0
whose frame error rate is at most 0.8 % -- a few hundred frame errors in 65536 frames; then every leg at that Es/N0 with
--frames frames (no early end on errors), all on the same noise stream and codewords.  Prints one JSON line and appends it to
--out.  Not a test and not gated: it records which way the comparison comes out."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import numpy as np  # noqa: E402

CODE, T, FACTOR, SEED = "ira_1998_1512", 10, 0.7, 20261
SCAN = np.arange(8.0, 24.01, 0.5)


def point(dec, code, con, snr_db, frames, max_errors, K=1, scale=1.0, block=16384):
    from simulation_framework import LDPSimulator, SimulationConfig
    cfg = SimulationConfig(snr_range=(snr_db, snr_db), max_frames=frames, max_errors=max_errors, batch_frames=block, seed=SEED,
                           channel="device", codeword="random", save_results=False, modulation=con, iterative_demapping=K,
                           demapping_feedback_scale=scale)
    fer, ber, avg_iter, secs, total, errors = LDPSimulator(cfg).simulate_single_snr(dec, code, snr_db, frames, max_errors)
    return {"K": K, "feedback_scale": scale, "frames": total, "frame_errors": errors, "fer": fer, "ber": ber,
            "avg_iterations": avg_iter, "seconds": secs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demap_prior_fer.jsonl"))
    a = ap.parse_args()
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from modulation import Constellation
    code = codes.load_code(CODE, max_iterations=T)
    dec = BasicMinSumDecoder(code, factor=FACTOR)
    sp = Constellation(np.exp(2j * np.pi * np.arange(8) / 8), name="psk8sp")      # label l at angle 2 pi l / 8
    gray = Constellation.psk(8)
    scan, snr = [], None
    for s in SCAN:
        r = point(dec, code, sp, float(s), 8192, 400)
        scan.append({"snr_db": float(s), "frames": r["frames"], "frame_errors": r["frame_errors"]})
        if r["frame_errors"] <= 0.008 * r["frames"]:
            snr = float(s)
            break
    if snr is None:
        raise SystemExit("the scan found no Es/N0 with a frame error rate of at most 0.8 %: " + json.dumps(scan))
    legs = {}
    for name, con in (("psk8_set_partitioned", sp), ("psk8_gray", gray)):
        legs[name] = [point(dec, code, con, snr, a.frames, 10 ** 9),
                      point(dec, code, con, snr, a.frames, 10 ** 9, K=4, scale=1.0),
                      point(dec, code, con, snr, a.frames, 10 ** 9, K=4, scale=0.5)]
    line = json.dumps({"tool": "fer_iterative_demapping", "code": CODE, "decoder": f"BasicMinSum({FACTOR})", "T": T, "seed": SEED,
                       "snr_db": snr, "scan_set_partitioned_K1": scan, "legs": legs})
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
