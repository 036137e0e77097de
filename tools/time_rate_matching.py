#!/usr/bin/env python3
"""Time the rate-matched channel kernel next to the plain one of the same build, and one resident Monte-Carlo point with a
profile next to the plain point.

    python tools/time_rate_matching.py [--reps 20] [--only channel|simulate]
Prints one JSON line.  Device events around every repetition, two warm-up repetitions, the median of --reps (at least 20).
  channel  : engine.awgn_llr(rate_matching=...) against engine.awgn_llr at 3 dB, at [65536, 1998] and [4096, 16200], timed
             alternately, output allocation included in both.  A repetition is 16 calls queued back to back and its time
             divided by 16: one call is 0.1 to 0.2 ms of device time, the same order as the host's work to launch it, and a
             single call between two events would time the host.  Profiles: empty (every mask NULL: what the mask plumbing
             costs), 10 % of the bits punctured, scattered at random (no quad is skipped to speak of), and one contiguous
             punctured block of 25 % (whole waves skip the Philox rounds and both Box-Muller pairs).
  simulate : DecodeEngine.simulate on (1998,1512), BasicMinSumDecoder(0.7) at T = 10 on the resident engine, 65536 frames in
             blocks of 16384, no error limit, at 3 dB (no frame converges: every frame costs all T iterations) and at 5.5 dB
             (early stop: the channel's share of the point is larger): ldpc_simulate against ldpc_simulate_rm with the empty
             profile (the same frames and decisions, so the difference is the channel kernel's) and with 10 % of the
             information bits punctured (the decode then works on other LLRs: not a like-for-like figure)."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CHANNEL_SHAPES = ((65536, 1998), (4096, 16200))
POINT = ("ira_1998_1512", 10, (3.0, 5.5), 65536, 16384)
WARMUP = 2
INNER = 16          # channel calls per timed repetition


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def medians(fns, reps):
    """ms per call of each of `fns`, timed alternately: (median, min, max)"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(timed(fn))
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def profiles(n, limit=None):
    """the three profiles over the first `limit` bits (all n by default)"""
    from rate_matching import RateMatching
    limit = n if limit is None else limit
    rng = np.random.default_rng(n)
    return {"empty": RateMatching(n),
            "punctured_10pct_scattered": RateMatching(n, punctured=np.sort(rng.permutation(limit)[:limit // 10])),
            "punctured_25pct_block": RateMatching(n, punctured=np.arange(limit // 4))}


def channel(reps, dev):
    import engine
    scale, shift = engine.awgn_scale_shift(3.0)
    out = []
    for batch, n in CHANNEL_SHAPES:
        kw = dict(seed=1234, stream_id=0, first_frame=0, scale=scale, shift=shift, device=dev)
        for name, rm in profiles(n).items():
            rm.packed(dev)                                               # the masks are uploaded once, outside the timing
            def many(**extra):
                def run():
                    for _ in range(INNER):
                        engine.awgn_llr(batch, n, **extra, **kw)
                return run
            (m, m_lo, m_hi), (p, p_lo, p_hi) = [tuple(v / INNER for v in r) for r in medians([many(rate_matching=rm), many()], reps)]
            out.append({"shape": [batch, n], "profile": name, "punctured": rm.n_punctured, "rm_ms": m, "rm_ms_min_max": [m_lo, m_hi],
                        "plain_ms": p, "plain_ms_min_max": [p_lo, p_hi], "rm_over_plain": m / p,
                        "rm_Gsamples_per_s": batch * n / m / 1e6, "plain_Gsamples_per_s": batch * n / p / 1e6})
        torch.cuda.empty_cache()
    return out


def simulate(reps, dev):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from simulation_framework import _engine_of
    name, T, snrs, frames, block = POINT
    code = codes.load_code(name, max_iterations=T)
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), dev)
    assert eng.info()["engine"] == "resident"
    return [simulate_point(eng, code, snr_db, reps) for snr_db in snrs]


def simulate_point(eng, code, snr_db, reps):
    name, T, _, frames, block = POINT
    kw = dict(seed=1234, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, max_frames=frames, max_errors=10 ** 12, block=block,
              poll_blocks=4)
    rms = profiles(code.n, code.n - eng.graph.m)
    del rms["punctured_25pct_block"]
    last = {}

    def point(key, rm):
        def run():
            last[key] = eng.simulate(rate_matching=rm, **kw)
        return run
    keys = ["plain"] + list(rms)
    res = medians([point("plain", None)] + [point(k, rm) for k, rm in rms.items()], reps)
    assert {k: last["empty"][k] for k in ("frames", "frame_errors", "bit_errors", "iterations")} == \
        {k: last["plain"][k] for k in ("frames", "frame_errors", "bit_errors", "iterations")}
    out = {"workload": f"{name} BasicMinSum 0.7, T={T}, {snr_db} dB, {frames} frames in blocks of {block}, resident engine"}
    for key, (m, lo, hi) in zip(keys, res):
        out[key] = {"ms": m, "ms_min_max": [lo, hi], "frames_per_s": frames / m * 1e3, "over_plain": m / res[0][0],
                    "frame_errors": last[key]["frame_errors"], "iterations_per_frame": last[key]["iterations"] / frames}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("channel", "simulate"), default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "time_rate_matching", "reps": a.reps}
    if a.only != "simulate":
        res["channel"] = channel(a.reps, dev)
    if a.only != "channel":
        res["simulate"] = simulate(a.reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
