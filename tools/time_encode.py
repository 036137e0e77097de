#!/usr/bin/env python3
"""Time the device encoder and the per-frame channel next to the one-codeword channel of the same build, and one resident
Monte-Carlo point on random codewords next to the same point on one fixed nonzero codeword.

    python tools/time_encode.py [--reps 20] [--only channel|simulate]
Prints one JSON line.  Device events around every repetition, two warm-up repetitions, the median of --reps (at least 20),
the legs timed alternately.
  channel  : engine.encode_random + engine.awgn_llr(codeword=rows) against engine.awgn_llr(codeword=one shared word) at 3 dB,
             at [65536, 1998] and [4096, 16200], output allocation included in both; encode_random alone as a third leg.  A
             repetition is 16 calls queued back to back and its time divided by 16: one call is 0.1 to 0.2 ms of device time,
             the same order as the host's work to launch it.
  simulate : DecodeEngine.simulate on (1998,1512), BasicMinSumDecoder(0.7) at T = 10 on the resident engine, 65536 frames in
             blocks of 16384, no error limit, at 3 dB (no frame converges) and at 5.5 dB (early stop): codeword="random"
             (ldpc_simulate_enc) against one fixed staircase-encoded codeword (ldpc_simulate).  The frames differ in their
             codewords, so the decisions are not the same frames': a like-for-like figure only as far as the decoder's work
             does not depend on the codeword."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CHANNEL_SHAPES = ((65536, "ira_1998_1512"), (4096, "dvbs2_like_16200_7200"))
POINT = ("ira_1998_1512", 10, (3.0, 5.5), 65536, 16384)
WARMUP = 2
INNER = 16          # calls per timed repetition


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


def fixed_codeword(graph):
    import codes
    c = codes.staircase_encode(graph, np.random.default_rng(graph.n).integers(0, 2, graph.n - graph.m))
    assert c.any()
    return c


def channel(reps, dev):
    import codes
    import engine
    scale, shift = engine.awgn_scale_shift(3.0)
    out = []
    for batch, name in CHANNEL_SHAPES:
        g = codes.load_graph(name)
        enc = codes.Encoder.from_graph(g)
        n = g.n
        one = engine.pack_codeword(fixed_codeword(g), n, dev)
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        engine.encode_random(enc, 1, **kw)                              # the encoder is uploaded once, outside the timing

        def rows():
            for _ in range(INNER):
                engine.awgn_llr(batch, n, scale=scale, shift=shift, codeword=engine.encode_random(enc, batch, **kw), **kw)

        def shared():
            for _ in range(INNER):
                engine.awgn_llr(batch, n, scale=scale, shift=shift, codeword=one, **kw)

        def encode_only():
            for _ in range(INNER):
                engine.encode_random(enc, batch, **kw)
        (r, r_lo, r_hi), (s, s_lo, s_hi), (e, e_lo, e_hi) = [tuple(v / INNER for v in m) for m in
                                                             medians([rows, shared, encode_only], reps)]
        out.append({"shape": [batch, n], "encoder_entries": int(enc.info_idx.size), "rows_ms": r, "rows_ms_min_max": [r_lo, r_hi],
                    "shared_ms": s, "shared_ms_min_max": [s_lo, s_hi], "encode_ms": e, "encode_ms_min_max": [e_lo, e_hi],
                    "rows_over_shared": r / s, "encode_Gbits_per_s": batch * n / e / 1e6})
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
    fixed = fixed_codeword(eng.graph)
    out = []
    for snr_db in snrs:
        kw = dict(seed=1234, stream_id=int(round(snr_db * 1000)), snr_db=snr_db, max_frames=frames, max_errors=10 ** 12,
                  block=block, poll_blocks=4)
        last = {}

        def point(key, cw):
            def run():
                last[key] = eng.simulate(codeword=cw, **kw)
            return run
        res = medians([point("random", "random"), point("fixed", fixed)], reps)
        row = {"workload": f"{name} BasicMinSum 0.7, T={T}, {snr_db} dB, {frames} frames in blocks of {block}, resident engine"}
        for key, (m, lo, hi) in zip(("random", "fixed"), res):
            row[key] = {"ms": m, "ms_min_max": [lo, hi], "frames_per_s": frames / m * 1e3, "frame_errors": last[key]["frame_errors"],
                        "iterations_per_frame": last[key]["iterations"] / frames}
        row["random_over_fixed"] = res[0][0] / res[1][0]
        out.append(row)
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
    res = {"tool": "time_encode", "reps": a.reps}
    if a.only != "simulate":
        res["channel"] = channel(a.reps, dev)
    if a.only != "channel":
        res["simulate"] = simulate(a.reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
