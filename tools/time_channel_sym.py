#!/usr/bin/env python3
"""Time the symbol channel (ldpc_channel_sym) per scheme next to the per-frame BI-AWGN channel (ldpc_channel_awgn_cw) of the
same build on the same codeword rows, and one resident Monte-Carlo point on random codewords under 16-QAM next to BPSK.

    python tools/time_channel_sym.py [--reps 20] [--only channel|simulate]
Prints one JSON line.  Device events around every repetition, two warm-up repetitions, the median of --reps (at least 20) with
the minimum and maximum beside it, the legs timed alternately.
  channel  : at [65536, 1998] and [4096, 16200], codeword rows drawn once outside the timing, 3 dB, output allocation included
             in every leg: engine.awgn_llr(codeword=rows) and, per scheme, engine.sym_llr with the identity interleaver and no
             fading, with Rayleigh fading, and with a random interleaver.  A repetition is 16 calls queued back to back and its
             time divided by 16: one call is 0.1 to 0.3 ms of device time, the same order as the host's work to launch it.
  simulate : DecodeEngine.simulate on (1998,1512), BasicMinSumDecoder(0.7) at T = 10 on the resident engine, 65536 frames in
             blocks of 16384, no error limit, codeword="random": 16-QAM at 11.5 dB, BPSK (modulation) at the SNR of a 0.25 dB
             grid whose mean iteration count over 4096 frames comes closest to 16-QAM's, and the BI-AWGN point
             (ldpc_simulate_enc) at that same SNR.  Both SNRs and both iteration counts are in the output."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CHANNEL_SHAPES = ((65536, "ira_1998_1512"), (4096, "dvbs2_like_16200_7200"))
SCHEMES = ("bpsk", "qpsk", "qam16", "qam64", "qam256")
POINT = ("ira_1998_1512", 10, 11.5, 65536, 16384)
BPSK_GRID = [4.5 + 0.25 * k for k in range(11)]
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


def channel(reps, dev):
    import codes
    import engine
    from modulation import Modulation
    scale, shift = engine.awgn_scale_shift(3.0)
    out = []
    for batch, name in CHANNEL_SHAPES:
        g = codes.load_graph(name)
        n = g.n
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        rows = engine.encode_random(codes.Encoder.from_graph(g), batch, **kw)
        pos = np.random.default_rng(n).permutation(n)
        names, fns = ["awgn_cw"], []

        def awgn():
            for _ in range(INNER):
                engine.awgn_llr(batch, n, scale=scale, shift=shift, codeword=rows, **kw)
        fns.append(awgn)

        def leg(mod):
            mod.native(1.0, n, dev)                                     # the interleaver is uploaded once, outside the timing

            def run():
                for _ in range(INNER):
                    engine.sym_llr(batch, n, modulation=mod, snr_db=3.0, codeword=rows, **kw)
            return run
        for scheme in SCHEMES:
            for tag, mod in (("", Modulation(scheme)), ("_rayleigh", Modulation(scheme, "rayleigh")),
                             ("_interleaved", Modulation(scheme, None, pos))):
                names.append(scheme + tag)
                fns.append(leg(mod))
        res = [tuple(v / INNER for v in m) for m in medians(fns, reps)]
        row = {"shape": [batch, n], "legs": {}}
        for key, (m, lo, hi) in zip(names, res):
            row["legs"][key] = {"ms": m, "ms_min_max": [lo, hi], "over_awgn_cw": m / res[0][0],
                                "Gllr_per_s": batch * n / m / 1e6}
        out.append(row)
        torch.cuda.empty_cache()
    return out


def simulate(reps, dev):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from modulation import Modulation
    from simulation_framework import _engine_of
    name, T, snr16, frames, block = POINT
    code = codes.load_code(name, max_iterations=T)
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), dev)
    assert eng.info()["engine"] == "resident"
    base = dict(seed=1234, stream_id=7, codeword="random", max_errors=10 ** 12, block=block, poll_blocks=4)
    q16, bpsk = Modulation("qam16"), Modulation("bpsk")
    its = lambda mod, snr: eng.simulate(modulation=mod, snr_db=snr, max_frames=4096, **base)["iterations"] / 4096
    target = its(q16, snr16)
    snr1 = min(BPSK_GRID, key=lambda s: abs(its(bpsk, s) - target))
    last = {}

    def point(key, **kw):
        def run():
            last[key] = eng.simulate(max_frames=frames, **base, **kw)
        return run
    legs = (("qam16", dict(modulation=q16, snr_db=snr16)), ("bpsk", dict(modulation=bpsk, snr_db=snr1)),
            ("bi_awgn", dict(snr_db=snr1)))
    res = medians([point(k, **kw) for k, kw in legs], reps)
    row = {"workload": f"{name} BasicMinSum 0.7, T={T}, {frames} frames in blocks of {block}, random codewords, resident engine"}
    for (key, kw), (m, lo, hi) in zip(legs, res):
        row[key] = {"snr_db": kw["snr_db"], "ms": m, "ms_min_max": [lo, hi], "frames_per_s": frames / m * 1e3,
                    "frame_errors": last[key]["frame_errors"], "iterations_per_frame": last[key]["iterations"] / frames}
    row["qam16_over_bpsk"] = res[0][0] / res[1][0]
    return [row]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("channel", "simulate"), default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "time_channel_sym", "reps": a.reps}
    if a.only != "simulate":
        res["channel"] = channel(a.reps, dev)
    if a.only != "channel":
        res["simulate"] = simulate(a.reps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
