#!/usr/bin/env python3
"""Time the device soft demapper (ldpc_demap_sym) next to the symbol channel (ldpc_channel_sym) and the channel's exact rule
(ldpc_channel_sym_dm) next to its max-log rule, and count frame errors of one Monte-Carlo point under both rules.

    python tools/time_demap.py [--reps 20] [--only timing|fer]
Prints one JSON line.  Device events around every repetition, two warm-up repetitions, the median of --reps (at least 20) with
the minimum and maximum beside it, the legs timed alternately.
  timing : at [65536, 1998] and [4096, 16200], for 16-, 64- and 256-QAM without fading at 3 dB, codeword rows and the received
           samples drawn once outside the timing, output allocation included in every leg: engine.sym_llr (max-log, the
           channel), engine.sym_llr with demapper="exact", engine.demap of the stored samples with "maxlog" and with "exact".
           A repetition is 16 calls queued back to back and its time divided by 16.
  fer    : DecodeEngine.simulate on (1998,1512), BasicMinSumDecoder(0.7) at T = 10, codeword="random", one seed: 64-QAM at
           17.0 dB and 256-QAM at 22.5 dB, 65536 frames each, no error limit, under max-log and under exact.  Counts, no gate."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import torch  # noqa: E402

SHAPES = ((65536, "ira_1998_1512"), (4096, "dvbs2_like_16200_7200"))
SCHEMES = ("qam16", "qam64", "qam256")
FER_POINTS = (("qam64", 17.0), ("qam256", 22.5))
FER_FRAMES, FER_BLOCK = 65536, 16384
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


def timing(reps, dev):
    import codes
    import engine
    from modulation import Modulation
    out = []
    for batch, name in SHAPES:
        g = codes.load_graph(name)
        n = g.n
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        rows = engine.encode_random(codes.Encoder.from_graph(g), batch, **kw)
        row = {"shape": [batch, n], "schemes": {}}
        for scheme in SCHEMES:
            ml, ex = Modulation(scheme), Modulation(scheme, demapper="exact")
            _, rec = engine.sym_llr(batch, n, modulation=ml, snr_db=3.0, codeword=rows, want_received=True, **kw)

            def channel(mod):
                def run():
                    for _ in range(INNER):
                        engine.sym_llr(batch, n, modulation=mod, snr_db=3.0, codeword=rows, **kw)
                return run

            def demap(rule):
                def run():
                    for _ in range(INNER):
                        engine.demap(rec, n, modulation=ml, demapper=rule)
                return run
            names = ("channel_maxlog", "channel_exact", "demap_maxlog", "demap_exact")
            res = [tuple(v / INNER for v in m) for m in medians([channel(ml), channel(ex), demap("maxlog"), demap("exact")], reps)]
            legs = {}
            for key, (m, lo, hi) in zip(names, res):
                legs[key] = {"ms": m, "ms_min_max": [lo, hi], "Gllr_per_s": batch * n / m / 1e6}
            legs["channel_exact_over_maxlog"] = res[1][0] / res[0][0]
            legs["demap_maxlog_over_channel_maxlog"] = res[2][0] / res[0][0]
            legs["demap_exact_over_demap_maxlog"] = res[3][0] / res[2][0]
            row["schemes"][scheme] = legs
            del rec
            torch.cuda.empty_cache()
        out.append(row)
    return out


def fer(dev):
    import codes
    from ldpc_decoder import BasicMinSumDecoder
    from modulation import Modulation
    from simulation_framework import _engine_of
    code = codes.load_code("ira_1998_1512", max_iterations=10)
    eng = _engine_of(BasicMinSumDecoder(code, 0.7), dev)
    base = dict(seed=1234, stream_id=7, codeword="random", max_frames=FER_FRAMES, max_errors=10 ** 12, block=FER_BLOCK,
                poll_blocks=4)
    out = []
    for scheme, snr in FER_POINTS:
        row = {"code": "ira_1998_1512", "decoder": "BasicMinSum 0.7, T=10", "scheme": scheme, "snr_db": snr, "seed": base["seed"],
               "engine": eng.info()["engine"]}
        for rule in ("maxlog", "exact"):
            r = eng.simulate(modulation=Modulation(scheme, demapper=rule), snr_db=snr, **base)
            row[rule] = {k: r[k] for k in ("frames", "frame_errors", "bit_errors", "iterations")}
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=("timing", "fer"), default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "time_demap", "reps": a.reps}
    if a.only != "fer":
        res["timing"] = timing(a.reps, dev)
    if a.only != "timing":
        res["fer"] = fer(dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
