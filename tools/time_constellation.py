#!/usr/bin/env python3
"""Time the constellation channel (ldpc_channel_con) and its demapper (ldpc_demap_con) under both rules, and the joint rule on
a QAM table next to the separable rule of the string scheme.

    python tools/time_constellation.py [--reps 20] [--out profiles/constellation_timing.jsonl]
Prints one JSON line and appends it to --out.  Device events around every repetition, two warm-up repetitions, the median of
--reps (at least 20) with the minimum and maximum beside it, the legs of a table timed alternately in the same run.
At [65536, 1998] and [4096, 16200], without fading at 6 dB, codeword rows and the received samples drawn once outside the
timing, output allocation included in every leg: engine.sym_llr and engine.demap of the stored samples, each with "maxlog" and
"exact", for Constellation.psk(8), 16-APSK 4 + 12, 32-APSK 4 + 12 + 16, and Constellation.from_modulation of "qam16" and "qam64"
with the same four legs of Modulation("qam16") / Modulation("qam64") beside them.  A repetition is 16 calls queued back to back
and its time divided by 16.  The joint search forms 2^m distances where the separable rule forms 2 * 2^(m/2): it is expected
to be slower, and this tool says by how much.  No threshold."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import torch  # noqa: E402

SHAPES = ((65536, "ira_1998_1512"), (4096, "dvbs2_like_16200_7200"))
SNR_DB = 6.0
WARMUP = 2
INNER = 16          # calls per timed repetition
LEGS = ("channel_maxlog", "channel_exact", "demap_maxlog", "demap_exact")


def tables():
    """(name, demapper -> Constellation, demapper -> Modulation or None)"""
    from modulation import Constellation, Modulation
    out = [("psk8", lambda dm: Constellation.psk(8, demapper=dm), None),
           ("apsk16_4+12", lambda dm: Constellation.apsk((4, 12), (1.0, 2.6), demapper=dm), None),
           ("apsk32_4+12+16", lambda dm: Constellation.apsk((4, 12, 16), (1.0, 2.64, 4.64), demapper=dm), None)]
    for scheme in ("qam16", "qam64"):
        out.append((scheme, lambda dm, s=scheme: Constellation.from_modulation(Modulation(s, demapper=dm)),
                    lambda dm, s=scheme: Modulation(s, demapper=dm)))
    return out


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def medians(fns, reps):
    """ms per repetition of each of `fns`, timed alternately: (median, min, max)"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(timed(fn))
    return [(statistics.median(v), min(v), max(v)) for v in ms]


def legs_of(make, batch, n, rows, kw):
    """the four legs of one modulation: closures over its own stored samples"""
    import engine
    ml, ex = make("maxlog"), make("exact")
    _, rec = engine.sym_llr(batch, n, modulation=ml, snr_db=SNR_DB, codeword=rows, want_received=True, **kw)

    def channel(mod):
        def run():
            for _ in range(INNER):
                engine.sym_llr(batch, n, modulation=mod, snr_db=SNR_DB, codeword=rows, **kw)
        return run

    def demap(rule):
        def run():
            for _ in range(INNER):
                engine.demap(rec, n, modulation=ml, demapper=rule)
        return run
    return [channel(ml), channel(ex), demap("maxlog"), demap("exact")]


def report(res, batch, n):
    legs = {}
    for key, (m, lo, hi) in zip(LEGS, res):
        legs[key] = {"ms": m, "ms_min_max": [lo, hi], "Gllr_per_s": batch * n / m / 1e6}
    legs["channel_exact_over_maxlog"] = res[1][0] / res[0][0]
    legs["demap_exact_over_maxlog"] = res[3][0] / res[2][0]
    return legs


def timing(reps, dev):
    import codes
    import engine
    out = []
    for batch, name in SHAPES:
        g = codes.load_graph(name)
        n = g.n
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        rows = engine.encode_random(codes.Encoder.from_graph(g), batch, **kw)
        row = {"shape": [batch, n], "snr_db": SNR_DB, "tables": {}}
        for label, table, string in tables():
            fns = legs_of(table, batch, n, rows, kw)
            if string is not None:
                fns += legs_of(string, batch, n, rows, kw)
            res = [tuple(v / INNER for v in m) for m in medians(fns, reps)]
            entry = {"bits_per_symbol": table("maxlog").bits_per_symbol, "table": report(res[:4], batch, n)}
            if string is not None:
                entry["string_scheme"] = report(res[4:], batch, n)
                entry["table_over_string"] = {key: res[k][0] / res[4 + k][0] for k, key in enumerate(LEGS)}
            row["tables"][label] = entry
            del fns
            torch.cuda.empty_cache()
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constellation_timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    line = json.dumps({"tool": "time_constellation", "reps": a.reps, "device": torch.cuda.get_device_name(dev),
                       "timing": timing(a.reps, dev)})
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
