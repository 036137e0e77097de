#!/usr/bin/env python3
"""Time the demapper with a priori LLRs (ldpc_demap_con_prior) against the demapper without (ldpc_demap_con) on the same table,
samples and shape, under both rules.

    python tools/time_demap_prior.py [--reps 20] [--out profiles/demap_prior_timing.jsonl]
Prints one JSON line and appends it to --out.  Device events around every repetition, two warm-up repetitions, the median of
--reps (at least 20) with the minimum and maximum beside it, the four legs of a table timed alternately in the same run.
At [65536, 1998] and [4096, 16200], samples without fading at 6 dB drawn once outside the timing, every leg writing into the
same preallocated output: engine.demap(received, out=...) and engine.demap(received, prior=P, prior_sub=Q, out=...) with P and
Q normal (sigma 4), each with "maxlog" and "exact", for Constellation.psk(8), a set-partitioned 16-point grid and a 64-point
table.  A repetition is 16 calls queued back to back and its time divided by 16.  The prior form reads 8 more bytes per LLR
and adds one add per candidate for A_c and two operations for Lam_c: it is expected to be slower, and this tool says by how
much.  No threshold."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = ((65536, "ira_1998_1512"), (4096, "dvbs2_like_16200_7200"))
SNR_DB = 6.0
WARMUP = 2
INNER = 16          # calls per timed repetition
LEGS = ("plain_maxlog", "prior_maxlog", "plain_exact", "prior_exact")


def sp_grid16():
    """the set-partitioned 16-point grid of DESIGN.md 3n: b0 = (x + y) & 1, b1 = x & 1, b2 = ((x >> 1) + (y >> 1)) & 1, b3 = (x >> 1) & 1"""
    pts = np.empty(16, dtype=np.complex128)
    for x in range(4):
        for y in range(4):
            b = ((x + y) & 1, x & 1, ((x >> 1) + (y >> 1)) & 1, (x >> 1) & 1)
            pts[sum(v << k for k, v in enumerate(b))] = (2 * x - 3) + 1j * (2 * y - 3)
    return pts


def tables():
    from modulation import Constellation
    rng = np.random.default_rng(64)
    return [("psk8", Constellation.psk(8)), ("grid16_sp", Constellation(sp_grid16(), name="grid16sp")),
            ("rand64", Constellation(rng.normal(size=64) + 1j * rng.normal(size=64), name="rand64"))]


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


def timing(reps, dev):
    import codes
    import engine
    out = []
    for batch, name in SHAPES:
        g = codes.load_graph(name)
        n = g.n
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        rows = engine.encode_random(codes.Encoder.from_graph(g), batch, **kw)
        gen = torch.Generator(device=dev).manual_seed(5)
        P = 4.0 * torch.randn((batch, n), generator=gen, device=dev, dtype=torch.float32)
        Q = 4.0 * torch.randn((batch, n), generator=gen, device=dev, dtype=torch.float32)
        dst = torch.empty((batch, n), dtype=torch.float32, device=dev)
        row = {"shape": [batch, n], "snr_db": SNR_DB, "tables": {}}
        for label, con in tables():
            _, rec = engine.sym_llr(batch, n, modulation=con, snr_db=SNR_DB, codeword=rows, want_received=True, **kw)

            def leg(rule, prior):
                extra = dict(prior=P, prior_sub=Q) if prior else {}

                def run():
                    for _ in range(INNER):
                        engine.demap(rec, n, modulation=con, demapper=rule, out=dst, **extra)
                return run
            fns = [leg("maxlog", False), leg("maxlog", True), leg("exact", False), leg("exact", True)]
            res = [tuple(v / INNER for v in m) for m in medians(fns, reps)]
            entry = {"bits_per_symbol": con.bits_per_symbol}
            for key, (m, lo, hi) in zip(LEGS, res):
                entry[key] = {"ms": m, "ms_min_max": [lo, hi], "Gllr_per_s": batch * n / m / 1e6}
            entry["prior_over_plain_maxlog"] = res[1][0] / res[0][0]
            entry["prior_over_plain_exact"] = res[3][0] / res[2][0]
            row["tables"][label] = entry
            del fns, rec
            torch.cuda.empty_cache()
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "demap_prior_timing.jsonl"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    line = json.dumps({"tool": "time_demap_prior", "reps": a.reps, "device": torch.cuda.get_device_name(dev),
                       "timing": timing(a.reps, dev)})
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
