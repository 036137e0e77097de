#!/usr/bin/env python3
"""Time the sum-product decoder next to normalised min-sum on the streaming engine (both in mode "sweeps": the two-sweep
form, the only one the sum-product form has): the check sweep alone (ldpc_debug_sweep, iteration 1) and a whole fixed-T
decode, on ira_1998_1512 and dvbs2_like_16200_7200.  Device events around work that ends in a synchronise; every shape is
warmed up; every timed sample repeats its call until it covers about `--window-ms` of device time (the repetitions are
calibrated per call from a warm run, so a 0.5 ms sweep is not timed over a few milliseconds); the two decoders alternate
inside each of `--rounds` rounds and the spread over the rounds is reported, so a difference can be read against the noise.  One JSON line per code, appended to profiles/sum_product_timing.jsonl.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (puts the package on sys.path)
import torch  # noqa: E402

CODES = {"ira_1998_1512": (10, 65536), "dvbs2_like_16200_7200": (20, 8192)}     # name -> (T, default batch)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--codes", nargs="*", default=list(CODES))
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0, help="device time one timed sample should cover")
    ap.add_argument("--snr-db", type=float, default=2.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_product_timing.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sum_product.py needs a GPU")
    import codes
    from ldpc_decoder import BasicMinSumDecoder, SumProductDecoder
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    for name in a.codes:
        T, B0 = CODES[name]
        B = a.batch or B0
        code = codes.load_code(name, max_iterations=T)
        g = code.tanner_graph()
        llr = bench.make_llr(B, code.n, a.snr_db, 1234, dev)
        engs = {"spa": SumProductDecoder(code)._get_engine(dev),
                "nms": BasicMinSumDecoder(code, 0.7)._engine(torch.float32, dev).set_mode("sweeps")}
        for eng in engs.values():
            assert eng.info()["kernel"] == "sweeps", eng.info()
        decode = {k: (lambda e=e: e.decode(llr, early_stop=False, want_posterior=False)) for k, e in engs.items()}
        sweep = {k: (lambda e=e: e.debug_sweep(B, 0, 1)) for k, e in engs.items()}
        samples = {f"{k}_{what}": [] for k in engs for what in ("decode_ms", "cn_ms")}
        for k in engs:                                   # warm-up: every kernel of every timed shape
            decode[k]()
            sweep[k]()
        torch.cuda.synchronize()
        reps = {}
        for k in engs:                                   # repetitions per sample: enough calls to fill the window
            reps[k, "decode"] = max(3, int(a.window_ms / timed(decode[k], 2)) + 1)
            reps[k, "cn"] = max(3, int(a.window_ms / timed(sweep[k], 5)) + 1)
        for _ in range(a.rounds):
            for k in engs:                               # alternate the two decoders inside a round
                samples[f"{k}_decode_ms"].append(timed(decode[k], reps[k, "decode"]))
                samples[f"{k}_cn_ms"].append(timed(sweep[k], reps[k, "cn"]))   # on the state the decode above left
        out = {"code": name, "n": g.n, "E": g.E, "max_dc": int(g.max_dc), "T": T, "B": B, "snr_db": a.snr_db, "rounds": a.rounds,
               "window_ms": a.window_ms, "reps": {f"{k}_{what}": v for (k, what), v in reps.items()},
               "build": os.path.basename(os.environ.get("LDPC_HIP_LIB", "shipped")), "transcendentals": "expf/log1pf (accurate)", "device": torch.cuda.get_device_name(dev)}
        for key, v in samples.items():
            v = sorted(v)
            out[key] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
        for what in ("decode_ms", "cn_ms"):
            out[f"spa_over_nms_{what[:-3]}"] = out[f"spa_{what}"]["median"] / out[f"nms_{what}"]["median"]
        # per check of degree dc the recursions form 3 (dc - 2) box-plus, 2 exp + 2 log1p each
        boxplus = 3 * int((g.dc.astype("int64") - 2).clip(min=0).sum()) * B
        out["spa_boxplus_per_ns"] = boxplus / (out["spa_cn_ms"]["median"] * 1e6)
        out["spa_cn_GBs"] = 20 * g.E * B / out["spa_cn_ms"]["median"] / 1e6     # 2 reads of the input, park + re-read, 1 write
        out["nms_cn_GBs"] = 8 * g.E * B / out["nms_cn_ms"]["median"] / 1e6
        print(json.dumps(out))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
