#!/usr/bin/env python3
"""Throughput of the block-parallel layered decode (layered_block_lds, LDPC_ENGINE_MODE=block) against the sequential
LDS kernels (`resident`: layered_minsum_lds / layered_paper_lds, the lanes on the edges of one check) on the same graph,
with the streaming walk and the flooding resident decode of the same code beside them.

Leg 1: qc_1944_972 and layered_order(ira_1998_1512), 65536 codewords, T = 10; normalised min-sum and W-RCQ type 2; fixed
T (low SNR: nothing stops) and early stop at an SNR where nearly every frame decodes (the decoded fraction is reported).
Leg 2: the base matrix of qc_1944_972 lifted at Z in {1, 2, 4, 8, 16, 32, 81} (shifts mod Z), normalised min-sum, fixed T:
block against resident -- the smallest Z at which block wins by more than the spread is what the AUTO rule may use.

Device events, one warm-up decode per variant and shape, then five ALTERNATING repetitions per variant in one process;
median, min and max are reported, and whether the timed batch's outputs (packed decisions, iterations, success) equal
the resident variant's.  One JSON line per measurement, also appended to profiles/block_layered_timing.jsonl.
Fails without a GPU."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import codes  # noqa: E402
from ldpc_decoder import BasicMinSumDecoder, LDPCCode  # noqa: E402
from rcq_decoder import WeightedRCQDecoder  # noqa: E402
from simulation_framework import _engine_of  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("time_block_layered.py needs a GPU")
QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
dev = torch.device("cuda", 0)
T, B, B_STREAM, REPS = 10, 65536, 8192, 5
OUT = os.path.join(ROOT, "profiles", "block_layered_timing.jsonl")
os.makedirs(os.path.dirname(OUT), exist_ok=True)
sink = open(OUT, "w")


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    sink.write(line + "\n")
    sink.flush()


def one(eng, llr, early_stop):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = eng.decode(llr, early_stop=early_stop, want_bits=False, want_posterior=False, want_packed=True)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1), res


def measure(variants, early_stop):
    """variants: [(label, engine, llr)] -> {label: (times, last result)}; one warm-up each, then REPS alternating rounds"""
    out = {label: ([], None) for label, _, _ in variants}
    for label, eng, llr in variants:
        one(eng, llr, early_stop)
    for _ in range(REPS):
        for label, eng, llr in variants:
            ms, res = one(eng, llr, early_stop)
            out[label][0].append(ms)
            out[label] = (out[label][0], res)
    return out


def same(a, b):
    return bool(torch.equal(a.packed_bits, b.packed_bits) and torch.equal(a.iterations, b.iterations) and
                torch.equal(a.success, b.success))


def engine(dec, mode):
    """a decoder's engine under `mode`, or None where the code has no such form"""
    eng = _engine_of(dec, dev)
    try:
        return eng.set_mode(mode)
    except NotImplementedError:
        return None


def nms(code, layered=True):
    return BasicMinSumDecoder(code, 0.7, **({"schedule": "layered"} if layered else {}))


def wrcq(code):
    dec = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=T, layered="paper")
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for p in dec.beta_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.8, 1.1))))
    return dec


def report(base, times, info, batch, res, early_stop, equal):
    t = sorted(times)
    rec = dict(base, kernel=info["kernel"], codewords_per_workgroup=info["codewords_per_workgroup"],
               threads_per_workgroup=info["threads_per_workgroup"], lds_bytes=info["lds_bytes"],
               workgroups_per_cu=info["workgroups_per_cu"], B=batch, T=T, early_stop=early_stop,
               decode_ms_median=round(t[len(t) // 2], 3), decode_ms_min=round(t[0], 3), decode_ms_max=round(t[-1], 3),
               Mcw_s=round(batch / t[len(t) // 2] / 1e3, 3), outputs_equal_resident=equal)
    if early_stop:
        rec["decoded"] = round(float(res.success.float().mean().item()), 4)
        rec["mean_iterations"] = round(float(res.iterations.float().mean().item()), 3)
    emit(rec)


# ---- leg 1 -----------------------------------------------------------------------------------------------------------------
g_qc = codes.load_graph("qc_1944_972")
g_ira = codes.layered_order(codes.load_graph("ira_1998_1512"))[0]
LEG1 = (("qc_1944_972", g_qc, 1.0, 3.5), ("layered_order(ira_1998_1512)", g_ira, 3.0, 5.5))
for code_name, g, snr_fixed, snr_stop in LEG1:
    code = LDPCCode.from_graph(g, k=g.n - g.m, max_iterations=T)
    for dec_name, make in (("NMS", nms), ("W-RCQ type 2", wrcq)):
        # one decoder object per mode: each keeps its own engine
        decs = {mode: make(code) for mode in ("block", "resident", "stream")}
        engs = {mode: engine(d, mode) for mode, d in decs.items()}
        flood = _engine_of(nms(code, layered=False), dev) if dec_name == "NMS" else None
        for early_stop, snr in ((False, snr_fixed), (True, snr_stop)):
            llr, llr_s = bench.make_llr(B, g.n, snr, 1234, dev), bench.make_llr(B_STREAM, g.n, snr, 1234, dev)
            variants = [(m, engs[m], llr_s if m == "stream" else llr) for m in ("block", "resident", "stream") if engs[m] is not None]
            if flood is not None:
                variants.append(("flooding-resident", flood, llr))
            got = measure(variants, early_stop)
            for label, eng, x in variants:
                times, res = got[label]
                equal = None
                if label == "block" and "resident" in got:
                    equal = same(res, got["resident"][1])
                report({"leg": 1, "code": code_name, "decoder": dec_name, "mode": label, "snr_db": snr, "layers": g.n_layers,
                        "mean_layer": round(g.m / g.n_layers, 2)}, times, eng.info(), x.shape[0], res, early_stop, equal)

# ---- leg 2: one base matrix, lifted ---------------------------------------------------------------------------------------------
Z0, mb, nb = 81, 12, 24
S0 = np.full((mb, nb), -1, dtype=np.int64)
for r in range(mb):
    i = r * Z0                                                   # row z = 0 of the block row: column (0 + s) mod Z0 of each block
    for v in g_qc.var_idx[g_qc.check_ptr[i]:g_qc.check_ptr[i + 1]]:
        S0[r, int(v) // Z0] = int(v) % Z0
for Z in (1, 2, 4, 8, 16, 32, 81):
    g = codes.quasi_cyclic(np.where(S0 >= 0, S0 % Z, -1), Z)
    code = LDPCCode.from_graph(g, k=g.n - g.m, max_iterations=T)
    decs = {mode: nms(code) for mode in ("block", "resident")}
    engs = {mode: engine(d, mode) for mode, d in decs.items()}
    llr = bench.make_llr(B, g.n, 1.0, 4321, dev)
    variants = [(m, engs[m], llr) for m in ("block", "resident") if engs[m] is not None]
    got = measure(variants, False)
    for label, eng, x in variants:
        times, res = got[label]
        equal = same(res, got["resident"][1]) if label == "block" and "resident" in got else None
        report({"leg": 2, "code": f"qc base 12x24 lifted at Z={Z}", "decoder": "NMS", "mode": label, "snr_db": 1.0, "Z": Z,
                "layers": g.n_layers, "mean_layer": float(Z)}, times, eng.info(), B, res, False, equal)
sink.close()
