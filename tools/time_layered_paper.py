#!/usr/bin/env python3
"""Throughput of the paper's layered RCQ schedule at T = 10: RCQMinSumDecoder(layered="paper") and
WeightedRCQDecoder(layered="paper") on the HBM-streaming kernel (layered_rcq<VEC, true>, engine mode "stream") and the
LDS-resident one (layered_paper_lds, "auto"); (1998,1512) at 4096 and 65536 codewords, (16200,7200) at 32768.
One JSON line per measurement (decode ms, M codewords/s; fixed T, no early stop).  --quick: (1998,1512) at 65536 on the
LDS kernel only (the kernel-trace run)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import codes  # noqa: E402
from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder  # noqa: E402

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
dev = torch.device("cuda", 0)


def timed(eng, llr, reps):
    eng.decode(llr, early_stop=False, want_posterior=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        eng.decode(llr, early_stop=False, want_posterior=False)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


QUICK = "--quick" in sys.argv[1:]
CASES = (("ira_1998_1512", 65536),) if QUICK else \
    (("ira_1998_1512", 4096), ("ira_1998_1512", 65536), ("dvbs2_like_16200_7200", 32768))
for name, B in CASES:
    code = codes.load_code(name, max_iterations=10)
    llr = bench.make_llr(B, code.n, 3.0, 1234, dev)
    w = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=10, layered="paper")
    rng = np.random.default_rng(0)
    with torch.no_grad():
        for p in w.beta_weights.values():
            p.fill_(float(np.float32(rng.uniform(0.6, 1.0))))
    u = RCQMinSumDecoder(code, 3, 8, QP, max_iterations=10, layered="paper")
    for label, dec in (("RCQMinSumDecoder", u), ("WeightedRCQDecoder", w)):
        for mode in (("auto",) if QUICK else ("stream", "auto")):
            eng = dec._get_engine(dev)
            eng.set_mode(mode)
            ms = timed(eng, llr, 3)
            info = eng.info()
            print(json.dumps({"decoder": f'{label}(layered="paper")', "code": name, "B": B, "T": 10, "mode": mode,
                              "kernel": info["kernel"], "codewords_per_workgroup": info["codewords_per_workgroup"],
                              "decode_ms": round(ms, 3), "Mcw_s": round(B / ms / 1e3, 3)}), flush=True)
