#!/usr/bin/env python3
"""Throughput of the layered schedule of the min-sum decoders (layered_minsum_lds; schedule="layered") on the (1998,1512)
code at 65536 codewords, T = 10: normalised (BasicMinSumDecoder) and offset (Neural2DOffsetMinSumDecoder, check-side
alpha) form, beside layered_paper_lds (WeightedRCQDecoder(layered="paper"): the same walk with 1-byte codes) and the
flooding resident decode (BasicMinSumDecoder) at the same shape in the same run.  Each decoder is measured at fixed T
(3 dB: nothing stops) and once with early stop at 5 dB, where the mean iterations to decode are reported as well.
One JSON line per measurement.  --stream adds the HBM-streaming kernel (layered_minsum) at 4096 codewords."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import numpy as np  # noqa: E402
import torch  # noqa: E402
import codes  # noqa: E402
from ldpc_decoder import BasicMinSumDecoder  # noqa: E402
from neural_2d_decoder import Neural2DOffsetMinSumDecoder  # noqa: E402
from rcq_decoder import WeightedRCQDecoder  # noqa: E402
from simulation_framework import _engine_of  # noqa: E402

QP = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
dev = torch.device("cuda", 0)
T, B = 10, 65536


def timed(eng, llr, early_stop, reps=3):
    res = eng.decode(llr, early_stop=early_stop, want_posterior=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        eng.decode(llr, early_stop=early_stop, want_posterior=False)
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps, res


code = codes.load_code("ira_1998_1512", max_iterations=T)
rng = np.random.default_rng(0)
oms = Neural2DOffsetMinSumDecoder(code, 2, T, schedule="layered")
paper = WeightedRCQDecoder(code, 3, 8, QP, weight_sharing_type=2, max_iterations=T, layered="paper")
with torch.no_grad():
    for p in oms.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.1, 0.4))))
    for p in oms.alpha_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.0, 0.1))))
    for p in paper.beta_weights.values():
        p.fill_(float(np.float32(rng.uniform(0.6, 1.0))))
DECODERS = (('BasicMinSumDecoder(schedule="layered")', BasicMinSumDecoder(code, 0.7, schedule="layered")),
            ('Neural2DOffsetMinSumDecoder(schedule="layered")', oms),
            ('WeightedRCQDecoder(layered="paper")', paper),
            ("BasicMinSumDecoder (flooding)", BasicMinSumDecoder(code, 0.7)))
SHAPES = [("auto", B)] + ([("stream", 4096)] if "--stream" in sys.argv[1:] else [])
for mode, batch in SHAPES:
    fixed, stop = bench.make_llr(batch, code.n, 3.0, 1234, dev), bench.make_llr(batch, code.n, 5.0, 1234, dev)
    for label, dec in DECODERS:
        eng = _engine_of(dec, dev)
        eng.set_mode(mode)
        info = eng.info()
        for early_stop, llr, snr in ((False, fixed, 3.0), (True, stop, 5.0)):
            ms, res = timed(eng, llr, early_stop)
            out = {"decoder": label, "code": "ira_1998_1512", "B": batch, "T": T, "mode": mode, "kernel": info["kernel"],
                   "codewords_per_workgroup": info["codewords_per_workgroup"], "workgroups_per_cu": info["workgroups_per_cu"],
                   "early_stop": early_stop, "snr_db": snr, "decode_ms": round(ms, 3), "Mcw_s": round(batch / ms / 1e3, 3)}
            if early_stop:
                out["decoded"] = round(float(res.success.float().mean().item()), 4)
                out["mean_iterations"] = round(float(res.iterations.float().mean().item()), 3)
            print(json.dumps(out), flush=True)
