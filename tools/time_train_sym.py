#!/usr/bin/env python3
"""Time the mixed-SNR symbol channel (ldpc_channel_sym_mix) next to the one-point kernel (ldpc_channel_sym) of the same build
on the same codeword rows, and stream training on 16-QAM with random codewords next to stream training on BI-AWGN.

    python tools/time_train_sym.py [--reps 20] [--steps 8] [--only channel|train]
Prints one JSON line.  Device events around every repetition, two warm-up repetitions, the median of --reps (at least 20) with
the minimum and maximum beside it, the legs timed alternately.
  channel : at [65536, 1998] and [4096, 16200], codeword rows drawn once outside the timing, output allocation included in
            every leg; for 16-QAM with the identity interleaver and no fading, with Rayleigh fading, and with a random
            interleaver: engine.sym_llr at 10 dB, engine.sym_llr_mix on the 13-point table of 7 .. 13 dB in steps of 0.5 (on
            the device already, as train_stream holds it), and the same with want_targets.  A repetition is 16 calls queued
            back to back and its time divided by 16, as in tools/time_channel_sym.py.
  train   : PosteriorJointTrainer.train_stream on (1998,1512), Neural-2D type 2 at T = 10 under the joint loss with batch
            4096, one epoch of --steps steps per repetition, no validation: the BI-AWGN stream on snr_range (0, 6), step 0.5,
            against 16-QAM (no fading) with codeword="random" on snr_range (7, 13), step 0.5 -- 13 points each.  The 16-QAM
            leg pays the encoder launch and the targets on top of the draw.  The output also holds the first and the last
            epoch's training loss of both trainers over all (reps + 2) * steps steps at learning rate 1e-3: what this
            training does is a measurement, no test asserts it."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

CHANNEL_SHAPES = ((65536, "ira_1998_1512"), (4096, "dvbs2_like_16200_7200"))
TRAIN = ("ira_1998_1512", 10, 4096)
SYM_RANGE, AWGN_RANGE, STEP = (7.0, 13.0), (0.0, 6.0), 0.5
WARMUP = 2
INNER = 16          # calls per timed repetition of the channel legs


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
    grid = engine.snr_grid(SYM_RANGE, STEP)
    out = []
    for batch, name in CHANNEL_SHAPES:
        g = codes.load_graph(name)
        n = g.n
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        rows = engine.encode_random(codes.Encoder.from_graph(g), batch, **kw)
        pos = np.random.default_rng(n).permutation(n)
        names, fns = [], []

        def legs(mod):
            mod.native(1.0, n, dev)                                     # the interleaver is uploaded once, outside the timing
            tab = torch.from_numpy(mod.amp_table(grid)).to(dev)

            def one():
                for _ in range(INNER):
                    engine.sym_llr(batch, n, modulation=mod, snr_db=10.0, codeword=rows, **kw)

            def mix():
                for _ in range(INNER):
                    engine.sym_llr_mix(batch, n, modulation=mod, amp=tab, codeword=rows, **kw)

            def mix_targets():
                for _ in range(INNER):
                    engine.sym_llr_mix(batch, n, modulation=mod, amp=tab, codeword=rows, want_targets=True, **kw)
            return one, mix, mix_targets
        for tag, mod in (("qam16", Modulation("qam16")), ("qam16_rayleigh", Modulation("qam16", "rayleigh")),
                         ("qam16_interleaved", Modulation("qam16", None, pos))):
            names.append(tag)
            fns.extend(legs(mod))
        res = [tuple(v / INNER for v in m) for m in medians(fns, reps)]
        row = {"shape": [batch, n], "points": len(grid), "legs": {}}
        for k, key in enumerate(names):
            one, mix, mixt = res[3 * k:3 * k + 3]
            row["legs"][key] = {"one_point_ms": one[0], "one_point_ms_min_max": list(one[1:]),
                                "mix_ms": mix[0], "mix_ms_min_max": list(mix[1:]),
                                "mix_targets_ms": mixt[0], "mix_targets_ms_min_max": list(mixt[1:]),
                                "mix_over_one_point": mix[0] / one[0], "mix_targets_over_one_point": mixt[0] / one[0],
                                "one_point_Gllr_per_s": batch * n / one[0] / 1e6, "mix_Gllr_per_s": batch * n / mix[0] / 1e6,
                                "mix_targets_GB_written_per_s": 2 * 4 * batch * n / mixt[0] / 1e6}
        out.append(row)
        torch.cuda.empty_cache()
    return out


def train(reps, steps, dev):
    import codes
    from modulation import Modulation
    from neural_2d_decoder import Neural2DMinSumDecoder
    from training_framework import PosteriorJointTrainer, TrainingConfig
    name, T, B = TRAIN
    code = codes.load_code(name, max_iterations=T)

    def trainer(snr_range, **kw):
        model = Neural2DMinSumDecoder(code, 2, T)
        with torch.no_grad():
            for p in model.beta_weights.values():
                p.fill_(0.7)
            for p in model.alpha_weights.values():
                p.fill_(1.0)
        cfg = TrainingConfig(batch_size=B, num_epochs=1, learning_rate=1e-3, snr_range=snr_range, snr_step=STEP,
                             device=str(dev), seed=1234, joint_posterior_loss=True)
        return PosteriorJointTrainer(model, cfg, **kw)

    awgn, sym = trainer(AWGN_RANGE), trainer(SYM_RANGE, modulation=Modulation("qam16"), codeword="random")
    (a, a_lo, a_hi), (s, s_lo, s_hi) = medians(
        [lambda: awgn.train_stream(code, steps, val_frames=0), lambda: sym.train_stream(code, steps, val_frames=0)], reps)
    assert awgn.stream_step == sym.stream_step == (reps + WARMUP) * steps

    def rates(ms, lo, hi, t):
        return {"ms_per_step": ms / steps, "ms_per_step_min_max": [lo / steps, hi / steps], "steps_per_s": steps / ms * 1e3,
                "steps_per_s_min_max": [steps / hi * 1e3, steps / lo * 1e3], "codewords_per_s": steps * B / ms * 1e3,
                "first_epoch_loss": t.train_losses[0], "last_epoch_loss": t.train_losses[-1],
                "first_epoch_accuracy": t.train_accuracies[0], "last_epoch_accuracy": t.train_accuracies[-1]}
    return {"workload": f"{name} Neural2D type 2, T={T}, batch {B}, joint loss, {steps} steps per repetition, "
                        f"{(reps + WARMUP) * steps} steps in all at learning rate 1e-3",
            "bi_awgn": dict(rates(a, a_lo, a_hi, awgn), snr_range=list(AWGN_RANGE)),
            "qam16_random": dict(rates(s, s_lo, s_hi, sym), snr_range=list(SYM_RANGE)),
            "qam16_over_bi_awgn_time": s / a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8, help="training steps per repetition")
    ap.add_argument("--only", choices=("channel", "train"), default=None)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"tool": "time_train_sym", "reps": a.reps}
    if a.only != "train":
        res["channel"] = channel(a.reps, dev)
    if a.only != "channel":
        res["training"] = train(a.reps, a.steps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
