#!/usr/bin/env python3
"""Time the mixed-SNR channel kernel next to the single-point one, and stream training next to dataset training.

    python tools/time_train_stream.py [--reps 20] [--steps 8] [--only channel|train]
Prints one JSON line.  Device events around every repetition, two warm-up repetitions, the median of --reps (at least 20).
  channel : engine.awgn_llr_mix with the 13-point grid of snr_range (0, 6), step 0.5, against engine.awgn_llr at 3 dB, at
            [65536, 1998] and [4096, 16200]; the two are timed alternately, output allocation included in both.
  train   : PosteriorJointTrainer on (1998,1512), Neural-2D type 2 at T = 10 under the joint loss with batch 4096, one epoch of
            --steps steps per repetition: `train` (generate_training_data on the host and the upload through the DataLoader
            included -- that is what a user pays) against `train_stream` (frames drawn on the device); no validation in either."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402,F401  (puts the package on sys.path)
import torch  # noqa: E402

CHANNEL_SHAPES = ((65536, 1998), (4096, 16200))
TRAIN = ("ira_1998_1512", 10, 4096)
WARMUP = 2


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
    import engine
    grid = engine.snr_grid((0.0, 6.0), 0.5)
    st, ht = engine.awgn_mix_tables(grid, device=dev)
    scale, shift = engine.awgn_scale_shift(3.0)
    out = []
    for batch, n in CHANNEL_SHAPES:
        kw = dict(seed=1234, stream_id=0, first_frame=0, device=dev)
        (mix, mix_lo, mix_hi), (one, one_lo, one_hi) = medians(
            [lambda: engine.awgn_llr_mix(batch, n, scale=st, shift=ht, **kw),
             lambda: engine.awgn_llr(batch, n, scale=scale, shift=shift, **kw)], reps)
        out.append({"shape": [batch, n], "points": len(grid), "mix_ms": mix, "mix_ms_min_max": [mix_lo, mix_hi],
                    "single_ms": one, "single_ms_min_max": [one_lo, one_hi], "mix_over_single": mix / one,
                    "mix_Gsamples_per_s": batch * n / mix / 1e6, "single_Gsamples_per_s": batch * n / one / 1e6})
        torch.cuda.empty_cache()
    return out


def train(reps, steps, dev):
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    from training_framework import PosteriorJointTrainer, TrainingConfig
    name, T, B = TRAIN
    code = codes.load_code(name, max_iterations=T)

    def trainer():
        model = Neural2DMinSumDecoder(code, 2, T)
        with torch.no_grad():
            for p in model.beta_weights.values():
                p.fill_(0.7)
            for p in model.alpha_weights.values():
                p.fill_(1.0)
        cfg = TrainingConfig(batch_size=B, num_epochs=1, learning_rate=1e-3, snr_range=(0.0, 6.0), snr_step=0.5,
                             device=str(dev), seed=1234, joint_posterior_loss=True)
        return PosteriorJointTrainer(model, cfg)

    host, stream = trainer(), trainer()
    (h, h_lo, h_hi), (s, s_lo, s_hi) = medians(
        [lambda: host.train(code, num_train_samples=steps * B, num_val_samples=0),
         lambda: stream.train_stream(code, steps, val_frames=0)], reps)
    assert stream.stream_step == (reps + WARMUP) * steps

    def rates(ms):
        return {"ms_per_step": ms / steps, "steps_per_s": steps / ms * 1e3, "codewords_per_s": steps * B / ms * 1e3}
    return {"workload": f"{name} Neural2D type 2, T={T}, batch {B}, joint loss, {steps} steps per repetition",
            "train": dict(rates(h), ms_per_step_min_max=[h_lo / steps, h_hi / steps]),
            "train_stream": dict(rates(s), ms_per_step_min_max=[s_lo / steps, s_hi / steps]),
            "stream_over_train_rate": h / s, "train_loss": host.train_losses[-1], "train_stream_loss": stream.train_losses[-1]}


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
    res = {"tool": "time_train_stream", "reps": a.reps}
    if a.only != "train":
        res["channel"] = channel(a.reps, dev)
    if a.only != "channel":
        res["training"] = train(a.reps, a.steps, dev)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
