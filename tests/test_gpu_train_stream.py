"""
GPU tests (-m gpu) of stream training, ``PosteriorJointTrainer.train_stream``: no dataset, every step draws fresh frames of
the device noise stream with each mini-batch holding every SNR point of the grid in equal share (engine.awgn_llr_mix).

The configuration is that of test_gpu_training.test_trainer_reduces_the_loss: small_96_48, Neural2DMinSumDecoder(code, 2, 5)
with all weights 0.3, batch 64, snr_range (1, 4) with step 0.5, lr 0.05, seed 9.  The native steps are deterministic (no
atomics), so a loop written out here reproduces the trainer EXACTLY: every comparison below is ``==`` / ``torch.equal``.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pjt_rcq_cases as rcq_cases

pytestmark = pytest.mark.gpu

B = 64


def fresh_model(kind="n2d"):
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    if kind == "wrcq":
        return rcq_cases.trainer_model(quantizer_gradient="straight_through")
    code = codes.load_code("small_96_48", max_iterations=5)
    model = Neural2DMinSumDecoder(code, 2, 5)
    with torch.no_grad():                     # a deliberately poor start: all weights 0.3
        for p in model.parameters():
            p.fill_(0.3)
    return code, model


def config(**kw):
    from training_framework import TrainingConfig
    base = dict(batch_size=B, num_epochs=2, learning_rate=0.05, snr_range=(1.0, 4.0), snr_step=0.5, device="cuda", seed=9)
    base.update(kw)
    return TrainingConfig(**base)


def fresh_trainer(kind="n2d", **kw):
    from training_framework import PosteriorJointTrainer
    code, model = fresh_model(kind)
    return code, model, PosteriorJointTrainer(model, config(**kw))


def params_of(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def same_params(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


class WrittenOut:
    """the loop the contract describes, step by step: the frames of global step g, the loss, the same Adam"""

    def __init__(self, kind, cfg, dev):
        self.code, self.model = fresh_model(kind)
        self.model.to(dev)
        self.cfg, self.dev = cfg, dev
        self.opt = torch.optim.Adam(self.model.parameters(), lr=cfg.learning_rate)

    def epoch(self, g0, steps):
        """-> (mean loss, per-iteration mean losses or None), formed as the trainer's pass forms them"""
        import engine
        from training_framework import stream_first_frame
        grid = engine.snr_grid(self.cfg.snr_range, self.cfg.snr_step)
        self.model.train(True)
        losses, per_iters = [], []
        for g in range(g0, g0 + steps):
            llr = engine.awgn_llr_mix(B, self.code.n, seed=self.cfg.seed, stream_id=0,
                                      first_frame=stream_first_frame(g, B, 0, 1), snr_db=grid, device=self.dev)
            if self.cfg.joint_posterior_loss:
                loss, per_iter, _, _ = self.model.joint_posterior_loss(llr, None)
                per_iters.append(per_iter.detach().double().cpu())
            else:
                _, post, _ = self.model(llr)
                loss = F.binary_cross_entropy_with_logits(-post, torch.zeros_like(post))
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
            losses.append(float(loss.item()))
        mean_iters = (functools.reduce(lambda a, b: a + b, per_iters) / steps).tolist() if per_iters else None
        return sum(losses, 0.0) / steps, mean_iters


def test_same_seed_same_run(gpu_device):
    runs = []
    for seed in (9, 9, 10):
        code, model, trainer = fresh_trainer(seed=seed, joint_posterior_loss=True)
        hist = trainer.train_stream(code, 4, val_frames=100)
        assert trainer.stream_seed == seed
        runs.append((hist, params_of(model)))
    assert len(runs[0][0]["train_losses"]) == 2
    assert runs[0][0] == runs[1][0] and same_params(runs[0][1], runs[1][1])
    assert runs[2][0]["train_losses"] != runs[0][0]["train_losses"] and runs[2][0]["val_losses"] != runs[0][0]["val_losses"]
    assert set(runs[0][0]) == {"train_losses", "train_accuracies", "gradient_norms", "train_iteration_losses", "val_losses",
                               "val_accuracies", "snr_points", "val_fer_per_point"}
    assert runs[0][0]["snr_points"] == [1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0]


@pytest.mark.parametrize("joint", [True, False])
def test_the_loop_is_what_the_contract_says_and_the_stream_continues(joint, gpu_device):
    code, model, trainer = fresh_trainer(joint_posterior_loss=joint)
    hist = trainer.train_stream(code, 4)
    assert trainer.stream_step == 8
    loop = WrittenOut("n2d", trainer.config, gpu_device)
    want = [loop.epoch(0, 4), loop.epoch(4, 4)]
    assert hist["train_losses"] == [w[0] for w in want]
    if joint:
        assert hist["train_iteration_losses"] == [w[1] for w in want]
        assert all(len(v) == 5 for v in hist["train_iteration_losses"])
    else:
        assert "train_iteration_losses" not in hist
    assert same_params(params_of(model), params_of(loop.model))
    # a second call of one epoch draws from step 8
    trainer.config.num_epochs = 1
    hist = trainer.train_stream(code, 4)
    assert trainer.stream_step == 12 and len(hist["train_losses"]) == 3
    loss, iters = loop.epoch(8, 4)
    assert hist["train_losses"][2] == loss
    if joint:
        assert hist["train_iteration_losses"][2] == iters
    assert same_params(params_of(model), params_of(loop.model))


def test_validation_frames_are_fixed(gpu_device):
    import engine
    code, model, trainer = fresh_trainer(learning_rate=0.0, num_epochs=3, joint_posterior_loss=True)
    before = params_of(model)
    hist = trainer.train_stream(code, 2, val_frames=100)
    assert same_params(before, params_of(model))
    assert len(hist["val_losses"]) == len(hist["val_accuracies"]) == len(hist["val_fer_per_point"]) == 3
    for key in ("val_losses", "val_accuracies", "val_fer_per_point"):
        assert hist[key][0] == hist[key][1] == hist[key][2], key
    assert hist["train_losses"][0] != hist["train_losses"][1]                  # ... while the training frames are fresh
    fer = hist["val_fer_per_point"][0]
    assert len(fer) == 7
    frames = engine.mix_points(0, 100, 7).bincount(minlength=7).tolist()
    assert frames == [15, 15, 14, 14, 14, 14, 14]
    errors = [r * f for r, f in zip(fer, frames)]                              # whole numbers of frames, at these counts
    assert all(abs(e - round(e)) < 1e-9 for e in errors)
    assert sum(round(e) for e in errors) == round((1.0 - hist["val_accuracies"][0]) * 100)
    assert 0 < sum(round(e) for e in errors) < 100                             # weights 0.3 at 1 .. 4 dB: some frames fail
    # they are the frames of stream 1, in blocks of 64 and 36: decoding them directly gives the same rates
    llr = engine.awgn_llr_mix(100, code.n, seed=9, stream_id=1, snr_db=hist["snr_points"], device=gpu_device)
    model.train(False)
    with torch.no_grad():
        bits = model.joint_posterior_loss(llr, None)[2]
    wrong = (bits != 0).any(dim=1).cpu()
    points = engine.mix_points(0, 100, 7)
    assert [int(wrong[points == p].sum()) for p in range(7)] == [round(e) for e in errors]

    code, model, trainer = fresh_trainer(joint_posterior_loss=True)
    hist = trainer.train_stream(code, 2, val_frames=0)
    assert hist["val_losses"] == [] and hist["val_accuracies"] == [] and hist["val_fer_per_point"] == []
    assert len(hist["snr_points"]) == 7 and len(hist["train_losses"]) == 2


def test_it_trains(gpu_device):
    code, model, trainer = fresh_trainer(num_epochs=6)
    hist = trainer.train_stream(code, 8)
    assert len(hist["train_losses"]) >= 2 and hist["train_losses"][-1] < hist["train_losses"][0]
    assert all(np.isfinite(hist["gradient_norms"])) and hist["gradient_norms"][0] > 0
    vals = torch.cat([p.detach().reshape(-1) for p in model.parameters()])
    assert float((vals - 0.3).abs().max()) > 0.05


def test_an_unseeded_run_draws_and_keeps_a_seed(gpu_device):
    code, model, trainer = fresh_trainer(seed=None, num_epochs=1, joint_posterior_loss=True)
    assert trainer.stream_seed is None
    trainer.train_stream(code, 1)
    seed = trainer.stream_seed
    assert isinstance(seed, int) and 0 <= seed < 2 ** 64
    trainer.train_stream(code, 1)
    assert trainer.stream_seed == seed and trainer.stream_step == 2


def test_the_quantised_decoder_trains_on_the_stream(gpu_device):
    code, model, trainer = fresh_trainer("wrcq", num_epochs=1, joint_posterior_loss=True)
    hist = trainer.train_stream(code, 2)
    loop = WrittenOut("wrcq", trainer.config, gpu_device)
    loss, iters = loop.epoch(0, 2)
    assert hist["train_losses"] == [loss] and hist["train_iteration_losses"] == [iters]
    assert same_params(params_of(model), params_of(loop.model))
    assert hist["gradient_norms"][0] > 0
