"""
GPU tests (-m gpu) of stream training on the symbol channel: ``PosteriorJointTrainer(model, config, modulation=...,
codeword="random").train_stream`` draws a fresh random codeword per frame (engine.encode_random), sends it as 16-QAM over
Rayleigh fading with each mini-batch holding every point of the grid in equal share, and trains against the bits that were
sent (engine.sym_llr_mix with want_targets).

Every case: small_96_48, T = 3, batch 64, the three points 6, 8 and 10 dB of Es/N0.  The native steps are deterministic (no
atomics), so a loop written out here reproduces the trainer EXACTLY: every comparison below is ``==`` / ``torch.equal``.
Whether the loss goes down on this channel is a measurement, not a test.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pjt_rcq_cases as rcq_cases

pytestmark = pytest.mark.gpu

B, T = 64, 3
GRID = [6.0, 8.0, 10.0]


def fresh_model(kind="n2d"):
    import codes
    from neural_2d_decoder import Neural2DMinSumDecoder
    from rcq_decoder import WeightedRCQDecoder
    code = codes.load_code("small_96_48", max_iterations=T)
    if kind == "wrcq":
        model = WeightedRCQDecoder(code, 3, 8, rcq_cases.QP3, 2, T, quantizer_gradient="straight_through")
        fill = 1.0
    else:
        model = Neural2DMinSumDecoder(code, 2, T)
        fill = 0.3                            # a deliberately poor start
    with torch.no_grad():
        for p in model.parameters():
            p.fill_(fill)
    return code, model


def modulation():
    from modulation import Modulation
    return Modulation("qam16", "rayleigh")


def config(**kw):
    from training_framework import TrainingConfig
    base = dict(batch_size=B, num_epochs=2, learning_rate=0.05, snr_range=(6.0, 10.0), snr_step=2.0, device="cuda", seed=9)
    base.update(kw)
    return TrainingConfig(**base)


def fresh_trainer(kind="n2d", **kw):
    from training_framework import PosteriorJointTrainer
    code, model = fresh_model(kind)
    return code, model, PosteriorJointTrainer(model, config(**kw), modulation=modulation(), codeword="random")


def params_of(model):
    return {k: p.detach().clone() for k, p in model.named_parameters()}


def same_params(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def block(code, seed, stream_id, first, frames, dev):
    """the frames of one block, by hand: random codewords, then the mixed-SNR symbol channel with the targets"""
    import codes
    import engine
    enc = codes.Encoder.from_graph(code.tanner_graph())
    cw = engine.encode_random(enc, frames, seed=seed, stream_id=stream_id, first_frame=first, device=dev)
    return engine.sym_llr_mix(frames, code.n, seed=seed, stream_id=stream_id, first_frame=first, modulation=modulation(),
                              snr_db=GRID, codeword=cw, device=dev, want_targets=True)


class WrittenOut:
    """the loop the contract describes, step by step: the frames of global step g, the loss, the same Adam"""

    def __init__(self, kind, cfg, dev):
        self.code, self.model = fresh_model(kind)
        self.model.to(dev)
        self.cfg, self.dev = cfg, dev
        self.opt = torch.optim.Adam(self.model.parameters(), lr=cfg.learning_rate)

    def epoch(self, g0, steps):
        """-> (per-step losses, mean loss, per-iteration mean losses or None), formed as the trainer's pass forms them"""
        from training_framework import stream_first_frame
        self.model.train(True)
        losses, per_iters = [], []
        for g in range(g0, g0 + steps):
            llr, targets = block(self.code, self.cfg.seed, 0, stream_first_frame(g, B), B, self.dev)
            assert set(np.unique(targets.cpu().numpy())) == {0.0, 1.0}                    # random codewords indeed
            if self.cfg.joint_posterior_loss:
                loss, per_iter, _, _ = self.model.joint_posterior_loss(llr, targets)
                per_iters.append(per_iter.detach().double().cpu())
            else:
                _, post, _ = self.model(llr)
                loss = F.binary_cross_entropy_with_logits(-post, targets)
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()
            losses.append(float(loss.item()))
        mean_iters = (functools.reduce(lambda a, b: a + b, per_iters) / steps).tolist() if per_iters else None
        return losses, sum(losses, 0.0) / steps, mean_iters


@pytest.mark.parametrize("joint", [True, False])
def test_the_loop_is_what_the_contract_says_and_the_stream_continues(joint, gpu_device):
    code, model, trainer = fresh_trainer(joint_posterior_loss=joint)
    loop = WrittenOut("n2d", trainer.config, gpu_device)
    # the first two steps, one epoch each, so that the history holds each step's own loss
    trainer.config.num_epochs = 2
    hist = trainer.train_stream(code, 1)
    assert trainer.stream_step == 2
    first = [loop.epoch(0, 1), loop.epoch(1, 1)]
    assert hist["train_losses"] == [first[0][0][0], first[1][0][0]]
    if joint:
        assert hist["train_iteration_losses"] == [first[0][2], first[1][2]]
        assert all(len(v) == T for v in hist["train_iteration_losses"])
    else:
        assert "train_iteration_losses" not in hist
    assert same_params(params_of(model), params_of(loop.model))
    assert hist["snr_points"] == GRID
    # a second call of one epoch of three steps draws from step 2
    trainer.config.num_epochs = 1
    hist = trainer.train_stream(code, 3)
    assert trainer.stream_step == 5 and len(hist["train_losses"]) == 3
    _, loss, iters = loop.epoch(2, 3)
    assert hist["train_losses"][2] == loss
    if joint:
        assert hist["train_iteration_losses"][2] == iters
    assert same_params(params_of(model), params_of(loop.model))
    assert all(np.isfinite(hist["gradient_norms"])) and hist["gradient_norms"][0] > 0


def test_same_seed_same_run(gpu_device):
    runs = []
    for seed in (9, 9, 10):
        code, model, trainer = fresh_trainer(seed=seed, joint_posterior_loss=True)
        hist = trainer.train_stream(code, 3, val_frames=100)
        assert trainer.stream_seed == seed
        runs.append((hist, params_of(model)))
    assert len(runs[0][0]["train_losses"]) == 2
    assert runs[0][0] == runs[1][0] and same_params(runs[0][1], runs[1][1])
    assert runs[2][0]["train_losses"] != runs[0][0]["train_losses"] and runs[2][0]["val_losses"] != runs[0][0]["val_losses"]
    assert not same_params(runs[0][1], runs[2][1])
    assert set(runs[0][0]) == {"train_losses", "train_accuracies", "gradient_norms", "train_iteration_losses", "val_losses",
                               "val_accuracies", "snr_points", "val_fer_per_point"}


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
    K = len(GRID)
    assert len(fer) == K
    # they are frames 0 .. 99 of stream 1, in blocks of 64 and 36: decoding them by hand gives the same counts per point
    parts = [block(code, 9, 1, first, frames, gpu_device) for first, frames in ((0, 64), (64, 36))]
    llr, targets = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    whole = block(code, 9, 1, 0, 100, gpu_device)
    assert torch.equal(llr, whole[0]) and torch.equal(targets, whole[1])
    model.train(False)
    with torch.no_grad():
        bits = model.joint_posterior_loss(llr, targets)[2]
    wrong = (bits != targets).any(dim=1).cpu()
    points = engine.mix_points(0, 100, K)
    frames = points.bincount(minlength=K).tolist()
    assert frames == [34, 33, 33]
    assert fer == [int(wrong[points == p].sum()) / frames[p] for p in range(K)]
    assert hist["val_accuracies"][0] == (100 - int(wrong.sum())) / 100


def test_the_quantised_decoder_trains_on_the_stream(gpu_device):
    code, model, trainer = fresh_trainer("wrcq", num_epochs=1, joint_posterior_loss=True)
    hist = trainer.train_stream(code, 2)
    loop = WrittenOut("wrcq", trainer.config, gpu_device)
    _, loss, iters = loop.epoch(0, 2)
    assert hist["train_losses"] == [loss] and hist["train_iteration_losses"] == [iters]
    assert same_params(params_of(model), params_of(loop.model))
    assert np.isfinite(hist["gradient_norms"][0]) and hist["gradient_norms"][0] > 0
    assert all(torch.isfinite(p).all() for p in model.parameters())
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads) and any((g != 0).any() for g in grads)


def test_one_word_and_the_all_zero_word(gpu_device):
    """codeword = a 0/1 array sends that word in every frame; QPSK may send the all-zero word, and the block still carries
    its (all +0.0) targets"""
    import codes
    import engine
    from modulation import Modulation
    from training_framework import PosteriorJointTrainer, stream_first_frame
    code, model = fresh_model()
    enc = codes.Encoder.from_graph(code.tanner_graph())
    word = enc.encode((np.random.default_rng(3).random(enc.k) < 0.5).astype(np.uint8))
    for mod, cw in ((modulation(), word), (Modulation("qpsk"), None)):
        code, model = fresh_model()
        trainer = PosteriorJointTrainer(model, config(num_epochs=1, joint_posterior_loss=True), modulation=mod, codeword=cw)
        hist = trainer.train_stream(code, 1)
        _, ref = fresh_model()
        ref.to(gpu_device)
        ref.train(True)
        llr, targets = engine.sym_llr_mix(B, code.n, seed=9, stream_id=0, first_frame=stream_first_frame(0, B), modulation=mod,
                                          snr_db=GRID, codeword=cw, device=gpu_device, want_targets=True)
        want = torch.from_numpy(np.broadcast_to(np.zeros(code.n) if cw is None else cw, (B, code.n)).astype(np.float32).copy())
        assert torch.equal(targets.cpu(), want)
        loss = ref.joint_posterior_loss(llr, targets)[0]
        assert hist["train_losses"] == [float(loss.item())]


def test_the_default_trainer_is_untouched(gpu_device):
    """without `modulation` the trainer draws what it drew before: all-zero BI-AWGN frames of engine.awgn_llr_mix, no targets"""
    import engine
    from training_framework import PosteriorJointTrainer, stream_first_frame
    code, model = fresh_model()
    cfg = config(snr_range=(1.0, 4.0), snr_step=0.5, num_epochs=1, joint_posterior_loss=True)
    trainer = PosteriorJointTrainer(model, cfg)
    hist = trainer.train_stream(code, 2, val_frames=40)
    _, ref = fresh_model()
    ref.to(gpu_device)
    ref.train(True)
    opt = torch.optim.Adam(ref.parameters(), lr=cfg.learning_rate)
    grid = engine.snr_grid(cfg.snr_range, cfg.snr_step)
    losses = []
    for g in range(2):
        llr = engine.awgn_llr_mix(B, code.n, seed=9, stream_id=0, first_frame=stream_first_frame(g, B), snr_db=grid,
                                  device=gpu_device)
        loss = ref.joint_posterior_loss(llr, None)[0]
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.item()))
    assert hist["train_losses"] == [sum(losses, 0.0) / 2]
    assert same_params(params_of(model), params_of(ref))
    assert hist["snr_points"] == grid.tolist() and len(hist["val_fer_per_point"][0]) == 7
    ref.train(False)
    with torch.no_grad():
        vllr = engine.awgn_llr_mix(40, code.n, seed=9, stream_id=1, snr_db=grid, device=gpu_device)
        vloss, _, bits, _ = ref.joint_posterior_loss(vllr, None)
    assert hist["val_losses"] == [float(vloss.item())]
    assert hist["val_accuracies"] == [int((bits == 0).all(dim=1).sum()) / 40]
