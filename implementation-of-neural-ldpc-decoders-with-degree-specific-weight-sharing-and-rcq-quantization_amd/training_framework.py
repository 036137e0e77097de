"""
Drop-in for the reference module of the same name (training_framework.py): posterior joint training of the
neural min-sum decoders, with the forward AND backward passes on the MI355X engine.

Reference surface mirrored (file:line in /root/reference/training_framework.py):
  TrainingConfig                                  :23-35   same fields and defaults (device default "cuda" here)
  PosteriorJointTrainer(model, config)            :37-291  Adam, generate_training_data, compute_loss,
                                                           train_epoch, train, validate, plot_training_history
  GradientExplosionAnalyzer(model, code)          :293-378 analyze_gradient_explosion, plot_gradient_analysis
  loss = binary_cross_entropy_with_logits(-posteriors, targets)                                       :101

The reference file does not run as shipped (`F` is never imported, :101/:328; the decoders' forward takes one
codeword while the DataLoader hands it [batch, n], :123-127).  This module implements what it sets out to do:
the decoders here accept [B, n], and their posterior carries a grad_fn whose backward is the HIP gradient
sweep (autograd_bridge.py), so the loop below is the reference's loop, batched.

Deviation, stated: training LLRs are generated in the DECODER's sign convention (positive LLR = bit 0) by
default.  The reference calls simulate_awgn_channel, whose opposite convention makes the all-zero codeword
undecodable; `TrainingConfig.llr_convention = "reference"` reproduces that literally.
`train_epoch` returns (loss, accuracy, gradient norm) -- the three values the reference's own caller unpacks
(:208), although its annotation says two.

By default the loss is the reference's: BCE of the posterior the decoder returns, differentiated through every
iteration (full backpropagation through time).  `TrainingConfig.joint_posterior_loss = True` trains the way the paper
does instead: the fixed-T decode with the BCE of EVERY iteration's posterior, each iteration's C2V messages receiving
the gradient of that iteration's posterior only (``model.joint_posterior_loss``, include/ldpc_hip.h ldpc_train_joint);
no per-iteration history is kept, so the memory does not grow with T.  `use_posterior_training` is the reference's
field and changes nothing.

Addition, stated: `PosteriorJointTrainer.train_stream` is the same loop without a dataset.  The reference trains on one
fixed set of 1000 host-drawn frames and never reads its own `snr_step`; `train_stream` draws fresh frames every step from
the counter-based device noise stream, each mini-batch holding every point of the grid snr_range / snr_step in equal share
(engine.awgn_llr_mix), reproducible bit for bit from (seed, step).  `PosteriorJointTrainer(..., modulation=, codeword=)` puts
that loop on the symbol channel: Gray-mapped QAM over AWGN or Rayleigh fading with a fresh random codeword per frame, the
LLRs and the targets of a block from one kernel (engine.sym_llr_mix).
"""

from __future__ import annotations

import logging
import os
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim
from torch.utils.data import DataLoader, TensorDataset

from ldpc_decoder import LDPCCode, simulate_awgn_channel

logger = logging.getLogger(__name__)


@dataclass
class TrainingConfig:
    """Training configuration"""
    batch_size: int = 32
    num_epochs: int = 100
    learning_rate: float = 0.001
    snr_range: Tuple[float, float] = (0.0, 6.0)
    snr_step: float = 0.5
    max_grad_norm: float = 1.0
    use_posterior_training: bool = True      # the reference's field; no effect (see joint_posterior_loss)
    use_gradient_clipping: bool = False
    clip_threshold: float = 1e-3
    device: str = "cuda"
    llr_convention: str = "decoder"          # "reference": simulate_awgn_channel literally (see module docstring)
    data_parallel: bool = False              # one process per GPU: average the gradients over the ranks every step
    seed: Optional[int] = None               # training-data noise seed (decoder convention only)
    joint_posterior_loss: bool = False       # True: the per-iteration posterior loss of the paper (model.joint_posterior_loss)


def _grad_norm(model: nn.Module) -> float:
    """l2 norm over every parameter gradient that exists"""
    sq = [float(p.grad.detach().pow(2).sum()) for p in model.parameters() if p.grad is not None]
    return float(np.sqrt(sum(sq))) if sq else 0.0


def _frames_ok(decoded: torch.Tensor, targets: Optional[torch.Tensor]) -> torch.Tensor:
    """bool [B]: every bit of the frame right; targets None is the all-zero codeword, for which no tensor is formed"""
    return (decoded == (0 if targets is None else targets)).all(dim=1)


def stream_first_frame(g: int, batch_size: int, rank: int = 0, world: int = 1) -> int:
    """first frame of global step g on rank `rank` of `world` in stream training: step g draws the `world` consecutive
    blocks of batch_size frames that start at frame g * world * batch_size, one per rank, so no frame is drawn twice"""
    g, batch_size, rank, world = int(g), int(batch_size), int(rank), int(world)
    if g < 0 or batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError("need g >= 0, batch_size >= 1 and 0 <= rank < world")
    return (g * world + rank) * batch_size


class _StreamBlocks:
    """what `_pass` iterates over in stream training: blocks (first_frame, frames) drawn one by one, with `drawn()` called after
    each block.  `draw` returns the block's LLRs, yielded as (llr, None) -- None is the all-zero codeword -- or the pair
    (llr, targets) of a draw on per-frame codewords, yielded as it is"""

    def __init__(self, blocks, draw, drawn=None):
        self.blocks, self.draw, self.drawn = list(blocks), draw, drawn

    def __len__(self):
        return len(self.blocks)

    def __iter__(self):
        for first, frames in self.blocks:
            block = self.draw(first, frames)
            if self.drawn is not None:
                self.drawn()
            yield block if isinstance(block, tuple) else (block, None)


def _plot_series(panels, figsize, save_path):
    """panels: [(kind, data, title, xlabel, ylabel)], kind in {"line", "hist", "scatter"}"""
    import matplotlib.pyplot as plt
    fig, axes = plt.subplots(1, len(panels), figsize=figsize)
    for ax, (kind, data, title, xlabel, ylabel) in zip(np.atleast_1d(axes), panels):
        if kind == "line":
            ax.plot(data)
        elif kind == "hist":
            ax.hist(data, bins=20, alpha=0.7)
        else:
            ax.scatter(data[0], data[1], alpha=0.6)
        ax.set(title=title, xlabel=xlabel, ylabel=ylabel)
        ax.grid(True)
    fig.tight_layout()
    if save_path:
        fig.savefig(save_path)
    plt.show()


class _TrainerType(type):
    """the call ``PosteriorJointTrainer(model, config, *, rate_matching=None, modulation=None, codeword=None)``.  `__init__`
    keeps the parameter list it has had since rate matching, which callers inspect and subclasses replace; the two
    symbol-channel keywords are taken here and set on the finished trainer by `_set_symbol_channel`, which refuses what
    cannot be trained."""

    def __call__(cls, *args, modulation=None, codeword=None, **kwargs):     # the rest is `__init__`'s, a subclass's included
        trainer = super().__call__(*args, **kwargs)
        if modulation is not None or codeword is not None:
            trainer._set_symbol_channel(modulation, codeword)
        return trainer


class PosteriorJointTrainer(metaclass=_TrainerType):
    """Adam on the BCE of the posterior the decoder returns (default), or -- config.joint_posterior_loss -- on the
    weighted sum of every iteration's posterior BCE with the paper's posterior-local gradient; then the history also
    holds each epoch's per-iteration training losses (`train_iteration_losses`, one [T] list per epoch).
    rate_matching (keyword only, a rate_matching.RateMatching): the profile `train_stream` draws its training and validation
    frames through -- punctured bits enter the decoder as +0.0, shortened ones as +short_llr; `train` does not use it.
    modulation (keyword only, a modulation.Modulation): `train_stream` draws its frames on the symbol channel instead
    (engine.sym_llr_mix: Gray-mapped BPSK .. 256-QAM over AWGN or Rayleigh fading, LLRs by the modulation's demapper, snr_range read as Es/N0) and
    trains against the bits that were sent.  codeword (with a modulation only): None, the all-zero word (BPSK and QPSK only:
    from 16-QAM up it sends one corner point and the bit levels are not output-symmetric); "random", a fresh codeword per frame
    (engine.encode_random on the code's graph); or a 0/1 array of length n, one word for every frame.  `train`, the
    host-drawn BI-AWGN dataset, refuses a trainer with a modulation."""

    modulation, codeword = None, None                 # the symbol channel of train_stream: set by _set_symbol_channel

    def __init__(self, model: nn.Module, config: TrainingConfig, *, rate_matching=None):
        self.model, self.config = model, config
        if rate_matching is not None:
            from rate_matching import RateMatching
            if not isinstance(rate_matching, RateMatching):
                raise ValueError("rate_matching must be a rate_matching.RateMatching")
        self.rate_matching = rate_matching
        self._stream_encoder = None                   # train_stream under codeword="random": (graph, codes.Encoder)
        self.device = torch.device(config.device)
        self.model.to(self.device)
        self.optimizer = optim.Adam(self.model.parameters(), lr=config.learning_rate)
        self.train_losses: List[float] = []
        self.train_accuracies: List[float] = []
        self.gradient_norms: List[float] = []
        self.train_iteration_losses: List[List[float]] = []
        self._pass_iteration_losses: Optional[List[float]] = None
        self.stream_step = 0                          # train_stream: global steps drawn so far over the trainer's life
        self.stream_seed: Optional[int] = None        # train_stream: config.seed, or the seed drawn at its first call
        self.val_losses: List[float] = []
        self.val_accuracies: List[float] = []
        self.val_fer_per_point: List[List[float]] = []
        # a decoder with learn_quantizer: its (C, gamma) pairs after each epoch (the float64 pair trains with the rest of
        # model.parameters(): Adam keeps its state per parameter in that parameter's dtype)
        self.quantizer_params: List[List[Tuple[float, float]]] = []
        logger.info("trainer ready: %d trainable scalars", sum(p.numel() for p in model.parameters()))

    def _set_symbol_channel(self, modulation, codeword):
        """the keywords `modulation` and `codeword` of the constructor call, checked against the rest of the trainer"""
        config, rate_matching = self.config, self.rate_matching
        if modulation is None:
            if codeword is not None:
                raise ValueError("codeword needs a modulation: per-frame codewords on the BI-AWGN stream are not provided "
                                 "(Modulation('qpsk') is that channel in law at the same snr_db)")
        else:
            from modulation import Constellation, Modulation
            if not isinstance(modulation, Modulation):
                raise ValueError("modulation must be a modulation.Modulation")
            if rate_matching is not None:
                raise ValueError("rate_matching together with modulation is not provided (DESIGN.md section 3j)")
            if config.llr_convention != "decoder":
                raise ValueError("modulation maps bit 0 to the positive half: llr_convention must be 'decoder'")
            if isinstance(codeword, str):
                if codeword != "random":
                    raise ValueError(f"codeword must be None, 'random' or a 0/1 array, got {codeword!r}")
            elif codeword is not None:
                codeword = np.asarray(codeword)
                if codeword.ndim != 1 or not np.isin(codeword, (0, 1)).all():
                    raise ValueError("codeword must be None, 'random' or a 0/1 array of length n")
            elif isinstance(modulation, Constellation):
                raise ValueError(f"{modulation.scheme}: a constellation table has no guaranteed symmetry, so the all-zero codeword "
                                 f"says nothing about the others: train with codeword=\"random\" (or give a codeword)")
            elif modulation.bits_per_symbol >= 4:
                raise ValueError(f"{modulation.scheme} with the all-zero codeword sends one corner point only and its bit "
                                 f"levels are not output-symmetric: train with codeword='random'")
        self.modulation, self.codeword = modulation, codeword

    # ---- data ------------------------------------------------------------------------------------------
    def generate_training_data(self, code: LDPCCode, num_samples: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(llrs [N, n], targets [N, n]): all-zero codewords over AWGN, sample i at SNR linspace(lo, hi, N)[i]
        (training_framework.py:57-84)"""
        targets = torch.zeros(num_samples, code.n, dtype=torch.float32)
        lo, hi = self.config.snr_range
        snr_db = torch.linspace(lo, hi, num_samples)
        if self.config.llr_convention == "reference":          # the reference's channel helper, one call per sample
            rows = [torch.as_tensor(simulate_awgn_channel(targets[i].numpy(), float(snr_db[i])), dtype=torch.float32)
                    for i in range(num_samples)]
            llrs = torch.stack(rows) if rows else torch.zeros_like(targets)
            return llrs, targets
        gen = torch.Generator()
        if self.config.seed is None:
            gen.seed()
        else:
            gen.manual_seed(int(self.config.seed))
        var = torch.pow(10.0, -snr_db.double() / 10.0).unsqueeze(1)            # noise variance at unit symbol energy
        noise = torch.randn(num_samples, code.n, generator=gen, dtype=torch.float64)
        return (2.0 * (1.0 + var.sqrt() * noise) / var).float(), targets

    def compute_loss(self, outputs: torch.Tensor, targets: torch.Tensor, posteriors: torch.Tensor) -> torch.Tensor:
        """BCE-with-logits of -posterior against the transmitted bits (training_framework.py:101); `outputs` unused"""
        return F.binary_cross_entropy_with_logits(posteriors.neg(), targets.to(posteriors.dtype))

    # ---- one pass over a loader ----------------------------------------------------------------------------
    def _pass(self, loader, train: bool, frame_errors: Optional[list] = None) -> Tuple[float, float, float]:
        """`loader`: a sized iterable of (llrs, targets); targets None is the all-zero codeword (stream training).
        frame_errors: a list that receives each batch's bool [B] frame-error flags, on the device"""
        self.model.train(train)
        loss_sum, right, seen, norms = 0.0, 0, 0, []
        joint = self.config.joint_posterior_loss
        iter_sum = None
        for step, (llrs, targets) in enumerate(loader):
            llrs, targets = llrs.to(self.device), None if targets is None else targets.to(self.device)
            with torch.set_grad_enabled(train):
                if joint:       # loss on every iteration's posterior, bits of the last one
                    loss, per_iter, decoded, _ = self.model.joint_posterior_loss(llrs, targets)
                    per_iter = per_iter.detach().double().cpu()
                    iter_sum = per_iter if iter_sum is None else iter_sum + per_iter
                else:
                    decoded, posteriors, _ = self.model(llrs)
                    loss = self.compute_loss(decoded, torch.zeros_like(posteriors) if targets is None else targets, posteriors)
            if train:
                self.optimizer.zero_grad()
                loss.backward()                                 # HIP backward sweeps (autograd_bridge.py)
                if self.config.data_parallel:                   # every rank trained on its own shard
                    import sharding
                    sharding.all_reduce_gradients(self.model.parameters())
                norms.append(_grad_norm(self.model))
                if self.config.use_gradient_clipping:
                    torch.nn.utils.clip_grad_norm_(self.model.parameters(), self.config.clip_threshold)
                self.optimizer.step()
                if step % 10 == 0:
                    logger.info("step %d: loss %.6f, |grad| %.6f", step, loss.item(), norms[-1])
            loss_sum += float(loss.item())
            ok = _frames_ok(decoded, targets)
            right += int(ok.sum().item())
            seen += llrs.shape[0]
            if frame_errors is not None:
                frame_errors.append(~ok)
        batches = max(len(loader), 1)
        self._pass_iteration_losses = None if iter_sum is None else (iter_sum / batches).tolist()
        return loss_sum / batches, right / max(seen, 1), (float(np.mean(norms)) if norms else 0.0)

    def _record_quantizer(self, history: Optional[dict] = None):
        """after an epoch: append the learned (C, gamma) pairs; with `history`: put the series into it as quantizer_params"""
        if not getattr(self.model, "learn_quantizer", False):
            return
        if history is not None:
            history["quantizer_params"] = self.quantizer_params
            return
        self.quantizer_params.append([(float(c), float(g)) for c, g in zip(self.model.quantizer_C.detach().cpu().tolist(),
                                                                          self.model.quantizer_gamma.detach().cpu().tolist())])

    def train_epoch(self, train_loader: DataLoader) -> Tuple[float, float, float]:
        """-> (mean loss, frame accuracy, mean gradient norm)"""
        return self._pass(train_loader, train=True)

    def validate(self, val_loader: DataLoader) -> Tuple[float, float, float]:
        """-> (mean loss, frame accuracy, 0.0)"""
        return self._pass(val_loader, train=False)

    def train(self, code: LDPCCode, num_train_samples: int = 1000, num_val_samples: int = 200) -> Dict[str, List[float]]:
        if self.modulation is not None:
            raise ValueError("train draws its dataset on the host as all-zero BI-AWGN frames: a trainer with a modulation "
                             "trains with train_stream")
        bs = self.config.batch_size
        train_loader = DataLoader(TensorDataset(*self.generate_training_data(code, num_train_samples)), batch_size=bs, shuffle=True)
        val_loader = DataLoader(TensorDataset(*self.generate_training_data(code, num_val_samples)), batch_size=bs, shuffle=False)
        for epoch in range(self.config.num_epochs):
            t0 = time.time()
            loss, acc, gnorm = self.train_epoch(train_loader)
            self._record_quantizer()
            if self.config.joint_posterior_loss:
                self.train_iteration_losses.append(self._pass_iteration_losses or [])
            vloss, vacc, _ = self.validate(val_loader)
            self.train_losses.append(loss)
            self.train_accuracies.append(acc)
            self.gradient_norms.append(gnorm)
            logger.info("epoch %d/%d: train loss %.6f acc %.4f | val loss %.6f acc %.4f | |grad| %.6f | %.2f s",
                        epoch + 1, self.config.num_epochs, loss, acc, vloss, vacc, gnorm, time.time() - t0)
            if acc > 0.99:                                       # the reference's stop rule (:222-224)
                break
        history = {"train_losses": self.train_losses, "train_accuracies": self.train_accuracies,
                   "gradient_norms": self.gradient_norms}
        if self.config.joint_posterior_loss:
            history["train_iteration_losses"] = self.train_iteration_losses
        self._record_quantizer(history)
        return history

    def train_stream(self, code: LDPCCode, steps_per_epoch: int, val_frames: int = 0, *, train_stream_id: int = 0,
                     val_stream_id: int = 1) -> Dict[str, list]:
        """`train` without a dataset: every step draws config.batch_size fresh frames of the counter-based device noise stream
        (engine.awgn_llr_mix, seed config.seed), frame f at point f % K of the grid engine.snr_grid(config.snr_range,
        config.snr_step), so every mini-batch holds each SNR point in equal share, up to one frame.  Global step g -- counted
        in self.stream_step over the trainer's life, a second call continues the stream -- draws the frames from
        stream_first_frame(g, batch_size, rank, world) of stream train_stream_id (one block per rank under
        config.data_parallel with an initialised process group); the transmitted codeword is all zero; with the trainer's
        rate_matching the draw is engine.awgn_llr_mix(..., rate_matching=...), the same frames with the profile applied.  A run is reproducible
        bit for bit from (seed, step); with config.seed None a seed is drawn once, kept in self.stream_seed and logged.
        With the trainer's modulation the draw of a block is instead engine.encode_random(Encoder.from_graph(graph), frames,
        seed, stream_id, first_frame) under codeword="random", then engine.sym_llr_mix(..., want_targets=True) at the table
        modulation.amp_table(grid), the grid read as Es/N0: the block is (llr, targets) and loss, accuracy and validation are
        computed against the bits that were sent; steps, streams and frame ranges are the same.
        After each epoch frames 0 .. val_frames - 1 of stream val_stream_id are validated, the same frames every epoch.
        -> the history of `train` plus val_losses, val_accuracies, snr_points (the grid) and val_fer_per_point (per epoch,
        the frame-error rate of each of the K points; nan for a point no validation frame falls on)."""
        import engine
        cfg = self.config
        bs, steps_per_epoch, val_frames = int(cfg.batch_size), int(steps_per_epoch), int(val_frames)
        if bs < 1 or steps_per_epoch < 1 or val_frames < 0:
            raise ValueError("need batch_size >= 1, steps_per_epoch >= 1 and val_frames >= 0")
        grid = engine.snr_grid(cfg.snr_range, cfg.snr_step)
        K = len(grid)
        if self.stream_seed is None:
            if cfg.seed is None:
                self.stream_seed = int.from_bytes(os.urandom(8), "little")
                logger.info("stream training: drew seed %d", self.stream_seed)
            else:
                self.stream_seed = int(cfg.seed)
        world, rank = 1, 0
        if cfg.data_parallel and torch.distributed.is_available() and torch.distributed.is_initialized():
            world, rank = torch.distributed.get_world_size(), torch.distributed.get_rank()
        if self.modulation is None:
            scale_tab, shift_tab = engine.awgn_mix_tables(grid, cfg.llr_convention, self.device)

            def draw(stream_id):
                return lambda first, frames: engine.awgn_llr_mix(frames, code.n, seed=self.stream_seed, stream_id=stream_id,
                                                                 first_frame=first, scale=scale_tab, shift=shift_tab,
                                                                 device=scale_tab.device, rate_matching=self.rate_matching)
        else:                         # the symbol channel: the encoder, the amp table and the one word are built once per call
            mod, dev = self.modulation, engine._require_gpu(self.device)
            mod.check(code.n)
            amp_tab = engine._mix_table(mod.amp_table(grid), "amp", dev)
            random = isinstance(self.codeword, str)
            encoder = None
            if random:                # kept across calls on one graph: its device copy is cached on the encoder object
                graph = code.tanner_graph()
                if self._stream_encoder is None or self._stream_encoder[0] is not graph:
                    from codes import Encoder
                    self._stream_encoder = (graph, Encoder.from_graph(graph))
                encoder = self._stream_encoder[1]
            one = None if random or self.codeword is None else engine.pack_codeword(self.codeword, code.n, dev)

            def draw(stream_id):
                def block(first, frames):
                    cw = one
                    if random:
                        cw = engine.encode_random(encoder, frames, seed=self.stream_seed, stream_id=stream_id,
                                                  first_frame=first, device=dev)
                    return engine.sym_llr_mix(frames, code.n, seed=self.stream_seed, stream_id=stream_id, first_frame=first,
                                              modulation=mod, amp=amp_tab, codeword=cw, device=dev, want_targets=True)
                return block

        def step_drawn():
            self.stream_step += 1

        val_blocks = [(first, min(bs, val_frames - first)) for first in range(0, val_frames, bs)]
        for epoch in range(cfg.num_epochs):
            t0 = time.time()
            g0 = self.stream_step
            blocks = [(stream_first_frame(g0 + k, bs, rank, world), bs) for k in range(steps_per_epoch)]
            loss, acc, gnorm = self._pass(_StreamBlocks(blocks, draw(train_stream_id), step_drawn), train=True)
            self._record_quantizer()
            if cfg.joint_posterior_loss:
                self.train_iteration_losses.append(self._pass_iteration_losses or [])
            self.train_losses.append(loss)
            self.train_accuracies.append(acc)
            self.gradient_norms.append(gnorm)
            if val_blocks:
                wrong: List[torch.Tensor] = []
                vloss, vacc, _ = self._pass(_StreamBlocks(val_blocks, draw(val_stream_id)), train=False, frame_errors=wrong)
                wrong = torch.cat(wrong)
                points = engine.mix_points(0, val_frames, K, device=wrong.device)
                frames = torch.bincount(points, minlength=K)
                errors = torch.bincount(points[wrong], minlength=K)
                self.val_losses.append(vloss)
                self.val_accuracies.append(vacc)
                self.val_fer_per_point.append((errors.double() / frames.double()).tolist())     # 0 / 0: nan
                logger.info("epoch %d/%d: train loss %.6f acc %.4f | val loss %.6f acc %.4f | |grad| %.6f | %.2f s",
                            epoch + 1, cfg.num_epochs, loss, acc, vloss, vacc, gnorm, time.time() - t0)
            else:
                logger.info("epoch %d/%d: train loss %.6f acc %.4f | |grad| %.6f | %.2f s",
                            epoch + 1, cfg.num_epochs, loss, acc, gnorm, time.time() - t0)
            if acc > 0.99:                                       # the stop rule of `train`
                break
        history = {"train_losses": self.train_losses, "train_accuracies": self.train_accuracies,
                   "gradient_norms": self.gradient_norms, "val_losses": self.val_losses,
                   "val_accuracies": self.val_accuracies, "snr_points": grid.tolist(),
                   "val_fer_per_point": self.val_fer_per_point}
        if cfg.joint_posterior_loss:
            history["train_iteration_losses"] = self.train_iteration_losses
        self._record_quantizer(history)
        return history

    def plot_training_history(self, save_path: Optional[str] = None):
        _plot_series([("line", self.train_losses, "Training Loss", "Epoch", "Loss"),
                      ("line", self.train_accuracies, "Training Accuracy", "Epoch", "Accuracy"),
                      ("line", self.gradient_norms, "Gradient Norms", "Epoch", "Gradient Norm")], (15, 5), save_path)


class GradientExplosionAnalyzer:
    """Distribution of the decoder's gradient norm over random inputs (training_framework.py:293-378)."""

    def __init__(self, model: nn.Module, code: LDPCCode):
        self.model, self.code = model, code

    def analyze_gradient_explosion(self, num_samples: int = 100) -> Dict[str, List[float]]:
        self.model.eval()
        norms, iteration_counts = [], []
        for _ in range(num_samples):
            decoded, posterior, iterations = self.model(2.0 * torch.randn(self.code.n))
            if posterior.requires_grad:     # no parameter on the path (e.g. sharing type 4 stopping at once): norm 0
                F.binary_cross_entropy_with_logits(posterior.neg(), torch.zeros_like(posterior)).backward()
            norms.append(_grad_norm(self.model))
            iteration_counts.append(iterations)
            self.model.zero_grad()
        return {"gradient_magnitudes": norms, "iteration_counts": iteration_counts,
                "mean_gradient": np.mean(norms), "std_gradient": np.std(norms), "max_gradient": np.max(norms)}

    def plot_gradient_analysis(self, results: Dict[str, List[float]], save_path: Optional[str] = None):
        _plot_series([("hist", results["gradient_magnitudes"], "Gradient Magnitude Distribution", "Gradient Magnitude", "Frequency"),
                      ("scatter", (results["iteration_counts"], results["gradient_magnitudes"]),
                       "Gradient Magnitude vs Iterations", "Iterations", "Gradient Magnitude")], (12, 5), save_path)


def create_dvbs2_code(reference_dense: bool = False) -> LDPCCode:
    """Create a DVBS-2 LDPC code for testing -- the (16200, 7200) code the reference's callers ask for
    (training_framework.py:379-400; examples.py:360, simulation_framework.py:428), ``max_iterations=50``.

    Deviation, stated: the reference fills a dense 9000 x 16200 matrix with ``np.random.randint(0, 2)`` (check
    degree ~8100, variable degree ~4500, 73 M edges) -- not an LDPC matrix, and its own per-edge Python loops
    cannot decode one vector of it in practical time.  By default this returns the committed DVB-S2-LIKE sparse
    code of the same dimensions (``codes.load_code("dvbs2_like_16200_7200")``: IRA staircase, E = 48599, the node
    degree profile of the paper's Table II), which every decoder of this package runs.
    ``reference_dense=True`` reproduces the reference's matrix bit for bit (same global-RNG draws, ~1.2 GB while it
    is being drawn); its degrees lie beyond the summation orders the engine restates, so decoding it raises
    NotImplementedError."""
    n, k = 16200, 7200
    if not reference_dense:
        import codes
        return codes.load_code("dvbs2_like_16200_7200", max_iterations=50)
    np.random.seed(42)
    H = np.random.randint(0, 2, (n - k, n))
    for i in range(n - k):
        if np.sum(H[i, :]) == 0:
            H[i, np.random.randint(0, n)] = 1
    for j in range(n):
        if np.sum(H[:, j]) == 0:
            H[np.random.randint(0, n - k), j] = 1
    return LDPCCode(n=n, k=k, H=H, max_iterations=50)
