"""
Drop-in for the reference module of the same name (rcq_decoder.py):
``NonUniformQuantizer``, ``RCQMinSumDecoder``, ``WeightedRCQDecoder`` with the
quantise / reconstruct / min-sum loop running on the MI355X engine (C2V messages
live in HBM as the 1-byte quantiser codes, reconstruction is a LUT in LDS).

Reference behaviour mirrored (file:line in /root/reference):
  NonUniformQuantizer(bc, C, gamma): thresholds C*(j/(2^(bc-1)-1))^gamma as Python
      floats; quantize -> int64 codes sign_bit*2^(bc-1)+level; dequantize -> float32
                                                               rcq_decoder.py:22-121
  RCQMinSumDecoder(code, bc, bv, quantizer_params, max_iterations=50, layered=False)
      .decode(llr[n]) -> (int32[n], bool, int); ``bv`` stored and unused as in the
      reference; quantiser schedule by thirds                  rcq_decoder.py:123-279
  WeightedRCQDecoder(code, bc, bv, quantizer_params, weight_sharing_type=2,
      max_iterations=50, layered=False)(llr[n]) -> (int32[n], float32[n], int);
      ``layered`` stored and ignored by forward as in the reference (every value but "paper", see below)
                                                               rcq_decoder.py:352-597

``RCQMinSumDecoder(layered=True)`` runs the reference's layered schedule exactly as the
reference executes it (rcq_decoder.py:281-350): checks in order on running
posteriors; because the reference re-creates its message matrix for every check, the
"previous message" it subtracts is always zero, and so it is here (bug-compatible by decision --
parity is the contract; a single-check code, the one case where the subtraction would be real,
is rejected).

Extensions: batched ``[B, n]`` input and ``early_stop=False`` as in the other decoders;
``RCQMinSumDecoder(layered="paper")`` runs the layered schedule that code sets out to implement (previous message
subtracted before a check's update, new one added -- the one change is the message matrix living across checks).
Nothing in the reference executes it, so its parity is UNPINNED: it is checked against an independent CPU
restatement only.

``WeightedRCQDecoder(layered="paper")`` is the weighted layered decoder of the RCQ paper, per codeword:
P_v = llr_v; R_{c,v} = "no message" (reconstructs to 0).  Iteration t: checks in ascending order; for check c
  u_v = P_v - Q_{t'}^{-1}(R_{c,v})          (t' = the iteration that wrote the code),
  min1 / min2 / sign product over the u_v  (tie and sign(0) conventions of the flooding W-RCQ decode),
  m = beta_t[beta_slot(c, v)] * sign_excl * (v == argmin ? min2 : min1)   (the flooding W-RCQ fp32 product),
  R_{c,v} = Q_t(m),  P_v = u_v + Q_t^{-1}(R_{c,v});
then hard decisions (P < 0) and the syndrome; with early_stop a codeword that satisfies every check stops with its
posteriors, iterations t+1.  beta is indexed exactly as in the flooding forward (same slots and tables, all four sharing
types).  alpha is NOT used: a layered update has no separate variable-node sum for it to scale.  Posteriors are fp32;
``bv`` stays stored and unused.  With every beta 1.0 the result is bit-identical to RCQMinSumDecoder(layered="paper").
Every other value of ``layered`` (True included) runs the flooding decode, as the reference does.  ``forward`` of the
layered schedule has no backward pass; ``joint_posterior_loss`` trains it (below).

Training the flooding ``WeightedRCQDecoder`` (an extension; under the reference's autograd the quantiser is a chain of
``torch.where`` over comparisons, rcq_decoder.py:59-91, and beta never receives a gradient): with
``quantizer_gradient="straight_through"`` -- constructor argument, or keyword of ``joint_posterior_loss`` --
``joint_posterior_loss`` runs the decoder's own fixed-T decode and gives the posterior-local gradient of the per-iteration
loss (as the min-sum decoders' ``joint_posterior_loss``) with the quantiser treated as
    c2v = Q^-1(code)                       (the forward's value, exact)
    d c2v / d m := 1  where the code the forward wrote lies below the top level (the dead zone included)
                   0  where it saturated,      m = beta_t[slot(e)] * sign product * min
(include/ldpc_hip.h ldpc_train_joint_ste).  Without the option the decoder refuses to train, as before.

Training ``WeightedRCQDecoder(layered="paper")``: ``joint_posterior_loss`` needs BOTH ``quantizer_gradient="straight_through"``
and ``layered_gradient="posterior_local"`` (each a keyword-only constructor argument or a keyword of the call; the call's
value wins) and refuses with either missing.  The forward is the fixed-T layered decode above, bit for bit; iteration t's
loss reaches beta_t and the LLRs through the one check update that wrote each message -- P_t[v] = llr_v + the messages at v,
u = llr_v + a constant, d Q^-1(Q(m)) / d m by the rule above on the code the update stored -- nothing earlier and nothing
through another check of the same iteration; alpha, which the schedule does not use, gets a zero gradient
(include/ldpc_hip.h ldpc_train_joint_layered_ste).  ``layered_gradient`` on a flooding W-RCQ decoder is a ValueError.

Learned quantisers: ``WeightedRCQDecoder(..., learn_quantizer=True)`` (keyword only) makes the ``(C, gamma)`` pairs
parameters -- ``quantizer_C`` and ``quantizer_gamma``, float64 ``[n_quantizers]``, initialised from ``quantizer_params`` --
and ``joint_posterior_loss`` gives them a gradient on both schedules.  The value path stays the reference's:
``self.quantizers`` is the list of ``NonUniformQuantizer(bc, float(C), float(gamma))`` of the current parameter values (rebuilt
when they change, writes through ``.data`` included), so at its initial parameters the decoder is bit-identical to the plain
one, and a plain decoder built from the learned pairs decodes as the trained one does.  The gradient: iteration t's
posterior is llr + the reconstructed messages at the variable and level l reconstructs to tau_l, so d J_t / d tau_l is the
signed per-level sum of the loss seed over the codes the forward stored (ldpc_train_joint_ste_levels; level 0 and the top
level like any other -- a saturated message, which passes nothing to beta, still moves the top level); the thresholds as
decision boundaries pass no gradient (straight-through), and with x_j = j / (L - 1)
    d tau_j / d C = x_j^gamma,      d tau_j / d gamma = C x_j^gamma ln x_j  (1 <= j <= L - 2;  := 0 at j = 0 and j = L - 1)
in float64 on the host (``quantizer_param_grads``).  A change of ``(C, gamma)`` re-uploads the tables into the SAME native
decoder (``DecodeEngine.set_quantizers``): the engine object and its handle survive optimiser steps.  Non-finite ``C`` or
``gamma``, or ``gamma < 0``, raise a ValueError naming the parameter at the next decode or loss; ``bc < 2`` cannot be learned
(one level, and the reference's constructor divides by zero).  No constraint keeps the learned table positive and sorted:
one that is not decodes through the generic kernel forms, as a freshly created decoder with it would.
"""

from __future__ import annotations

import logging
from typing import List, Tuple

import numpy as np
import torch

from ldpc_decoder import LDPCCode, _as_batch
from neural_2d_decoder import _DegreeSharedDecoder

logger = logging.getLogger(__name__)


class NonUniformQuantizer:
    """
    Non-uniform quantiser with power-function thresholds
    tau_j = C * (j / (2^(bc-1) - 1))^gamma,  j = 0 .. 2^(bc-1)-1.
    Host-side utility (vector API of the reference); inside the decoders the same
    tables are applied by the HIP kernels.
    """

    def __init__(self, bc: int, C: float, gamma: float):
        self.bc = bc
        self.C = C
        self.gamma = gamma
        self.thresholds = self._calculate_thresholds()
        logger.info(f"Initialized quantizer: bc={bc}, C={C}, gamma={gamma}")

    def _calculate_thresholds(self) -> List[float]:
        levels = 2 ** (self.bc - 1)
        top = levels - 1
        return [self.C * (j / top) ** self.gamma for j in range(levels)]

    def thresholds_f32(self) -> np.ndarray:
        """float32(tau): the values the fp32 comparisons actually use."""
        return np.asarray(self.thresholds, dtype=np.float32)

    def quantize(self, x: torch.Tensor) -> torch.Tensor:
        """code = (sign(x) < 0) * 2^(bc-1) + max{j : |x| >= tau_j}   (int64)"""
        levels = 2 ** (self.bc - 1)
        mag = torch.abs(x)
        level = torch.zeros_like(mag, dtype=torch.long)
        for j, tau in enumerate(self.thresholds):      # later thresholds overwrite earlier ones
            level = torch.where(mag >= tau, torch.full_like(level, j), level)
        sign_bit = (torch.sign(x) < 0).long()
        return sign_bit * levels + level

    def dequantize(self, quantized: torch.Tensor) -> torch.Tensor:
        """(1 - 2*sign_bit) * tau[code mod 2^(bc-1)] as float32 (code 2^(bc-1) is -0.0)"""
        levels = 2 ** (self.bc - 1)
        sign_bit = (quantized >= levels).long()
        idx = quantized % levels
        table = torch.tensor(self.thresholds, dtype=torch.float32, device=quantized.device)
        mag = table[idx.clamp(0, levels - 1)]
        return (1 - 2 * sign_bit.float()) * mag


def _quantizer_index(n_quantizers: int, max_iterations: int, iteration: int) -> int:
    """which quantiser an iteration uses: a single quantiser always; otherwise the first
    for the first third of max_iterations, the second for the second third, the last
    afterwards (rcq_decoder.py:156-167, 482-493)."""
    if n_quantizers == 1:
        return 0
    if iteration < max_iterations // 3:
        return 0
    if iteration < 2 * max_iterations // 3:
        return 1 if n_quantizers > 1 else 0
    return n_quantizers - 1


def _quantizer_schedule(n_quantizers: int, max_iterations: int) -> np.ndarray:
    T = int(max_iterations)
    out = np.zeros(max(T, 1), dtype=np.int32)
    for it in range(T):
        out[it] = _quantizer_index(n_quantizers, T, it)
    return out


def _threshold_table(quantizers) -> np.ndarray:
    return np.stack([q.thresholds_f32() for q in quantizers]).astype(np.float32)


def quantizer_param_grads(C, gamma, grad_table):
    """Chain rule from d J / d tau [Q, L] to the parameters of tau_j = C * x_j^gamma, x_j = j / (L - 1), in float64:
    d tau_j / d C = x_j^gamma (0^0 = 1, as the value path has it);  d tau_j / d gamma = C * x_j^gamma * ln x_j for
    1 <= j <= L - 2 and := 0 at j = 0 (the limit for gamma > 0; at gamma = 0 the derivative does not exist) and at
    j = L - 1 (ln 1).  -> (d J / d C [Q], d J / d gamma [Q]), torch float64 on the device of grad_table."""
    as64 = lambda v: v.detach().to(torch.float64) if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v, dtype=np.float64))
    g = as64(grad_table)
    C, gamma = as64(C).to(g.device).reshape(-1, 1), as64(gamma).to(g.device).reshape(-1, 1)
    L = g.shape[1]
    if L < 2:
        raise ValueError("a quantiser with one level has no (C, gamma) parametrisation")
    x = (torch.arange(L, dtype=torch.float64, device=g.device) / (L - 1)).reshape(1, -1)
    xg = x ** gamma
    lnx = torch.zeros_like(x)
    lnx[:, 1:L - 1] = torch.log(x[:, 1:L - 1])
    # j = 0 and j = L - 1 carry no gamma term: a `where`, not a product with 0 (x_0^gamma * ln x_0 is 0 * -inf)
    dgamma = torch.where(lnx != 0, C * xg * lnx, torch.zeros_like(xg))
    return (g * xg).sum(dim=1), (g * dgamma).sum(dim=1)


class _ThresholdTable(torch.autograd.Function):
    """(C [Q], gamma [Q], table [Q, L]) -> table: the VALUES are the reference's (float32 of Python-float arithmetic, handed
    in), the derivative is quantizer_param_grads"""

    @staticmethod
    def forward(ctx, C, gamma, table):
        ctx.save_for_backward(C, gamma)
        return table.clone()

    @staticmethod
    def backward(ctx, g):
        C, gamma = ctx.saved_tensors
        gC, gg = quantizer_param_grads(C, gamma, g)
        return gC.to(device=C.device, dtype=C.dtype), gg.to(device=gamma.device, dtype=gamma.dtype), None


class RCQMinSumDecoder:
    """RCQ MinSum decoder with non-uniform quantisation (flooding schedule)."""

    def __init__(self, code: LDPCCode, bc: int, bv: int, quantizer_params: List[Tuple[float, float]],
                 max_iterations: int = 50, layered: bool = False):
        self.code = code
        self.bc = bc
        self.bv = bv                      # stored, never used (as in the reference)
        self.max_iterations = max_iterations
        self.layered = layered
        self.quantizers = [NonUniformQuantizer(bc, C, gamma) for C, gamma in quantizer_params]
        self._engine = None
        self._engine_key = None
        logger.info(f"Initialized RCQ MinSum decoder: bc={bc}, bv={bv}, "
                    f"layered={layered}, {len(self.quantizers)} quantizers")

    def _get_quantizer(self, iteration: int) -> NonUniformQuantizer:
        return self.quantizers[_quantizer_index(len(self.quantizers), self.max_iterations, iteration)]

    def _get_engine(self, device):
        import _native as nat
        from engine import DecodeEngine, _require_gpu
        dev = _require_gpu(device)
        g = self.code.tanner_graph()
        T = int(self.max_iterations)
        thr = _threshold_table(self.quantizers)
        key = (dev.index, id(g), T, thr.tobytes(), self.layered if isinstance(self.layered, str) else bool(self.layered))
        if self._engine is None or self._engine_key != key:
            rows = max(T, 1)
            self._engine = DecodeEngine(
                g, dtype=torch.float32, c2v_form=nat.C2V_RCQ, iters=T, device=dev,
                schedule=(nat.SCHED_LAYERED if self.layered == "paper" else
                          nat.SCHED_LAYERED_REF if self.layered else nat.SCHED_FLOODING),
                beta=np.ones((rows, 1), np.float32), beta_slot=np.zeros(g.E, np.int32),     # prod(signs) * min
                alpha=np.ones((rows, 1), np.float32), alpha_slot=np.zeros(g.n, np.int32),   # llr + sum(others)
                thresholds=thr, q_of_iter=_quantizer_schedule(len(self.quantizers), T))
            self._engine_key = key
        return self._engine

    def decode(self, llr: torch.Tensor, early_stop: bool = True, device=None):
        """
        Args:
            llr: log-likelihood ratios from the channel (torch tensor), ``[n]`` or ``[B, n]``
        Returns:
            decoded_bits (int32), success (bool / bool[B]), iterations (int / int32[B])
        """
        if not isinstance(llr, torch.Tensor):
            raise TypeError("llr must be a torch.Tensor")    # the reference needs llr.device as well
        _, x, single = _as_batch(llr, self.code.n)
        eng = self._get_engine(x.device if x.is_cuda else device)
        if not x.is_cuda and x.shape[0] <= eng.HOST_BATCH_MAX:       # the reference's call shape: torch.ops.ldpc.decode_host
            res = eng.decode_host_op(x.detach().to(torch.float32), early_stop=early_stop, want_posterior=False)
        else:
            res = eng.decode_op(x.detach().to(device=eng.device, dtype=torch.float32), early_stop=early_stop,
                                want_posterior=False)
        out_dev = llr.device
        if single:
            return res.bits[0].to(out_dev), bool(res.success[0].item()), int(res.iterations[0].item())
        return res.bits.to(out_dev), res.success.to(out_dev), res.iterations.to(out_dev)


class WeightedRCQDecoder(_DegreeSharedDecoder):
    """Weighted RCQ decoder: degree-shared neural weights + RCQ quantisation."""

    def __init__(self, code: LDPCCode, bc: int, bv: int, quantizer_params: List[Tuple[float, float]],
                 weight_sharing_type: int = 2, max_iterations: int = 50, layered: bool = False, *,
                 quantizer_gradient=None, layered_gradient=None, learn_quantizer: bool = False):
        super().__init__()
        import autograd_bridge as ab
        self.bc = bc
        self.bv = bv
        self.layered = layered            # stored; forward ignores it like the reference's, except "paper" (module docstring)
        # how joint_posterior_loss differentiates the quantiser: None (it refuses) or "straight_through"
        self.quantizer_gradient = ab.check_quantizer_gradient(quantizer_gradient)
        # how joint_posterior_loss differentiates the layered schedule (layered="paper" only): None (it refuses) or "posterior_local"
        self.layered_gradient = ab.check_layered_gradient(layered_gradient, self._schedule_name())
        self.learn_quantizer = bool(learn_quantizer)
        if self.learn_quantizer:
            if bc < 2:
                raise ValueError(f"learn_quantizer=True needs bc >= 2 (bc = {bc} has one level and no (C, gamma) to learn)")
            self._quantizers, self._quantizer_key = None, None     # built from the parameter VALUES on demand
        else:
            self.quantizers = [NonUniformQuantizer(bc, C, gamma) for C, gamma in quantizer_params]
        self._init_sharing(code, weight_sharing_type, max_iterations)
        if self.learn_quantizer:                      # after the weights: their order in parameters() / state_dict stays
            self.quantizer_C = torch.nn.Parameter(torch.tensor([float(C) for C, _ in quantizer_params], dtype=torch.float64))
            self.quantizer_gamma = torch.nn.Parameter(torch.tensor([float(g) for _, g in quantizer_params], dtype=torch.float64))
        logger.info(f"Initialized Weighted RCQ decoder: bc={bc}, bv={bv}, "
                    f"weight_type={weight_sharing_type}, layered={layered}")

    @property
    def quantizers(self) -> List[NonUniformQuantizer]:
        """the quantisers of the decoder; with learn_quantizer the list built from the CURRENT values of quantizer_C /
        quantizer_gamma -- compared by value on every access, as _get_engine compares the weight tables (`p.data` writes
        leave no other trace)"""
        if not self.__dict__.get("learn_quantizer", False):
            return self.__dict__["_quantizers"]
        C = self.quantizer_C.detach().to("cpu", torch.float64).numpy()
        gamma = self.quantizer_gamma.detach().to("cpu", torch.float64).numpy()
        key = (C.tobytes(), gamma.tobytes())
        if self._quantizers is None or self._quantizer_key != key:
            for name, v in (("quantizer_C", C), ("quantizer_gamma", gamma)):
                if not np.all(np.isfinite(v)):
                    raise ValueError(f"{name} holds a non-finite value: {v.tolist()}")
            if np.any(gamma < 0):
                raise ValueError(f"quantizer_gamma holds a negative value ({gamma.tolist()}): tau_0 = C * 0^gamma would "
                                 "divide by zero")
            self._quantizers = [NonUniformQuantizer(self.bc, float(c), float(g)) for c, g in zip(C, gamma)]
            self._quantizer_key = key
        return self._quantizers

    @quantizers.setter
    def quantizers(self, value):
        if self.__dict__.get("learn_quantizer", False):
            raise AttributeError("the quantisers of a learn_quantizer decoder follow quantizer_C / quantizer_gamma")
        self.__dict__["_quantizers"] = value

    def __getstate__(self):
        state = super().__getstate__()
        if self.learn_quantizer:
            state.update(_quantizers=None, _quantizer_key=None)
        return state

    def _get_quantizer(self, iteration: int) -> NonUniformQuantizer:
        quantizers = self.quantizers
        return quantizers[_quantizer_index(len(quantizers), self.max_iterations, iteration)]

    def _get_engine(self, device):
        """the weights' engine cache; a learn_quantizer decoder also brings the engine's quantiser table up to the current
        parameter values -- into the same native decoder (DecodeEngine.set_quantizers), never a rebuild"""
        if not self.learn_quantizer:
            return super()._get_engine(device)
        thr = _threshold_table(self.quantizers)          # validates (C, gamma) before any device work
        eng = super()._get_engine(device)
        if not np.array_equal(eng.current_thresholds(), thr):
            eng.set_quantizers(thr)
        return eng

    def thresholds_tensor(self) -> torch.Tensor:
        """[Q, L] float64: the float32 table the engine decodes with, differentiable in quantizer_C / quantizer_gamma"""
        table = torch.from_numpy(_threshold_table(self.quantizers).astype(np.float64))
        return _ThresholdTable.apply(self.quantizer_C, self.quantizer_gamma, table)

    def _schedule(self) -> int:
        """message schedule of the engine: the paper's layered one for layered="paper", else flooding (the reference
        ignores ``layered`` here, rcq_decoder.py:377)"""
        import _native as nat
        return nat.SCHED_LAYERED if isinstance(self.layered, str) and self.layered == "paper" else nat.SCHED_FLOODING

    def _schedule_name(self) -> str:
        """the schedule in the min-sum decoders' words (autograd_bridge.check_layered_gradient)"""
        return "layered" if isinstance(self.layered, str) and self.layered == "paper" else "flooding"

    def _extra_key(self):
        # learned thresholds are no part of the engine's identity: they reach it through set_quantizers
        if self.learn_quantizer:
            return (len(self.quantizer_C), self.bc, self._schedule())
        return (_threshold_table(self.quantizers).tobytes(), self._schedule())

    def _engine_kwargs(self, layout, beta, alpha):
        import _native as nat
        return dict(c2v_form=nat.C2V_RCQ, schedule=self._schedule(), beta=beta, beta_slot=layout.beta_slot,
                    alpha=alpha, alpha_slot=layout.alpha_slot,
                    thresholds=_threshold_table(self.quantizers),
                    q_of_iter=_quantizer_schedule(len(self.quantizers), self.max_iterations))

    def joint_posterior_loss(self, llr, targets=None, iteration_weights=None, device=None, *, quantizer_gradient=None,
                             layered_gradient=None):
        """Posterior joint training of the quantised decoder.  ``quantizer_gradient`` (default: the constructor's) names
        the estimator the quantiser is differentiated with: None -- the RCQ quantiser passes no gradient, so there is
        nothing to train through (NotImplementedError); "straight_through" -- the decoder's own fixed-T decode
        with the loss of ``Neural2DMinSumDecoder.joint_posterior_loss`` and the rule of the module docstring.
        ``layered_gradient`` (default: the constructor's): ``layered="paper"`` trains only with "posterior_local" as well
        (NotImplementedError without it); any value but None on a flooding decoder is a ValueError.
        -> (loss 0-d, loss_per_iteration [T], bits int32, posterior of the last iteration)"""
        import autograd_bridge as ab
        how = ab.check_quantizer_gradient(self.quantizer_gradient if quantizer_gradient is None else quantizer_gradient)
        lay = ab.check_layered_gradient(self.layered_gradient if layered_gradient is None else layered_gradient,
                                        self._schedule_name())
        if how is None:
            raise NotImplementedError("WeightedRCQDecoder has no gradient path: the RCQ quantiser passes no gradient "
                                      "(quantizer_gradient=\"straight_through\" trains through it with that estimator)")
        if not isinstance(llr, torch.Tensor):
            raise TypeError("llr must be a torch.Tensor")
        ab.check_joint_args(self.code.n, int(self.max_iterations), llr, targets, iteration_weights)
        paper = self._schedule_name() == "layered"
        if paper and lay is None:
            raise NotImplementedError("WeightedRCQDecoder(layered=\"paper\") has no gradient path without "
                                      "layered_gradient=\"posterior_local\": the straight-through joint loss alone exists "
                                      "for the flooding schedule")
        eng = self._get_engine(llr.device if llr.is_cuda else device)
        bt, at = self._sharing_layout().tables_torch(self.beta_weights, self.alpha_weights, int(self.max_iterations),
                                                     self._beta_default, self._alpha_default)
        thr = self.thresholds_tensor() if self.learn_quantizer else None
        return ab.joint_loss_ste(bt, at, eng, llr, targets, iteration_weights, layered=paper, thresholds=thr)

    def forward(self, llr: torch.Tensor, early_stop: bool = True, device=None):
        """
        Returns:
            decoded_bits (int32), posterior (float32), iterations (int / int32[B])
        """
        res, single, out_dev = self._decode(llr, early_stop, device)
        if single:
            return res.bits[0].to(out_dev), res.posterior[0].to(out_dev), int(res.iterations[0].item())
        return res.bits.to(out_dev), res.posterior.to(out_dev), res.iterations.to(out_dev)
