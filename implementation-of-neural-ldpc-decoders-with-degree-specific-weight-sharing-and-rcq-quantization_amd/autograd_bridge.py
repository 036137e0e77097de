"""
torch.autograd bridge of the gradient path: makes ``loss.backward()`` work on the posterior the
normalised min-sum decoders return, the way it does in the reference where ``forward`` is a chain of
differentiable torch operations on ``nn.Parameter``s (neural_2d_decoder.py:133-225; used by
training_framework.py:127-134 and :322-324).

The weight tables are assembled from the ``ParameterDict`` entries with differentiable torch
operations (``cat`` / ``index_put``) and handed to the registered operator
``torch.ops.ldpc.minsum_decode_train`` (torch_ops.py), so autograd itself routes the table gradients
the HIP backward sweeps return (include/ldpc_hip.h: ldpc_decode_saving / ldpc_backward) to the
individual parameters.
Parameters that do not influence the returned posterior get a zero gradient (the reference leaves
``.grad`` at None for them).

No CPU fallback: without the native engine ``forward`` raises like every other decode call.
"""

from __future__ import annotations

import logging
import os

import numpy as np
import torch

logger = logging.getLogger(__name__)

# forward state kept for backward is (2T-1)*E*4 bytes per codeword; above this many bytes the decoders
# return a posterior without grad_fn (and say so once) instead of exhausting HBM
MAX_SAVED_BYTES = int(os.environ.get("LDPC_TRAIN_MAX_SAVED_BYTES", str(8 << 30)))
_warned = False


def wants_grad(module: torch.nn.Module, llr=None) -> bool:
    if not torch.is_grad_enabled():
        return False
    if isinstance(llr, torch.Tensor) and llr.requires_grad:
        return True
    return any(p.requires_grad for p in module.parameters())


def saved_state_fits(engine, batch: int) -> bool:
    global _warned
    need = engine.train_saved_bytes(batch)
    if need <= MAX_SAVED_BYTES:
        return True
    if not _warned:
        _warned = True
        logger.warning("decode of %d codewords under autograd would keep %.1f GiB of messages for backward "
                       "(limit LDPC_TRAIN_MAX_SAVED_BYTES = %.1f GiB): returning a posterior without grad_fn; "
                       "wrap inference in torch.no_grad() or train on smaller batches",
                       batch, need / 2**30, MAX_SAVED_BYTES / 2**30)
    return False


def decode_train(beta_table: torch.Tensor, alpha_table: torch.Tensor, engine, x: torch.Tensor, early_stop: bool,
                 alpha_is_oms: bool = False):
    """(beta_table [T, Sb], alpha_table [T, Sa], llr x [B, n]) -> (posterior [B, n], bits, iterations) through the
    registered operator ``torch.ops.ldpc.minsum_decode_train`` (torch_ops.py): its autograd formula runs the HIP
    backward sweeps (``torch.ops.ldpc.minsum_backward``) and returns d loss/d beta, d loss/d alpha and -- when `x`
    requires grad (a trainable front end feeding the decoder) -- d loss/d llr from the same sweep.
    `alpha_is_oms`: the alpha table is the check-side offset of the offset decoders (engine slot oms_alpha),
    otherwise the variable-side multiplier (engine slot alpha)."""
    import torch_ops
    xd = x.to(device=engine.device, dtype=torch.float32)       # differentiable: the LLR gradient flows back through it
    if not x.requires_grad:
        xd = xd.detach()
    post, bits, iters, _saved = torch.ops.ldpc.minsum_decode_train(xd.contiguous(), beta_table, alpha_table,
                                                                  torch_ops.engine_handle(engine), bool(early_stop),
                                                                  bool(alpha_is_oms))
    return post, bits, iters


def table_from_params(params, where, shape, default: float) -> torch.Tensor:
    """Differentiable [rows, cols] table: `default` everywhere, params[k] (shape [1]) at where[k] = (row, col)"""
    out = torch.full(shape, float(default), dtype=torch.float32)
    if not params:
        return out
    vals = torch.cat([p.reshape(-1)[:1] for p in params]).to("cpu", torch.float32)
    rr = torch.tensor([w[0] for w in where], dtype=torch.long)
    cc = torch.tensor([w[1] for w in where], dtype=torch.long)
    return out.index_put((rr, cc), vals)


def check_joint_args(n: int, T: int, llr, targets, iteration_weights):
    """shape checks of joint_posterior_loss (before any device work): ValueError on a mismatch"""
    shape = tuple(llr.shape)
    if len(shape) not in (1, 2) or shape[-1] != n:
        raise ValueError(f"llr must have shape [n] or [B, n] with n = {n}, got {shape}")
    if targets is not None and tuple(targets.shape) != shape:
        raise ValueError(f"targets must have the shape of llr {shape}, got {tuple(targets.shape)}")
    if iteration_weights is not None and tuple(torch.as_tensor(iteration_weights).shape) != (T,):
        raise ValueError(f"iteration_weights must have shape ({T},), got {tuple(torch.as_tensor(iteration_weights).shape)}")
    if T < 1:
        raise ValueError("the joint posterior loss needs max_iterations >= 1")


QUANTIZER_GRADIENTS = ("straight_through",)


def check_quantizer_gradient(value):
    """the estimators joint_posterior_loss of the quantised decoder knows: None (no gradient path) or one of
    QUANTIZER_GRADIENTS; ValueError otherwise"""
    if value is not None and value not in QUANTIZER_GRADIENTS:
        raise ValueError(f"quantizer_gradient must be None or one of {QUANTIZER_GRADIENTS}, got {value!r}")
    return value


LAYERED_GRADIENTS = ("posterior_local",)


def check_layered_gradient(value, schedule="layered"):
    """the gradients joint_posterior_loss of a ``schedule="layered"`` decoder (min-sum, or W-RCQ ``layered="paper"``) knows: None (no gradient path) or one
    of LAYERED_GRADIENTS; ValueError otherwise, and for any value but None on a flooding decoder (nothing to choose there)"""
    if value is not None and value not in LAYERED_GRADIENTS:
        raise ValueError(f"layered_gradient must be None or one of {LAYERED_GRADIENTS}, got {value!r}")
    if value is not None and schedule != "layered":
        raise ValueError(f"layered_gradient={value!r} applies to schedule=\"layered\" only, this decoder runs {schedule!r}")
    return value


def joint_loss_ste(beta_table: torch.Tensor, alpha_table: torch.Tensor, engine, llr: torch.Tensor, targets,
                   iteration_weights, layered: bool = False, thresholds=None):
    """joint_loss() of the quantised WeightedRCQDecoder through ``torch.ops.ldpc.rcq_joint_loss``: the same loss on the
    decoder's own fixed-T decode, differentiable with the straight-through rule of include/ldpc_hip.h
    (ldpc_train_joint_ste) -> (loss, loss_per_iteration, bits, posterior).  ``layered``: the engine runs the paper's
    layered schedule -- ``torch.ops.ldpc.rcq_layered_joint_loss`` (ldpc_train_joint_layered_ste).
    ``thresholds`` [Q, L] (a learned quantiser, rcq_decoder.WeightedRCQDecoder.thresholds_tensor): the call goes through
    ``torch.ops.ldpc.rcq_joint_loss_levels`` / ``rcq_layered_joint_loss_levels``, which decode with that table and whose
    backward sums the level gradients [T, L] per quantiser (the engine's q_of_iter) into d loss / d thresholds."""
    return joint_loss(beta_table, alpha_table, engine, llr, targets, iteration_weights, False, quantised=True, layered=layered,
                      thresholds=thresholds)


def joint_loss(beta_table: torch.Tensor, alpha_table: torch.Tensor, engine, llr: torch.Tensor, targets, iteration_weights,
               alpha_is_oms: bool, quantised: bool = False, layered: bool = False, thresholds=None):
    """posterior joint training through ``torch.ops.ldpc.minsum_joint_loss`` (torch_ops.py) -> (loss, loss_per_iteration,
    bits, posterior): loss = sum_t w_t * mean BCEWithLogits(-posterior_t, targets) over the T iterations of the fixed-T
    decode, differentiable in the tables (and in `llr` when it requires grad) with the posterior-local gradient of the
    paper's training method.  No saved history: MAX_SAVED_BYTES does not apply.
    ``layered``: the engine runs the layered schedule -- ``torch.ops.ldpc.minsum_layered_joint_loss``, whose gradient is the
    layered posterior-local one of include/ldpc_hip.h (ldpc_train_joint_layered); with ``quantised``
    ``torch.ops.ldpc.rcq_layered_joint_loss`` (ldpc_train_joint_layered_ste)."""
    import torch_ops
    from ldpc_decoder import _as_batch
    T = int(engine.iters)
    check_joint_args(engine.graph.n, T, llr, targets, iteration_weights)
    _, x, single = _as_batch(llr, engine.graph.n)
    xd = x.to(device=engine.device, dtype=torch.float32)
    grad_on = torch.is_grad_enabled()
    want_llr = grad_on and x.requires_grad
    if not want_llr:
        xd = xd.detach()
    want_grads = grad_on and (beta_table.requires_grad or alpha_table.requires_grad)
    y = None
    if targets is not None:
        y = torch.as_tensor(targets).detach().to(device=engine.device, dtype=torch.float32).reshape(xd.shape).contiguous()
    w = (torch.full((T,), 1.0 / T, dtype=torch.float32) if iteration_weights is None
         else torch.as_tensor(iteration_weights).detach().to(torch.float32))
    w = w.to(engine.device).contiguous()
    op, form = ((torch.ops.ldpc.rcq_layered_joint_loss if layered else torch.ops.ldpc.rcq_joint_loss, ())
                if quantised else                                               # the quantised operators have no alpha_is_oms
                (torch.ops.ldpc.minsum_layered_joint_loss if layered else torch.ops.ldpc.minsum_joint_loss, (bool(alpha_is_oms),)))
    if thresholds is not None:
        if not quantised:
            raise ValueError("thresholds belong to the quantised decoders")
        op = torch.ops.ldpc.rcq_layered_joint_loss_levels if layered else torch.ops.ldpc.rcq_joint_loss_levels
        loss, lpi, post, bits = op(xd.contiguous(), y, beta_table, alpha_table, thresholds, w, torch_ops.engine_handle(engine),
                                   bool(want_grads), bool(want_llr))[:4]
    else:
        loss, lpi, post, bits, _gb, _ga, _gl = op(xd.contiguous(), y, beta_table, alpha_table, w,
                                                  torch_ops.engine_handle(engine), *form, bool(want_grads), bool(want_llr))
    out_dev = llr.device
    if single:
        bits, post = bits[0], post[0]
    return loss.to(out_dev), lpi.to(out_dev), bits.to(out_dev), post.to(out_dev)
