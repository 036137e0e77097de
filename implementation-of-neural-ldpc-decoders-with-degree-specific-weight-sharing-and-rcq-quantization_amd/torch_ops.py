"""
PyTorch operator registration of the decode path (BASELINE.json north_star: "Python host code calling
hand-written CDNA4 HIP kernels through PyTorch-ROCm custom ops").

The reference has no operator registry -- its decoders are Python loops behind
``decoder.decode(llr)`` / ``decoder(llr)`` (ldpc_decoder.py:63, neural_2d_decoder.py:133,
rcq_decoder.py:169, :495).  Here those methods end in ``torch.ops.ldpc.*`` calls, which in turn
enter the C ABI of include/ldpc_hip.h (ldpc_decode / ldpc_decode_saving / ldpc_backward):

  ldpc::decode(Tensor llr, int engine, bool early_stop, bool want_posterior, bool want_packed)
        -> (Tensor bits, Tensor posterior, Tensor iterations, Tensor success, Tensor packed_bits)
     every decoder family (the engine handle carries the descriptor: C2V rule, tables, quantisers);
     outputs that were not asked for come back as empty tensors.  No autograd (inference).
  ldpc::decode_host(Tensor llr_cpu, int engine, bool early_stop, bool want_posterior)
        -> (Tensor bits, Tensor posterior, Tensor iterations, Tensor success)      all on the CPU
     the reference's own call shape (one vector, or a batch of at most 64, in host memory): one staged async copy
     each way around the same ldpc_decode.
  ldpc::minsum_decode_train(Tensor llr, Tensor beta, Tensor alpha, int engine, bool early_stop, bool alpha_is_oms)
        -> (Tensor posterior, Tensor bits, Tensor iterations, Tensor saved)
     the same decode keeping every iteration's messages (`saved`) for the backward sweeps; differentiable in
     beta [T, Sb], alpha [T, Sa] and llr through register_autograd, whose backward is
  ldpc::minsum_backward(Tensor saved, Tensor llr, Tensor iterations, Tensor grad_posterior, Tensor beta,
                        Tensor alpha, int engine, bool alpha_is_oms, bool want_grad_llr)
        -> (Tensor grad_beta, Tensor grad_alpha, Tensor grad_llr)
  ldpc::minsum_joint_loss(Tensor llr, Tensor? targets, Tensor beta, Tensor alpha, Tensor iteration_weights, int engine,
                          bool alpha_is_oms, bool want_grads=True, bool want_grad_llr=False)
        -> (Tensor loss, Tensor loss_per_iter, Tensor posterior, Tensor bits, Tensor grad_beta, Tensor grad_alpha,
            Tensor grad_llr)
     posterior joint training (ldpc_train_joint): the fixed-T decode with loss = sum_t w_t * BCE of iteration t's
     posterior, whose gradients the forward already formed (no saved history); differentiable in `loss` only, the
     backward scales the last three outputs (and d loss/d w_t = loss_per_iter[t]).

  ldpc::rcq_joint_loss(Tensor llr, Tensor? targets, Tensor beta, Tensor alpha, Tensor iteration_weights, int engine,
                       bool want_grads=True, bool want_grad_llr=False)
        -> the same seven outputs
     the same for the quantised WeightedRCQDecoder (ldpc_train_joint_ste): the forward is its fixed-T flooding decode
     bit for bit; the gradients treat the quantiser with the straight-through rule -- d c2v/d m := 1 where the code the
     forward wrote lies below the top level (the dead zone included), 0 where it saturated, m = beta * sign product * min.

  ldpc::minsum_layered_joint_loss(... the arguments of minsum_joint_loss ...) -> the same seven outputs
     the same for a min-sum decoder under ``schedule="layered"`` (ldpc_train_joint_layered): the forward is its fixed-T layered
     decode bit for bit; the gradients are layered posterior-local -- iteration t's loss reaches beta_t, the check-side offset
     alpha_t and the LLRs through the check update that wrote each message, the variable's other messages held constant.  The
     variable-side alpha of the normalised form is not used by the schedule: its gradient is all zero.

  ldpc::rcq_layered_joint_loss(... the arguments of rcq_joint_loss ...) -> the same seven outputs
     the same for ``WeightedRCQDecoder(layered="paper")`` (ldpc_train_joint_layered_ste): the forward is its fixed-T layered decode
     bit for bit; the gradients are layered posterior-local with the straight-through rule on the code each check update wrote.
     alpha is not used by the schedule: its gradient is all zero.

  ldpc::rcq_joint_loss_levels(Tensor llr, Tensor? targets, Tensor beta, Tensor alpha, Tensor thresholds,
                              Tensor iteration_weights, int engine, bool want_grads=True, bool want_grad_llr=False)
        -> the seven outputs of rcq_joint_loss and Tensor grad_levels
  ldpc::rcq_layered_joint_loss_levels(... the same arguments ...) -> the same eight outputs
     rcq_joint_loss / rcq_layered_joint_loss with the quantiser as an input (ldpc_train_joint_ste_levels,
     ldpc_train_joint_layered_ste_levels): `thresholds` [Q, L] is the table the decode runs with (the engine's own is put back
     afterwards when it differs) and is differentiable -- grad_levels [T, L] fp32 holds d loss / d (reconstruction value of
     level l) of iteration t, the signed per-level sum of the loss seed over the codes the forward stored, and the backward
     sums its rows per quantiser (the engine's q_of_iter) into d loss / d thresholds.  The thresholds as decision boundaries
     pass no gradient (straight-through).  The first seven outputs equal the base operator's bit for bit.

  ldpc::awgn_llr(int batch, int n, int seed, int stream_id, int first_frame, float scale, float shift, Tensor? codeword_packed,
                 Device device) -> Tensor llr
     the counter-based BI-AWGN channel (ldpc_channel_awgn): fp32 LLRs [batch, n] of frames first_frame .. of stream
     (seed, stream_id), the same whatever block a frame is drawn in; needs no engine.
  ldpc::sym_llr(int batch, int n, int seed, int stream_id, int first_frame, str scheme, bool rayleigh, float amp,
                Tensor? interleaver, Tensor? codeword_packed, Device device) -> Tensor llr
     the symbol channel (ldpc_channel_sym): max-log LLRs of Gray-mapped "bpsk" / "qpsk" / "qam16" / "qam64" / "qam256" symbols
     over AWGN or per-symbol Rayleigh fading; codeword_packed is one packed word or [batch, ceil(n/8)] rows; needs no engine.
  ldpc::awgn_llr_mix(int batch, int n, int seed, int stream_id, int first_frame, Tensor scale_tab, Tensor shift_tab,
                     Tensor? codeword_packed, Device device) -> Tensor llr
     the same stream with the SNR point a function of the frame (ldpc_channel_awgn_mix): frame f is drawn with
     (scale_tab[p], shift_tab[p]), p = f % K, of two float32 tables of K entries on the device.

``engine`` is an integer handle of a live ``engine.DecodeEngine`` (``engine_handle(eng)``): operator schemas
carry tensors and scalars, and the native decoder handle is neither.  There is no CPU implementation: the
ops exist for ROCm tensors only and fail loudly otherwise (no fallback).
"""

from __future__ import annotations

import threading
import weakref
from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor

_engines = weakref.WeakValueDictionary()
_lock = threading.Lock()
_next = [1]


def engine_handle(eng) -> int:
    """integer handle under which `eng` is known to the ops (stable for the engine's lifetime)"""
    h = getattr(eng, "_op_handle", None)
    if h is None:
        with _lock:
            h = _next[0]
            _next[0] += 1
            _engines[h] = eng
        eng._op_handle = h
    return h


def _engine(handle: int):
    eng = _engines.get(int(handle))
    if eng is None:
        raise RuntimeError(f"ldpc ops: no live decode engine with handle {handle}")
    return eng


def _empty(dev, dtype=torch.uint8):
    return torch.empty((0,), dtype=dtype, device=dev)


# ------------------------------------------------------------------------------------------ inference
@torch.library.custom_op("ldpc::decode", mutates_args=())
def decode(llr: Tensor, engine: int, early_stop: bool, want_posterior: bool,
           want_packed: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    eng = _engine(engine)
    res = eng.decode(llr, early_stop=early_stop, want_bits=True, want_posterior=want_posterior, want_packed=want_packed)
    dev = llr.device
    return (res.bits, res.posterior if want_posterior else _empty(dev, llr.dtype), res.iterations, res.success,
            res.packed_bits if want_packed else _empty(dev))


@decode.register_fake
def _(llr, engine, early_stop, want_posterior, want_packed):
    B, n = llr.shape
    dev = llr.device
    return (torch.empty((B, n), dtype=torch.int32, device=dev),
            torch.empty((B, n), dtype=llr.dtype, device=dev) if want_posterior else torch.empty((0,), dtype=llr.dtype, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B,), dtype=torch.bool, device=dev),
            torch.empty((B, (n + 7) // 8), dtype=torch.uint8, device=dev) if want_packed else torch.empty((0,), dtype=torch.uint8, device=dev))


@torch.library.custom_op("ldpc::decode_host", mutates_args=())
def decode_host(llr: Tensor, engine: int, early_stop: bool, want_posterior: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """the reference's call shape -- a small batch in HOST memory, results back in host memory -- through one staged
    copy each way (engine.DecodeEngine.decode_host); still the GPU engine, there is no CPU arithmetic"""
    eng = _engine(engine)
    bits, post, iters, succ = eng.decode_host(llr.to(eng.dtype), early_stop=early_stop, want_posterior=want_posterior)
    return bits, post if want_posterior else torch.empty((0,), dtype=eng.dtype), iters, succ


@decode_host.register_fake
def _(llr, engine, early_stop, want_posterior):
    B, n = llr.shape
    dt = _engine(engine).dtype
    return (torch.empty((B, n), dtype=torch.int32), torch.empty((B, n), dtype=dt) if want_posterior else torch.empty((0,), dtype=dt),
            torch.empty((B,), dtype=torch.int32), torch.empty((B,), dtype=torch.bool))


@torch.library.custom_op("ldpc::awgn_llr", mutates_args=())
def awgn_llr(batch: int, n: int, seed: int, stream_id: int, first_frame: int, scale: float, shift: float,
             codeword_packed: Optional[Tensor], device: torch.device) -> Tensor:
    import engine
    return engine.awgn_llr(batch, n, seed=seed, stream_id=stream_id, first_frame=first_frame, scale=scale, shift=shift,
                           codeword=codeword_packed, device=device)


@awgn_llr.register_fake
def _(batch, n, seed, stream_id, first_frame, scale, shift, codeword_packed, device):
    return torch.empty((batch, n), dtype=torch.float32, device=device)


@torch.library.custom_op("ldpc::sym_llr", mutates_args=())
def sym_llr(batch: int, n: int, seed: int, stream_id: int, first_frame: int, scheme: str, rayleigh: bool, amp: float,
            interleaver: Optional[Tensor], codeword_packed: Optional[Tensor], device: torch.device) -> Tensor:
    import engine
    from modulation import Modulation
    mod = Modulation(scheme, "rayleigh" if rayleigh else None,
                     None if interleaver is None else interleaver.detach().cpu().numpy())
    return engine.sym_llr(batch, n, seed=seed, stream_id=stream_id, first_frame=first_frame, modulation=mod, amp=amp,
                          codeword=codeword_packed, device=device)


@sym_llr.register_fake
def _(batch, n, seed, stream_id, first_frame, scheme, rayleigh, amp, interleaver, codeword_packed, device):
    return torch.empty((batch, n), dtype=torch.float32, device=device)


@torch.library.custom_op("ldpc::awgn_llr_mix", mutates_args=())
def awgn_llr_mix(batch: int, n: int, seed: int, stream_id: int, first_frame: int, scale_tab: Tensor, shift_tab: Tensor,
                 codeword_packed: Optional[Tensor], device: torch.device) -> Tensor:
    import engine
    return engine.awgn_llr_mix(batch, n, seed=seed, stream_id=stream_id, first_frame=first_frame, scale=scale_tab,
                               shift=shift_tab, codeword=codeword_packed, device=device)


@awgn_llr_mix.register_fake
def _(batch, n, seed, stream_id, first_frame, scale_tab, shift_tab, codeword_packed, device):
    return torch.empty((batch, n), dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------ training path
def _np_table(t: Tensor) -> np.ndarray:
    return t.detach().to("cpu", torch.float32).numpy().copy()


def _with_tables(eng, beta: np.ndarray, alpha: np.ndarray, alpha_is_oms: bool):
    """make the device tables equal (beta, alpha) for the duration of a call; returns a restore() closure.
    (A backward may run after the parameters moved on: the sweep must see the tables its forward used.)"""
    held = eng.current_tables()
    held_alpha = held[2] if alpha_is_oms else held[1]
    same = np.array_equal(held[0], beta) and (held_alpha is None or np.array_equal(held_alpha, alpha))

    def upload(b, a):
        if alpha_is_oms:
            eng.set_weights(b, None, a if eng.current_tables()[2] is not None else None)
        else:
            eng.set_weights(b, a)

    if same:
        return lambda: None
    upload(beta, alpha)
    return lambda: upload(held[0], held_alpha)


@torch.library.custom_op("ldpc::minsum_decode_train", mutates_args=())
def minsum_decode_train(llr: Tensor, beta: Tensor, alpha: Tensor, engine: int, early_stop: bool,
                        alpha_is_oms: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    eng = _engine(engine)
    restore = _with_tables(eng, _np_table(beta), _np_table(alpha), alpha_is_oms)
    try:
        res, saved = eng.decode_saving(llr.detach(), early_stop=early_stop)
    finally:
        restore()
    return res.posterior, res.bits, res.iterations, saved


@minsum_decode_train.register_fake
def _(llr, beta, alpha, engine, early_stop, alpha_is_oms):
    B, n = llr.shape
    dev = llr.device
    nbytes = _engine(engine).train_saved_bytes(int(B)) if not isinstance(B, torch.SymInt) else torch.library.get_ctx().new_dynamic_size()
    return (torch.empty((B, n), dtype=torch.float32, device=dev), torch.empty((B, n), dtype=torch.int32, device=dev),
            torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((nbytes,), dtype=torch.uint8, device=dev))


@torch.library.custom_op("ldpc::minsum_backward", mutates_args=())
def minsum_backward(saved: Tensor, llr: Tensor, iterations: Tensor, grad_posterior: Tensor, beta: Tensor, alpha: Tensor,
                    engine: int, alpha_is_oms: bool, want_grad_llr: bool) -> Tuple[Tensor, Tensor, Tensor]:
    eng = _engine(engine)
    restore = _with_tables(eng, _np_table(beta), _np_table(alpha), alpha_is_oms)
    try:
        if want_grad_llr:
            gb, ga, goa, gl = eng.backward(saved, llr, iterations, grad_posterior, want_grad_llr=True)
        else:
            gb, ga, goa = eng.backward(saved, llr, iterations, grad_posterior)
            gl = torch.empty((0,), dtype=torch.float32, device=llr.device)
    finally:
        restore()
    if alpha_is_oms:
        ga = goa if goa is not None else torch.zeros(tuple(alpha.shape), dtype=torch.float32, device=gb.device)
    return gb.to(device=beta.device, dtype=beta.dtype), ga.to(device=alpha.device, dtype=alpha.dtype), gl


@minsum_backward.register_fake
def _(saved, llr, iterations, grad_posterior, beta, alpha, engine, alpha_is_oms, want_grad_llr):
    return (torch.empty_like(beta), torch.empty_like(alpha),
            torch.empty_like(llr, dtype=torch.float32) if want_grad_llr else torch.empty((0,), dtype=torch.float32, device=llr.device))


def _train_setup(ctx, inputs, output):
    llr, beta, alpha, engine, early_stop, alpha_is_oms = inputs
    _post, _bits, iters, saved = output
    ctx.engine, ctx.alpha_is_oms = engine, alpha_is_oms
    # the handle table holds engines weakly; the autograd node keeps ITS engine alive until the graph is freed (the
    # decoder may be rebuilt or go out of scope between forward and backward -- the reference's graph is self-contained)
    ctx._engine_obj = _engine(engine)
    ctx.save_for_backward(saved, llr, iters, beta, alpha)
    ctx.set_materialize_grads(False)


def _train_backward(ctx, g_post, _g_bits, _g_iters, _g_saved):
    saved, llr, iters, beta, alpha = ctx.saved_tensors
    if g_post is None:
        return None, None, None, None, None, None
    want_llr = bool(ctx.needs_input_grad[0])
    gb, ga, gl = torch.ops.ldpc.minsum_backward(saved, llr, iters, g_post.contiguous(), beta, alpha, ctx.engine,
                                                ctx.alpha_is_oms, want_llr)
    return (gl if want_llr else None), gb, ga, None, None, None


minsum_decode_train.register_autograd(_train_backward, setup_context=_train_setup)


# ------------------------------------------------------------------------------------------ posterior joint training
def _with_thresholds(eng, thresholds: np.ndarray):
    """_with_tables for the quantiser table of an RCQ engine"""
    held = eng.current_thresholds()
    if held is None:
        raise NotImplementedError("ldpc ops: the engine has no quantiser (RCQ decoders only)")
    if np.array_equal(held, thresholds):
        return lambda: None
    eng.set_quantizers(thresholds)
    return lambda: eng.set_quantizers(held)


def _joint(llr, targets, beta, alpha, iteration_weights, engine, alpha_is_oms, want_grads, want_grad_llr, method,
           thresholds=None):
    """the joint-loss operators; `method`: the engine's train_joint | train_joint_ste | train_joint_layered |
    train_joint_layered_ste.  `thresholds` (the two ..._levels operators): the quantiser table of the call; the result
    gains grad_levels [T, L] -- formed whenever the table is given, it is what the operator exists for"""
    eng = _engine(engine)
    restore_q = (lambda: None) if thresholds is None else _with_thresholds(eng, _np_table(thresholds))
    try:
        restore = _with_tables(eng, _np_table(beta), _np_table(alpha), alpha_is_oms)
        try:
            extra = {} if thresholds is None else {"want_levels": True}
            r = getattr(eng, method)(llr.detach(), None if targets is None else targets.detach(), iteration_weights.detach(),
                                     want_grads=want_grads, want_grad_llr=want_grad_llr, **extra)
        finally:
            restore()
    finally:
        restore_q()
    dev = llr.device
    if want_grads:
        gb = r["grad_beta"].to(device=beta.device, dtype=beta.dtype)
        ga = r["grad_oms_alpha"] if alpha_is_oms else r["grad_alpha"]
        ga = (torch.zeros(tuple(alpha.shape), dtype=alpha.dtype, device=alpha.device) if ga is None
              else ga.to(device=alpha.device, dtype=alpha.dtype))
    else:
        gb, ga = torch.empty((0,), dtype=beta.dtype, device=beta.device), torch.empty((0,), dtype=alpha.dtype, device=alpha.device)
    gl = r["grad_llr"] if want_grad_llr else torch.empty((0,), dtype=torch.float32, device=dev)
    if thresholds is not None:
        return r["loss"], r["loss_per_iter"], r["posterior"], r["bits"], gb, ga, gl, r["grad_levels"]
    return r["loss"], r["loss_per_iter"], r["posterior"], r["bits"], gb, ga, gl


@torch.library.custom_op("ldpc::minsum_joint_loss", mutates_args=())
def minsum_joint_loss(llr: Tensor, targets: Optional[Tensor], beta: Tensor, alpha: Tensor, iteration_weights: Tensor,
                      engine: int, alpha_is_oms: bool, want_grads: bool = True,
                      want_grad_llr: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """fixed-T decode with the loss on every iteration's posterior (ldpc_train_joint):
    loss = sum_t w_t J_t, loss_per_iter = J_t, posterior / bits of the last iteration, and the gradients of `loss`
    the autograd formula scales: d loss/d beta [T, Sb], d loss/d alpha [T, Sa] (alpha_is_oms: the check-side offset)
    -- empty when not want_grads -- and d loss/d llr [B, n] (empty when not want_grad_llr)"""
    return _joint(llr, targets, beta, alpha, iteration_weights, engine, alpha_is_oms, want_grads, want_grad_llr, "train_joint")


@torch.library.custom_op("ldpc::minsum_layered_joint_loss", mutates_args=())
def minsum_layered_joint_loss(llr: Tensor, targets: Optional[Tensor], beta: Tensor, alpha: Tensor, iteration_weights: Tensor,
                              engine: int, alpha_is_oms: bool, want_grads: bool = True,
                              want_grad_llr: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """minsum_joint_loss of a decoder under the layered schedule (ldpc_train_joint_layered): the fixed-T layered decode, its
    per-iteration loss, and the layered posterior-local gradients d loss/d beta [T, Sb], d loss/d alpha [T, Sa]
    (alpha_is_oms: the check-side offset; otherwise the unused variable-side table, all zero), d loss/d llr [B, n]"""
    return _joint(llr, targets, beta, alpha, iteration_weights, engine, alpha_is_oms, want_grads, want_grad_llr,
                  "train_joint_layered")


@torch.library.custom_op("ldpc::rcq_joint_loss", mutates_args=())
def rcq_joint_loss(llr: Tensor, targets: Optional[Tensor], beta: Tensor, alpha: Tensor, iteration_weights: Tensor,
                   engine: int, want_grads: bool = True,
                   want_grad_llr: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """minsum_joint_loss of the quantised decoder (ldpc_train_joint_ste): the fixed-T W-RCQ decode, its per-iteration
    loss, and the straight-through gradients d loss/d beta [T, Sb], d loss/d alpha [T, Sa] (variable side),
    d loss/d llr [B, n]"""
    return _joint(llr, targets, beta, alpha, iteration_weights, engine, False, want_grads, want_grad_llr, "train_joint_ste")


@torch.library.custom_op("ldpc::rcq_layered_joint_loss", mutates_args=())
def rcq_layered_joint_loss(llr: Tensor, targets: Optional[Tensor], beta: Tensor, alpha: Tensor, iteration_weights: Tensor,
                           engine: int, want_grads: bool = True,
                           want_grad_llr: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """rcq_joint_loss of the quantised decoder under the paper's layered schedule (ldpc_train_joint_layered_ste): the fixed-T
    layered W-RCQ decode, its per-iteration loss, and the layered straight-through gradients d loss/d beta [T, Sb],
    d loss/d alpha [T, Sa] (the unused table, all zero), d loss/d llr [B, n]"""
    return _joint(llr, targets, beta, alpha, iteration_weights, engine, False, want_grads, want_grad_llr,
                  "train_joint_layered_ste")


@minsum_layered_joint_loss.register_fake
@minsum_joint_loss.register_fake
def _joint_fake(llr, targets, beta, alpha, iteration_weights, engine, alpha_is_oms, want_grads=True, want_grad_llr=False):
    B, n = llr.shape
    dev = llr.device
    T = iteration_weights.shape[0]
    return (torch.empty((), dtype=torch.float32, device=dev), torch.empty((T,), dtype=torch.float32, device=dev),
            torch.empty((B, n), dtype=torch.float32, device=dev), torch.empty((B, n), dtype=torch.int32, device=dev),
            torch.empty_like(beta) if want_grads else torch.empty((0,), dtype=beta.dtype, device=beta.device),
            torch.empty_like(alpha) if want_grads else torch.empty((0,), dtype=alpha.dtype, device=alpha.device),
            torch.empty((B, n), dtype=torch.float32, device=dev) if want_grad_llr
            else torch.empty((0,), dtype=torch.float32, device=dev))


# the dispatcher drops trailing arguments that equal their defaults, so a fake cannot read the two flags from the tail of
# *args without knowing whether alpha_is_oms (no default) precedes them: the quantised operators, which have none, bind their
# own signature and call the one fake
@rcq_layered_joint_loss.register_fake
@rcq_joint_loss.register_fake
def _(llr, targets, beta, alpha, iteration_weights, engine, want_grads=True, want_grad_llr=False):
    return _joint_fake(llr, targets, beta, alpha, iteration_weights, engine, False, want_grads, want_grad_llr)


def _joint_setup(ctx, inputs, output):
    ctx.want_grads, ctx.want_grad_llr = inputs[-2:]
    ctx.n_inputs = len(inputs)
    _loss, lpi, post, bits, gb, ga, gl = output
    ctx.save_for_backward(lpi, gb, ga, gl)
    # only the scalar loss is differentiable: the gradients above are d loss / d input
    ctx.mark_non_differentiable(lpi, post, bits, gb, ga, gl)
    ctx.set_materialize_grads(False)


def _joint_backward(ctx, g_loss, *_unused):
    lpi, gb, ga, gl = ctx.saved_tensors
    if g_loss is None:
        return (None,) * ctx.n_inputs
    # J is linear in its seed: the saved gradients of `loss` scale by the incoming gradient
    g_beta = gb * g_loss.to(gb.device) if ctx.want_grads and ctx.needs_input_grad[2] else None
    g_alpha = ga * g_loss.to(ga.device) if ctx.want_grads and ctx.needs_input_grad[3] else None
    g_llr = gl * g_loss if ctx.want_grad_llr and ctx.needs_input_grad[0] else None
    g_w = lpi * g_loss if ctx.needs_input_grad[4] else None          # d loss / d w_t = J_t
    return (g_llr, None, g_beta, g_alpha, g_w) + (None,) * (ctx.n_inputs - 5)    # engine and the flags: no gradient


for _op in (minsum_joint_loss, minsum_layered_joint_loss, rcq_joint_loss, rcq_layered_joint_loss):
    _op.register_autograd(_joint_backward, setup_context=_joint_setup)


# ------------------------------------------------------------------------------------------ learned quantisers
@torch.library.custom_op("ldpc::rcq_joint_loss_levels", mutates_args=())
def rcq_joint_loss_levels(llr: Tensor, targets: Optional[Tensor], beta: Tensor, alpha: Tensor, thresholds: Tensor,
                          iteration_weights: Tensor, engine: int, want_grads: bool = True,
                          want_grad_llr: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """rcq_joint_loss run with the quantiser table `thresholds` [Q, L] (ldpc_train_joint_ste_levels): its seven outputs and
    grad_levels [T, L], d loss / d (reconstruction value of level l) of iteration t"""
    return _joint(llr, targets, beta, alpha, iteration_weights, engine, False, want_grads, want_grad_llr, "train_joint_ste",
                  thresholds=thresholds)


@torch.library.custom_op("ldpc::rcq_layered_joint_loss_levels", mutates_args=())
def rcq_layered_joint_loss_levels(llr: Tensor, targets: Optional[Tensor], beta: Tensor, alpha: Tensor, thresholds: Tensor,
                                  iteration_weights: Tensor, engine: int, want_grads: bool = True,
                                  want_grad_llr: bool = False) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """rcq_joint_loss_levels under the paper's layered schedule (ldpc_train_joint_layered_ste_levels)"""
    return _joint(llr, targets, beta, alpha, iteration_weights, engine, False, want_grads, want_grad_llr,
                  "train_joint_layered_ste", thresholds=thresholds)


@rcq_layered_joint_loss_levels.register_fake
@rcq_joint_loss_levels.register_fake
def _(llr, targets, beta, alpha, thresholds, iteration_weights, engine, want_grads=True, want_grad_llr=False):
    T, L = iteration_weights.shape[0], thresholds.shape[1]
    return _joint_fake(llr, targets, beta, alpha, iteration_weights, engine, False, want_grads, want_grad_llr) + (
        torch.empty((T, L), dtype=torch.float32, device=llr.device),)


def _levels_setup(ctx, inputs, output):
    ctx.want_grads, ctx.want_grad_llr = inputs[-2:]
    thresholds, engine = inputs[4], inputs[6]
    _loss, lpi, post, bits, gb, ga, gl, glv = output
    # row t of grad_levels belongs to the quantiser of iteration t
    ctx.q_of_iter = [int(q) for q in _engine(engine).q_of_iter[:glv.shape[0]]]
    ctx.thr_meta = (tuple(thresholds.shape), thresholds.dtype, thresholds.device)
    ctx.save_for_backward(lpi, gb, ga, gl, glv)
    ctx.mark_non_differentiable(lpi, post, bits, gb, ga, gl, glv)
    ctx.set_materialize_grads(False)


def _levels_backward(ctx, g_loss, *_unused):
    lpi, gb, ga, gl, glv = ctx.saved_tensors
    if g_loss is None:
        return (None,) * 9
    g_beta = gb * g_loss.to(gb.device) if ctx.want_grads and ctx.needs_input_grad[2] else None
    g_alpha = ga * g_loss.to(ga.device) if ctx.want_grads and ctx.needs_input_grad[3] else None
    g_llr = gl * g_loss if ctx.want_grad_llr and ctx.needs_input_grad[0] else None
    g_thr = None
    if ctx.needs_input_grad[4]:
        shape, dtype, dev = ctx.thr_meta
        rows = (glv * g_loss.to(glv.device)).to(device=dev, dtype=dtype)
        g_thr = torch.zeros(shape, dtype=dtype, device=dev).index_add(
            0, torch.tensor(ctx.q_of_iter, dtype=torch.long, device=dev), rows)     # [T, L] -> [Q, L], rows in order
    g_w = lpi * g_loss if ctx.needs_input_grad[5] else None
    return g_llr, None, g_beta, g_alpha, g_thr, g_w, None, None, None


for _op in (rcq_joint_loss_levels, rcq_layered_joint_loss_levels):
    _op.register_autograd(_levels_backward, setup_context=_levels_setup)
