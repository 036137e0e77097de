"""
Batched decode engine: Python owner of the native handles (include/ldpc_hip.h).

One ``DecodeEngine`` = one Tanner graph + one decoder descriptor (C2V rule,
weight tables, quantiser tables) on one GPU.  PyTorch is used only as plumbing:
device memory (``torch.empty``), the current HIP stream, and dtype bookkeeping.
The arithmetic runs in the hand-written HIP kernels; there is no CPU path.

The host decoder classes (ldpc_decoder.py, neural_2d_decoder.py, rcq_decoder.py)
flatten their reference-style parameters into the tables this class uploads.
"""

from __future__ import annotations

import collections
import ctypes as C
import os
import threading
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import _native as nat
from tanner_graph import TannerGraph


@dataclass
class DecodeResult:
    """Row-wise map of the reference's return tuple over a batch."""
    bits: Optional[torch.Tensor]          # int32 [B, n]     (posterior < 0)
    posterior: Optional[torch.Tensor]     # dtype [B, n]
    iterations: torch.Tensor              # int32 [B]        1-based, T when not converged
    success: torch.Tensor                 # bool  [B]
    packed_bits: Optional[torch.Tensor] = None   # uint8 [B, ceil(n/8)]
    rounds: Optional[torch.Tensor] = None        # int32 [B]        demapping rounds run (decode_iterative only)


def _require_gpu(device) -> torch.device:
    if not torch.cuda.is_available():
        raise nat.NativeEngineError(
            "no HIP device visible: the LDPC decode path runs only on the MI355X engine "
            "(libldpc_hip.so); there is no CPU fallback")
    dev = torch.device(device if device is not None else "cuda")
    if dev.type != "cuda":
        raise nat.NativeEngineError(f"decode device must be a ROCm GPU, got {dev}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def awgn_scale_shift(snr_db: float, llr_convention: str = "decoder"):
    """(scale, shift) = (2/sigma, +-2/sigma^2) of the BI-AWGN LLR llr = 2 (symbol + sigma z) / sigma^2 at Es/N0 = snr_db
    (sigma^2 = 10^(-snr_db/10)), computed in double; "reference" is the reference's literal channel (bit 0 -> -1): -shift"""
    if llr_convention not in ("decoder", "reference"):
        raise ValueError(f"llr_convention must be 'decoder' or 'reference', got {llr_convention!r}")
    noise_power = 1.0 / (10.0 ** (float(snr_db) / 10.0))
    shift = 2.0 / noise_power
    return 2.0 / noise_power ** 0.5, shift if llr_convention == "decoder" else -shift


def pack_codeword(codeword, n: int, device) -> torch.Tensor:
    """a 0/1 array of length n -> uint8 [ceil(n/8)] on `device`, bit j at byte j/8, bit j%8 (the decoders' packed format)"""
    c = np.asarray(codeword)
    if c.shape != (n,) or not np.isin(c, (0, 1)).all():
        raise ValueError(f"codeword must be a 0/1 array of length {n}")
    return torch.from_numpy(np.packbits(c.astype(np.uint8), bitorder="little")).to(device)


def _channel_codeword(codeword, n: int, dev: torch.device) -> Optional[torch.Tensor]:
    """the codeword argument of the channel functions -- None, a 0/1 array, or an already packed tensor -- as packed bytes on `dev`"""
    if codeword is None:
        return None
    if isinstance(codeword, str):
        raise ValueError(f"codeword must be None, a 0/1 array or a packed uint8 tensor, got {codeword!r}")
    cw = codeword if isinstance(codeword, torch.Tensor) else pack_codeword(codeword, n, dev)
    if cw.dtype != torch.uint8 or cw.device != dev or cw.numel() != (n + 7) // 8 or not cw.is_contiguous():
        raise ValueError(f"packed codeword must be a contiguous uint8 tensor of {(n + 7) // 8} bytes on {dev}")
    return cw


def _profile(rate_matching, n: int, dev: torch.device):
    """(struct, ctypes argument) of a RateMatching for the _rm entry points on `dev`; (None, None) without one.  The struct
    is returned so that it outlives the call."""
    if rate_matching is None:
        return None, None
    from rate_matching import RateMatching
    if not isinstance(rate_matching, RateMatching) or rate_matching.n != n:
        raise ValueError(f"rate_matching must be a RateMatching of n = {n}")
    rm = rate_matching.native(dev)
    return rm, C.byref(rm)


def _codeword_rows(codeword: torch.Tensor, batch: int, n: int, dev: torch.device) -> torch.Tensor:
    """one packed codeword per frame: a contiguous uint8 tensor [batch, ceil(n/8)] on `dev`"""
    if (codeword.dtype != torch.uint8 or codeword.device != dev or tuple(codeword.shape) != (batch, (n + 7) // 8)
            or not codeword.is_contiguous()):
        raise ValueError(f"codeword rows must be a contiguous uint8 tensor [{batch}, {(n + 7) // 8}] on {dev}")
    return codeword


def awgn_llr(batch: int, n: int, *, seed: int, stream_id: int = 0, first_frame: int = 0, snr_db: Optional[float] = None,
             scale: Optional[float] = None, shift: Optional[float] = None, codeword=None, device=None,
             rate_matching=None) -> torch.Tensor:
    """LLRs [batch, n] fp32 of frames first_frame .. first_frame + batch - 1 of the counter-based BI-AWGN stream
    (ldpc_channel_awgn; the stream is defined in include/ldpc_hip.h and INTEGRATION.md): frame f gets the same noise whatever
    block it is drawn in.  Give snr_db (Es/N0, positive-mean LLRs for the all-zero codeword) or (scale, shift) = (2/sigma,
    2/sigma^2).  codeword: 0/1 array of length n, or an already packed uint8 tensor on the device; None: all zero.
    rate_matching: a RateMatching of this n (ldpc_channel_awgn_rm): +0.0 at its punctured bits, +-short_llr at its shortened
    bits, the plain draw bit for bit everywhere else.  A 2-D uint8 tensor [batch, ceil(n/8)] is one packed codeword per frame,
    as ``encode_random`` returns them (ldpc_channel_awgn_cw): frame b is the one-codeword draw of that frame with row b."""
    dev = _require_gpu(device)
    if (snr_db is None) == (scale is None or shift is None):
        raise ValueError("give either snr_db or both scale and shift")
    if snr_db is not None:
        scale, shift = awgn_scale_shift(snr_db)
    batch, n = int(batch), int(n)
    if batch < 0 or n < 1:
        raise ValueError("batch must be >= 0 and n >= 1")
    rows = isinstance(codeword, torch.Tensor) and codeword.dim() == 2
    cw = _codeword_rows(codeword, batch, n, dev) if rows else _channel_codeword(codeword, n, dev)
    rm, rm_arg = _profile(rate_matching, n, dev)
    lib = nat.load()
    out = torch.empty((batch, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (C.c_void_p(out.data_ptr()), batch, n, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1),
                int(first_frame) & (2 ** 64 - 1), float(scale), float(shift), None if cw is None else C.c_void_p(cw.data_ptr()))
        if rows:
            nat.check(lib.ldpc_channel_awgn_cw(*args, rm_arg, C.c_void_p(stream)), "ldpc_channel_awgn_cw")
        elif rm is None:
            nat.check(lib.ldpc_channel_awgn(*args, C.c_void_p(stream)), "ldpc_channel_awgn")
        else:
            nat.check(lib.ldpc_channel_awgn_rm(*args, rm_arg, C.c_void_p(stream)), "ldpc_channel_awgn_rm")
    return out


def _check_modulation(modulation):
    from modulation import Modulation
    if not isinstance(modulation, Modulation):
        raise ValueError("modulation must be a modulation.Modulation")
    return modulation


def _is_constellation(modulation) -> bool:
    """a modulation.Constellation: the table-driven entry points (ldpc_*_con) instead of the separable ones (ldpc_*_sym)"""
    from modulation import Constellation
    return isinstance(modulation, Constellation)


def _symbol_amp(modulation, snr_db, amp) -> float:
    if (snr_db is None) == (amp is None):
        raise ValueError("with a modulation give either snr_db or amp")
    return modulation.amp(snr_db) if amp is None else float(amp)


def sym_llr(batch: int, n: int, *, seed: int, stream_id: int = 0, first_frame: int = 0, modulation, snr_db: Optional[float] = None,
            amp: Optional[float] = None, codeword=None, device=None, want_received: bool = False):
    """LLRs [batch, n] fp32 of frames first_frame .. first_frame + batch - 1 sent as Gray-mapped symbols of `modulation`
    (a modulation.Modulation) over AWGN or per-symbol Rayleigh fading, demapped by the modulation's demapper: max-log
    (ldpc_channel_sym; defined in include/ldpc_hip.h and INTEGRATION.md 6f) or exact (ldpc_channel_sym_dm).
    Frame f gets the same noise and fading whatever block it is drawn in.  Give snr_db (Es/N0) or amp, the
    constellation's half-spacing over the per-dimension noise standard deviation.  codeword: None (all zero), a 0/1 array of
    length n, a packed uint8 tensor, or a 2-D uint8 tensor [batch, ceil(n/8)] of one packed codeword per frame, as
    ``encode_random`` returns them.  want_received: -> (llr, received), received fp32 [batch, S, 4] = (vI, vQ, e, 0) per
    symbol, e the fading gain times amp (vQ = 0 for BPSK) -- for a constellation plot, for ``demap``, or a demapper of your own.
    A modulation.Constellation sends the points of its table and is demapped jointly over all of them (ldpc_channel_con;
    INTEGRATION.md 6i); amp is then 1 / sigma, sigma the per-dimension noise standard deviation."""
    dev = _require_gpu(device)
    mod = _check_modulation(modulation)
    amp = _symbol_amp(mod, snr_db, amp)
    batch, n = int(batch), int(n)
    if batch < 0 or n < 1:
        raise ValueError("batch must be >= 0 and n >= 1")
    rows = isinstance(codeword, torch.Tensor) and codeword.dim() == 2
    cw = _codeword_rows(codeword, batch, n, dev) if rows else _channel_codeword(codeword, n, dev)
    desc, _keep = mod.native(amp, n, dev)
    lib = nat.load()
    out = torch.empty((batch, n), dtype=torch.float32, device=dev)
    rec = torch.empty((batch, mod.symbols(n), 4), dtype=torch.float32, device=dev) if want_received else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (C.c_void_p(out.data_ptr()), batch, n, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1),
                int(first_frame) & (2 ** 64 - 1), C.byref(desc), None if cw is None else C.c_void_p(cw.data_ptr()),
                (n + 7) // 8 if rows else 0, None if rec is None else C.c_void_p(rec.data_ptr()))
        if _is_constellation(mod):
            from modulation import DEMAPPERS
            nat.check(lib.ldpc_channel_con(*args, DEMAPPERS[mod.demapper], C.c_void_p(stream)), "ldpc_channel_con")
        elif mod.demapper == "exact":
            nat.check(lib.ldpc_channel_sym_dm(*args, nat.DEMAP_EXACT, C.c_void_p(stream)), "ldpc_channel_sym_dm")
        else:
            nat.check(lib.ldpc_channel_sym(*args, C.c_void_p(stream)), "ldpc_channel_sym")
    return (out, rec) if want_received else out


def demap(received, n: int, *, modulation, demapper: Optional[str] = None, device=None, prior=None, prior_sub=None,
          prior_scale: float = 1.0, out=None) -> torch.Tensor:
    """LLRs [batch, n] fp32 from received samples (ldpc_demap_sym): `received` is a contiguous float32
    tensor [batch, S, 4] = (vI, vQ, e, 0) per symbol on the device, S = ceil(n / m) -- what ``sym_llr(want_received=True)``
    returns, or ``modulation.normalise_received`` of physical samples.  demapper "maxlog" | "exact"; None: the modulation's
    own.  The modulation's fading is not used (e travels with the samples); its interleaver is honoured.  With "maxlog" the
    samples of a ``sym_llr`` call give that call's LLRs bit for bit, with "exact" those of the same call under
    ``Modulation(..., demapper="exact")``.  A modulation.Constellation goes through ldpc_demap_con.

    prior / prior_sub / prior_scale / out (a modulation.Constellation only; ldpc_demap_con_prior): with
    a priori LLRs La = prior_scale * (prior - prior_sub) of the frame's variables (prior_sub None: prior_scale * prior) the
    result is the *extrinsic* LLR of every bit, what the samples and the other bits of its symbol say about it -- the demapper
    of iterative demapping, fed with prior = a decoder's posterior and prior_sub = the LLRs that decoder was given.  Both are
    contiguous fp32 [batch, n] tensors on the samples' device, finite.  out: a contiguous fp32 [batch, n] tensor on that device
    to write into; it may be prior or prior_sub themselves.  Without any of the four the call is the one above."""
    mod = _check_modulation(modulation)
    from modulation import DEMAPPERS
    rule = mod.demapper if demapper is None else demapper
    if not isinstance(rule, str) or rule not in DEMAPPERS:
        raise ValueError(f"demapper must be None, 'maxlog' or 'exact', got {demapper!r}")
    n = int(n)
    if n < 1:
        raise ValueError("n must be >= 1")
    S = mod.symbols(n)
    if (not isinstance(received, torch.Tensor) or received.dtype != torch.float32 or received.dim() != 3
            or tuple(received.shape[1:]) != (S, 4) or not received.is_contiguous()):
        raise ValueError(f"received must be a contiguous float32 tensor [batch, {S}, 4] = (vI, vQ, e, 0) per symbol")
    if isinstance(prior_scale, (bool, str)) or not np.isscalar(prior_scale) or not np.isreal(prior_scale):
        raise ValueError(f"prior_scale must be a finite number, got {prior_scale!r}")
    prior_scale = float(prior_scale)
    if prior is not None or prior_sub is not None or out is not None or prior_scale != 1.0:
        if (prior is not None or prior_sub is not None) and not _is_constellation(mod):
            raise ValueError(f"priors need a modulation.Constellation: the separable Gray demapper of {mod.scheme!r} has no prior "
                             f"form (Gray labels gain nothing from feedback); Constellation.from_modulation gives its table")
        if prior_sub is not None and prior is None:
            raise ValueError("prior_sub without a prior")
        if not np.isfinite(prior_scale):
            raise ValueError(f"prior_scale must be a finite number, got {prior_scale!r}")
        if prior_scale != 1.0 and prior is None:
            raise ValueError("prior_scale without a prior")
        for name, t in (("prior", prior), ("prior_sub", prior_sub), ("out", out)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32
                                  or tuple(t.shape) != (int(received.shape[0]), n) or not t.is_contiguous()
                                  or t.device != received.device):
                raise ValueError(f"{name} must be a contiguous float32 tensor [{int(received.shape[0])}, {n}] on the samples' "
                                 f"device {received.device}")
    want = None if device is None else torch.device(device)
    if received.device.type != "cuda" or (want is not None and (want.type != "cuda" or want.index not in
                                                                (None, received.device.index))):
        raise ValueError(f"received must be on the GPU the call is for, got {received.device}"
                         f"{'' if want is None else f' and device={want}'}")
    dev = _require_gpu(received.device)
    batch = int(received.shape[0])
    desc, _keep = mod.native(0.0, n, dev)
    lib = nat.load()
    if out is None:
        out = torch.empty((batch, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if prior is not None:
            nat.check(lib.ldpc_demap_con_prior(C.c_void_p(out.data_ptr()), batch, n, C.byref(desc), DEMAPPERS[rule],
                                               C.c_void_p(received.data_ptr()), C.c_void_p(prior.data_ptr()),
                                               None if prior_sub is None else C.c_void_p(prior_sub.data_ptr()),
                                               float(prior_scale), C.c_void_p(stream)), "ldpc_demap_con_prior")
            return out
        fn, name = (lib.ldpc_demap_con, "ldpc_demap_con") if _is_constellation(mod) else (lib.ldpc_demap_sym, "ldpc_demap_sym")
        nat.check(fn(C.c_void_p(out.data_ptr()), batch, n, C.byref(desc), DEMAPPERS[rule],
                     C.c_void_p(received.data_ptr()), C.c_void_p(stream)), name)
    return out


MIX_MAX_POINTS = 4096     # ldpc_channel_awgn_mix: n_points <= 4096, batch <= 2^31 - 1 (the point index stays in 32 bits)


def snr_grid(snr_range, snr_step: float) -> np.ndarray:
    """the SNR points lo + k * step, k = 0 .. K - 1, of (lo, hi) = snr_range as float64, K = floor((hi - lo) / step + 1e-9) + 1:
    (0, 6) with step 0.5 gives 13 points, (3, 3) with any step one"""
    lo, hi = (float(v) for v in snr_range)
    step = float(snr_step)
    if not step > 0:
        raise ValueError(f"snr_step must be > 0, got {snr_step!r}")
    if hi < lo:
        raise ValueError(f"snr_range must be (lo, hi) with hi >= lo, got {snr_range!r}")
    return lo + step * np.arange(int(np.floor((hi - lo) / step + 1e-9)) + 1, dtype=np.float64)


def mix_points(first_frame: int, batch: int, n_points: int, device=None) -> torch.Tensor:
    """int64 [batch]: the SNR point (first_frame + b) % n_points of each frame of a block of ldpc_channel_awgn_mix.  The
    remainder of first_frame is taken on Python integers, so frame indices of 2^63 and above are right."""
    first_frame, batch, n_points = int(first_frame), int(batch), int(n_points)
    if batch < 0 or n_points < 1 or first_frame < 0:
        raise ValueError("batch and first_frame must be >= 0 and n_points >= 1")
    return (first_frame % n_points + torch.arange(batch, dtype=torch.int64, device=device)) % n_points


def _mix_table(values, what: str, dev: torch.device) -> torch.Tensor:
    """a 1-D sequence, or an fp32 tensor already on `dev`, as a contiguous fp32 table on `dev`"""
    if isinstance(values, torch.Tensor):
        if values.dtype != torch.float32 or values.device != dev or values.dim() != 1 or not values.is_contiguous():
            raise ValueError(f"{what} tensor must be a contiguous 1-D float32 tensor on {dev}")
        return values
    tab = np.asarray(values, dtype=np.float64)
    if tab.ndim != 1:
        raise ValueError(f"{what} must be a 1-D sequence")
    return torch.from_numpy(tab.astype(np.float32)).to(dev)


def awgn_mix_tables(snr_db, llr_convention: str = "decoder", device=None):
    """(scale_tab, shift_tab): float32 [K] on the device for the K SNR points of snr_db, each through ``awgn_scale_shift`` in
    double and then cast -- what ``awgn_llr_mix(snr_db=...)`` builds per call, for callers that draw many blocks"""
    dev = _require_gpu(device)
    snr = np.asarray(snr_db, dtype=np.float64)
    if snr.ndim != 1:
        raise ValueError("snr_db must be a 1-D sequence of SNR points")
    pairs = [awgn_scale_shift(float(s), llr_convention) for s in snr]
    return _mix_table([p[0] for p in pairs], "scale", dev), _mix_table([p[1] for p in pairs], "shift", dev)


def awgn_llr_mix(batch: int, n: int, *, seed: int, stream_id: int = 0, first_frame: int = 0, snr_db=None, scale=None,
                 shift=None, llr_convention: str = "decoder", codeword=None, device=None,
                 rate_matching=None) -> torch.Tensor:
    """``awgn_llr`` with the SNR point a function of the frame (ldpc_channel_awgn_mix): frame f = first_frame + b is drawn at
    point f % K of a table of K points -- the same noise as ``awgn_llr`` gives frame f, and the same point whatever block the
    frame is drawn in, so every run of K consecutive frames holds each point once.  Give snr_db, a sequence of K values of
    Es/N0 (tables through ``awgn_scale_shift(snr, llr_convention)`` per point in double, then fp32), or scale and shift: two
    1-D sequences, or float32 tensors on the device, of equal length.  codeword and rate_matching as in ``awgn_llr``
    (ldpc_channel_awgn_mix_rm with a profile)."""
    dev = _require_gpu(device)
    if (snr_db is None) == (scale is None or shift is None):
        raise ValueError("give either snr_db or both scale and shift")
    if llr_convention not in ("decoder", "reference"):
        raise ValueError(f"llr_convention must be 'decoder' or 'reference', got {llr_convention!r}")
    if snr_db is not None:
        scale_tab, shift_tab = awgn_mix_tables(snr_db, llr_convention, dev)
    else:
        scale_tab, shift_tab = _mix_table(scale, "scale", dev), _mix_table(shift, "shift", dev)
    n_points = scale_tab.numel()
    if shift_tab.numel() != n_points:
        raise ValueError(f"scale and shift must have equal length, got {n_points} and {shift_tab.numel()}")
    if not 1 <= n_points <= MIX_MAX_POINTS:
        raise ValueError(f"the number of SNR points must be in 1 .. {MIX_MAX_POINTS}, got {n_points}")
    batch, n = int(batch), int(n)
    if batch < 0 or n < 1:
        raise ValueError("batch must be >= 0 and n >= 1")
    if batch > 2 ** 31 - 1:
        raise ValueError("batch must be <= 2^31 - 1")
    cw = _channel_codeword(codeword, n, dev)
    rm, rm_arg = _profile(rate_matching, n, dev)
    lib = nat.load()
    out = torch.empty((batch, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (C.c_void_p(out.data_ptr()), batch, n, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1),
                int(first_frame) & (2 ** 64 - 1), C.c_void_p(scale_tab.data_ptr()), C.c_void_p(shift_tab.data_ptr()), n_points,
                None if cw is None else C.c_void_p(cw.data_ptr()))
        if rm is None:
            nat.check(lib.ldpc_channel_awgn_mix(*args, C.c_void_p(stream)), "ldpc_channel_awgn_mix")
        else:
            nat.check(lib.ldpc_channel_awgn_mix_rm(*args, rm_arg, C.c_void_p(stream)), "ldpc_channel_awgn_mix_rm")
    return out


def sym_llr_mix(batch: int, n: int, *, seed: int, stream_id: int = 0, first_frame: int = 0, modulation, snr_db=None, amp=None,
                codeword=None, device=None, want_targets: bool = False):
    """``sym_llr`` with the SNR point a function of the frame (ldpc_channel_sym_mix): frame
    f = first_frame + b is drawn at point f % K of a table of K points and gets, bit for bit, what ``sym_llr`` gives frame f at
    that point, whatever block it is drawn in (``mix_points`` tells which point a frame has).  Give snr_db, a sequence of K
    values of Es/N0 (the table is ``modulation.amp_table(snr_db)``), or amp: a 1-D sequence, or a contiguous float32 tensor on
    the device, whose entries are then the caller's responsibility.  codeword as in ``sym_llr``.  want_targets: ->
    (llr, targets), targets fp32 [batch, n] = the bits that were sent as 0.0 / 1.0, written by the same kernel: what
    ``model.joint_posterior_loss(llr, targets)`` takes."""
    mod = _check_modulation(modulation)
    if (snr_db is None) == (amp is None):
        raise ValueError("with a modulation give either snr_db or amp")
    values = mod.amp_table(snr_db) if amp is None else amp
    if isinstance(values, torch.Tensor):
        n_points = values.numel()
    else:
        host = np.asarray(values, dtype=np.float64)
        if host.ndim != 1:
            raise ValueError("amp must be a 1-D sequence")
        if not (np.isfinite(host).all() and (host >= 0.0).all()):
            raise ValueError("amp must be finite and >= 0 at every point")
        n_points = host.size
    if not 1 <= n_points <= MIX_MAX_POINTS:
        raise ValueError(f"the number of SNR points must be in 1 .. {MIX_MAX_POINTS}, got {n_points}")
    batch, n = int(batch), int(n)
    if batch < 0 or n < 1:
        raise ValueError("batch must be >= 0 and n >= 1")
    if batch > 2 ** 31 - 1:
        raise ValueError("batch must be <= 2^31 - 1")
    dev = _require_gpu(device)
    amp_tab = _mix_table(values, "amp", dev)
    rows = isinstance(codeword, torch.Tensor) and codeword.dim() == 2
    cw = _codeword_rows(codeword, batch, n, dev) if rows else _channel_codeword(codeword, n, dev)
    desc, _keep = mod.native(0.0, n, dev)
    lib = nat.load()
    out = torch.empty((batch, n), dtype=torch.float32, device=dev)
    targets = torch.empty((batch, n), dtype=torch.float32, device=dev) if want_targets else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        args = (C.c_void_p(out.data_ptr()), batch, n, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1),
                int(first_frame) & (2 ** 64 - 1), C.byref(desc), C.c_void_p(amp_tab.data_ptr()), n_points,
                None if cw is None else C.c_void_p(cw.data_ptr()), (n + 7) // 8 if rows else 0,
                None if targets is None else C.c_void_p(targets.data_ptr()))
        if _is_constellation(mod):
            from modulation import DEMAPPERS
            nat.check(lib.ldpc_channel_con_mix(*args, DEMAPPERS[mod.demapper], C.c_void_p(stream)), "ldpc_channel_con_mix")
        elif mod.demapper == "exact":
            nat.check(lib.ldpc_channel_sym_mix_dm(*args, nat.DEMAP_EXACT, C.c_void_p(stream)), "ldpc_channel_sym_mix_dm")
        else:
            nat.check(lib.ldpc_channel_sym_mix(*args, C.c_void_p(stream)), "ldpc_channel_sym_mix")
    return (out, targets) if want_targets else out


SIM_COUNTERS = ("frames", "frame_errors", "bit_errors", "iterations", "done", "blocks_seen")
ERROR_FRAME_DTYPE = np.dtype([("frame", np.uint64), ("wrong_bits", np.int64), ("iterations", np.int64), ("undetected", np.int64)])


def sim_diag_words(T: int, capture: int) -> int:
    """int64 words of a diag buffer (ldpc_sim_diag_words): 4 header words, T + 1 histogram bins, 4 words per captured frame"""
    T, capture = int(T), int(capture)
    if T < 0 or capture < 0:
        raise ValueError("T and capture must be >= 0")
    return 4 + T + 1 + 4 * capture


def parse_sim_diag(words, T: int, capture: int) -> dict:
    """a diag buffer of ldpc_sim_count_diag / ldpc_simulate_diag (include/ldpc_hip.h) -> {undetected_errors, captured,
    iteration_histogram np.int64 [T + 1], error_frames}: error_frames is a structured array (frame uint64, wrong_bits,
    iterations, undetected) of the `captured` recorded frame errors, in frame order."""
    w = np.ascontiguousarray(np.asarray(words, dtype=np.int64)).reshape(-1)
    if w.size != sim_diag_words(T, capture):
        raise ValueError(f"a diag buffer of T = {T}, capture = {capture} has {sim_diag_words(T, capture)} words, got {w.size}")
    captured = int(w[1])
    if not 0 <= captured <= capture:
        raise ValueError(f"diag buffer records {captured} frames, capture is {capture}")
    rec = w[4 + T + 1:].reshape(capture, 4)[:captured]
    frames = np.empty(captured, dtype=ERROR_FRAME_DTYPE)
    frames["frame"] = rec[:, 0].view(np.uint64) if captured else 0
    frames["wrong_bits"], frames["iterations"], frames["undetected"] = rec[:, 1], rec[:, 2], rec[:, 3]
    return {"undetected_errors": int(w[0]), "captured": captured, "iteration_histogram": w[4:4 + T + 1].copy(),
            "error_frames": frames}


class _NativeGraph:
    """ldpc_graph* for (graph, device); shared by all engines on that graph.  The cache holds the host graph WEAKLY: when
    the TannerGraph object dies its entries are evicted, and the device copy is destroyed (ldpc_graph_destroy) as soon as
    no engine uses it either -- a sweep over many codes does not accumulate device memory."""
    _cache = {}
    _lock = threading.Lock()

    def __init__(self, graph: TannerGraph, device: torch.device):
        lib = nat.load()
        self.handle = C.c_void_p()
        with torch.cuda.device(device):
            cp = np.ascontiguousarray(graph.check_ptr, dtype=np.int32)
            vi = np.ascontiguousarray(graph.var_idx, dtype=np.int32)
            lp = getattr(graph, "layer_ptr", None)
            if lp is None:
                nat.check(lib.ldpc_graph_create(C.byref(self.handle), graph.n, graph.m, graph.E,
                                                nat.ptr(cp), nat.ptr(vi)), "ldpc_graph_create")
            else:       # a graph that declares layers (TannerGraph.with_layers): the block-parallel layered kernel may run on it
                lp = np.ascontiguousarray(lp, dtype=np.int32)
                nat.check(lib.ldpc_graph_create_layered(C.byref(self.handle), graph.n, graph.m, graph.E, nat.ptr(cp),
                                                        nat.ptr(vi), lp.size - 1, nat.ptr(lp)), "ldpc_graph_create_layered")
        self._lib = lib

    def __del__(self):
        try:
            if getattr(self, "handle", None) is not None and self.handle.value:
                self._lib.ldpc_graph_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    @classmethod
    def _evict(cls, key):
        with cls._lock:
            cls._cache.pop(key, None)

    @classmethod
    def get(cls, graph: TannerGraph, device: torch.device) -> "_NativeGraph":
        return cls._get(graph, device.index, lambda: cls(graph, device))

    @classmethod
    def _get(cls, graph, dev_index, make):
        key = (id(graph), dev_index)
        with cls._lock:
            hit = cls._cache.get(key)
            if hit is not None and hit[0]() is graph:
                return hit[1]
            ng = make()
            cls._cache[key] = (weakref.ref(graph), ng)
            weakref.finalize(graph, cls._evict, key)
            return ng


class _NativeEncoder:
    """ldpc_encoder* for (codes.Encoder, device), cached as _NativeGraph caches graphs: weakly on the host object"""
    _cache = {}
    _lock = threading.Lock()

    def __init__(self, encoder, device: torch.device):
        lib = nat.load()
        self.handle = C.c_void_p()
        with torch.cuda.device(device):
            nat.check(lib.ldpc_encoder_create(C.byref(self.handle), encoder.n, encoder.k, nat.ptr(encoder.info_pos),
                                              nat.ptr(encoder.parity_pos), nat.ptr(encoder.row_ptr), nat.ptr(encoder.info_idx),
                                              int(encoder.accumulate)), "ldpc_encoder_create")
        self._lib = lib

    def __del__(self):
        try:
            if getattr(self, "handle", None) is not None and self.handle.value:
                self._lib.ldpc_encoder_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    @classmethod
    def _evict(cls, key):
        with cls._lock:
            cls._cache.pop(key, None)

    @classmethod
    def get(cls, encoder, device: torch.device) -> "_NativeEncoder":
        key = (id(encoder), device.index)
        with cls._lock:
            hit = cls._cache.get(key)
            if hit is not None and hit[0]() is encoder:
                return hit[1]
            ne = cls(encoder, device)
            cls._cache[key] = (weakref.ref(encoder), ne)
            weakref.finalize(encoder, cls._evict, key)
            return ne


def _check_encoder(encoder):
    from codes import Encoder
    if not isinstance(encoder, Encoder):
        raise ValueError("encoder must be a codes.Encoder")
    return encoder


def encode_random(encoder, batch: int, *, seed: int, stream_id: int = 0, first_frame: int = 0, device=None,
                  want_info: bool = False):
    """Codewords of frames first_frame .. first_frame + batch - 1 of the information-bit stream (ldpc_encode_random; the
    stream is defined in include/ldpc_hip.h and INTEGRATION.md): uint8 [batch, ceil(n/8)] on the device, bit j at byte j/8,
    bit j%8 -- what ``awgn_llr(codeword=...)`` and ``DecodeEngine.sim_count(codeword=...)`` take.  The codeword of a frame does
    not depend on the block it is drawn in.  want_info: -> (codewords, information rows uint8 [batch, ceil(k/8)])."""
    enc = _check_encoder(encoder)
    dev = _require_gpu(device)
    batch = int(batch)
    if batch < 0:
        raise ValueError("batch must be >= 0")
    ne = _NativeEncoder.get(enc, dev)
    cw = torch.empty((batch, (enc.n + 7) // 8), dtype=torch.uint8, device=dev)
    info = torch.empty((batch, (enc.k + 7) // 8), dtype=torch.uint8, device=dev) if want_info else None
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        nat.check(ne._lib.ldpc_encode_random(ne.handle, batch, int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1),
                                             int(first_frame) & (2 ** 64 - 1), C.c_void_p(cw.data_ptr()),
                                             None if info is None else C.c_void_p(info.data_ptr()), C.c_void_p(stream)),
                  "ldpc_encode_random")
    return (cw, info) if want_info else cw


def encode(encoder, info_packed: torch.Tensor) -> torch.Tensor:
    """Codewords uint8 [B, ceil(n/8)] of the information rows info_packed, uint8 [B, ceil(k/8)] on a GPU in the packed format
    (ldpc_encode); bits at and beyond k in a row's last byte are ignored."""
    enc = _check_encoder(encoder)
    if not isinstance(info_packed, torch.Tensor) or info_packed.dtype != torch.uint8 or info_packed.dim() != 2 \
            or info_packed.shape[1] != (enc.k + 7) // 8:
        raise ValueError(f"info_packed must be a uint8 tensor [B, {(enc.k + 7) // 8}]")
    dev = _require_gpu(info_packed.device)
    info_packed = info_packed.contiguous()
    batch = int(info_packed.shape[0])
    ne = _NativeEncoder.get(enc, dev)
    cw = torch.empty((batch, (enc.n + 7) // 8), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        nat.check(ne._lib.ldpc_encode(ne.handle, C.c_void_p(info_packed.data_ptr()), batch, C.c_void_p(cw.data_ptr()),
                                      C.c_void_p(stream)), "ldpc_encode")
    return cw


class DecodeEngine:
    def __init__(self, graph: TannerGraph, *, dtype: torch.dtype, c2v_form: int, iters: int,
                 beta: np.ndarray, beta_slot: np.ndarray, alpha: np.ndarray, alpha_slot: np.ndarray,
                 thresholds: Optional[np.ndarray] = None, q_of_iter: Optional[np.ndarray] = None,
                 oms_alpha: Optional[np.ndarray] = None, oms_alpha_slot: Optional[np.ndarray] = None,
                 schedule: int = nat.SCHED_FLOODING, device=None):
        if dtype not in (torch.float32, torch.float64):
            raise TypeError("engine dtype must be float32 or float64")
        self.device = _require_gpu(device)
        self.graph = graph
        self.dtype = dtype
        self.np_dtype = np.float32 if dtype == torch.float32 else np.float64
        self.iters = int(iters)
        self.c2v_form = int(c2v_form)
        self.schedule = int(schedule)
        lib = nat.load()
        self._lib = lib
        self._ng = _NativeGraph.get(graph, self.device)
        rows = max(self.iters, 1)
        beta = np.ascontiguousarray(beta, dtype=self.np_dtype).reshape(rows, -1)
        alpha = np.ascontiguousarray(alpha, dtype=self.np_dtype).reshape(rows, -1)
        beta_slot = np.ascontiguousarray(beta_slot, dtype=np.int32)
        alpha_slot = np.ascontiguousarray(alpha_slot, dtype=np.int32)
        if beta_slot.shape != (graph.E,) or alpha_slot.shape != (graph.n,):
            raise ValueError("slot arrays must have one entry per edge / per variable")
        desc = nat.DecoderDesc()
        desc.dtype = nat.LDPC_F32 if dtype == torch.float32 else nat.LDPC_F64
        desc.c2v_form, desc.iters = self.c2v_form, self.iters
        desc.schedule = int(schedule)
        desc.n_beta_slots, desc.beta, desc.beta_slot = beta.shape[1], nat.ptr(beta), nat.ptr(beta_slot)
        desc.n_alpha_slots, desc.alpha, desc.alpha_slot = alpha.shape[1], nat.ptr(alpha), nat.ptr(alpha_slot)
        keep = [beta, alpha, beta_slot, alpha_slot]
        if self.c2v_form == nat.C2V_RCQ:
            thresholds = np.ascontiguousarray(thresholds, dtype=np.float32)
            q_of_iter = np.ascontiguousarray(q_of_iter, dtype=np.int32)
            if thresholds.ndim != 2 or q_of_iter.shape[0] < self.iters:
                raise ValueError("bad quantiser tables")
            desc.n_quantizers, desc.n_levels = thresholds.shape
            desc.thresholds, desc.q_of_iter = nat.ptr(thresholds), nat.ptr(q_of_iter)
            keep += [thresholds, q_of_iter]
            self._thresholds = thresholds.copy()   # what the device holds (set_quantizers replaces it)
            self.q_of_iter = q_of_iter[:max(self.iters, 1)].copy()
        if self.c2v_form == nat.C2V_OMS and oms_alpha is not None:
            oms_alpha = np.ascontiguousarray(oms_alpha, dtype=self.np_dtype).reshape(rows, -1)
            oms_alpha_slot = np.ascontiguousarray(oms_alpha_slot, dtype=np.int32)
            desc.n_oms_alpha_slots = oms_alpha.shape[1]
            desc.oms_alpha, desc.oms_alpha_slot = nat.ptr(oms_alpha), nat.ptr(oms_alpha_slot)
            keep += [oms_alpha, oms_alpha_slot]
        self._table_shapes = (beta.shape, alpha.shape, None if oms_alpha is None else oms_alpha.shape)
        # what the device holds (the gradient path restores them): beta, alpha, check-side alpha of the offset form
        self._tables = [beta.copy(), alpha.copy(), None if oms_alpha is None else oms_alpha.copy()]
        self.handle = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(lib.ldpc_decoder_create(C.byref(self.handle), self._ng.handle, C.byref(desc)),
                      "ldpc_decoder_create")
        # scratch of ldpc_decode, one buffer PER STREAM: the C ABI wants one workspace per decode that may overlap
        # another on the device, and calls from different threads arrive on different (or the same) torch streams --
        # same stream = serialised by the stream, different streams = different buffers.  Guarded by _ws_lock.
        self._ws = collections.OrderedDict()       # stream handle -> buffer, least recently used first; at most _WS_MAX
        self._ws_lock = threading.Lock()
        self._host_lock = threading.Lock()         # staging buffers of decode_host (not held by _workspace callers)
        mode = os.environ.get("LDPC_ENGINE_MODE", "auto")
        try:
            self.set_mode(mode)
        except NotImplementedError:
            if mode not in ("gather", "pair"):
                raise
            self.set_mode("stream")          # the RCQ-only forms, asked for process-wide: other decoders stream

    def __del__(self):
        try:
            if getattr(self, "handle", None) is not None and self.handle.value:
                self._lib.ldpc_decoder_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:
            pass

    # ------------------------------------------------------------------ engine choice
    _MODES = {"auto": nat.MODE_AUTO, "stream": nat.MODE_STREAM, "resident": nat.MODE_RESIDENT, "sweeps": nat.MODE_SWEEPS,
              "gather": nat.MODE_GATHER, "pair": nat.MODE_PAIR, "block": nat.MODE_BLOCK}

    def set_mode(self, mode: str):
        """'auto' (LDS-resident fused kernel when the code qualifies, else streaming), 'stream' (HBM-streaming
        engine; fp32 RCQ decoders run its cheapest applicable form: 1-byte codes both ways ('pair'), else the fused
        one-kernel-per-iteration form ('gather')), 'sweeps' (streaming, always one kernel per sweep with fp32
        variable->check rows), 'gather' / 'pair' (force that RCQ form; error when the decoder does not qualify),
        'resident', 'block' (the block-parallel layered kernel: a layered decoder on a graph that declares layers; error
        otherwise) -- every choice gives identical results."""
        nat.check(self._lib.ldpc_decoder_set_mode(self.handle, self._MODES[mode]), "ldpc_decoder_set_mode")
        with self._ws_lock:
            self._ws.clear()
        return self

    def info(self) -> dict:
        out = np.zeros(4, dtype=np.int32)
        nat.check(self._lib.ldpc_decoder_info(self.handle, nat.ptr(out)), "ldpc_decoder_info")
        block = int(out[0]) == nat.MODE_BLOCK          # LDS-resident too: the block-parallel layered kernel
        resident = int(out[0]) == nat.MODE_RESIDENT or block
        if self.schedule == nat.SCHED_FLOODING:
            kernel = "resident" if resident else {3: "sweeps", 4: "cn_gather", 5: "code_pair"}[int(out[0])]
        else:   # the layered schedules: LDS-resident walk (ldpc_layered.hip) or the HBM-streaming one (layered_rcq / layered_minsum)
            paper = self.schedule == nat.SCHED_LAYERED
            if self.c2v_form != nat.C2V_RCQ:      # the min-sum forms: check records in LDS, or fp32 messages in HBM
                kernel = "layered_block_lds" if block else "layered_minsum_lds" if resident else "layered_minsum"
            else:
                kernel = "layered_block_lds" if block else ("layered_paper_lds" if paper else "layered_lds") if resident else \
                         ("layered_rcq<paper>" if paper else "layered_rcq<ref>")
        # workgroups per CU as LDS (160 KiB) and the wave slots (32 per CU) allow; 0 on the streaming engine
        threads, lds = int(out[2]), int(out[3])
        per_cu = min((160 * 1024) // lds, (32 * 64) // threads) if resident and threads and lds else 0
        # the compact fixed-T plan's variable grid, costed by the body-cost model of its variable phase (per wave and phase)
        stats = np.zeros(4, dtype=np.int32)
        plan = None
        if self._lib.ldpc_debug_compact_layout(self.handle, 0, 0, 0, None, None, None, None, nat.ptr(stats)) == 0:
            plan = {"positions": int(stats[0]), "worst_wave_cost": int(stats[1]), "mean_wave_cost": float(stats[2]) / 8,
                    "mixed_cells": int(stats[3])}
            # waves whose check phase runs on a scalar trip count (bit 31 of a check word: the per-lane form)
            words = np.zeros(8, dtype=np.uint32)
            nat.check(self._lib.ldpc_debug_compact_checks(self.handle, 0, 0, 0, None, None, nat.ptr(words)),
                      "ldpc_debug_compact_checks")
            plan["scalar_check_waves"] = int(np.count_nonzero((words != 0) & (words >> 31 == 0)))
        # what a flooding decode launches on the resident engine, per stop mode (None on the streaming engine)
        kernels = None
        if resident and self.schedule == nat.SCHED_FLOODING:
            kernels = {"fixed_T": self._resident_kernel(False), "early_stop": self._resident_kernel(True)}
        form = {nat.C2V_NMS: "NMS", nat.C2V_RCQ: "RCQ", nat.C2V_OMS: "OMS", nat.C2V_SPA: "SPA"}[self.c2v_form]
        n_layers = C.c_int32(0)
        nat.check(self._lib.ldpc_graph_layers(self._ng.handle, C.byref(n_layers), None), "ldpc_graph_layers")
        return {"engine": {2: "resident", 3: "stream", 4: "stream", 5: "stream", 6: "resident"}[int(out[0])], "kernel": kernel, "form": form,
                "stream_form": {2: None, 3: "two-sweeps", 4: "fused-rcq-iteration", 5: "rcq-code-pair", 6: None}[int(out[0])],
                "layers": int(n_layers.value),
                "codewords_per_workgroup": int(out[1]),
                "threads_per_workgroup": threads, "lds_bytes": lds, "workgroups_per_cu": per_cu,
                "compact_plan": plan, "resident_kernel": kernels}

    def _resident_kernel(self, early_stop: bool) -> dict:
        """the resident_decode instantiation and table flags of a decode in this stop mode (ldpc_debug_resident_kernel)"""
        o = np.zeros(12, dtype=np.int32)
        nat.check(self._lib.ldpc_debug_resident_kernel(self.handle, int(early_stop), nat.ptr(o)),
                  "ldpc_debug_resident_kernel")
        return {"plan": ("general", "register-state", "compact")[int(o[0])], "G": int(o[1]),
                "form": {nat.C2V_NMS: "NMS", nat.C2V_RCQ: "RCQ", nat.C2V_OMS: "OMS"}[int(o[2])], "bpc": bool(o[3]),
                "nl": int(o[4]), "ms": int(o[5]), "row_stride": int(o[6]), "split": bool(o[7]),
                "unit_alpha": bool(o[8]), "rcq_zero0": bool(o[9]), "oms_alpha": bool(o[10]),
                "alpha_in_lds": bool(o[11])}

    def boundary_kernels(self, batch: int, *, llr: int = 0, posterior: int = 0, bits: int = 0,
                         max_iters: Optional[int] = None, saving: bool = False) -> dict:
        """which kernels move the rows of a streaming decode between the caller's layout and the tiles
        (ldpc_debug_boundary_kernels; host only).  llr / posterior / bits are ADDRESSES (tensor.data_ptr(); 0: NULL).
        NotImplementedError when the decode runs an LDS-resident kernel."""
        o = np.zeros(5, dtype=np.int32)
        a = lambda v: C.c_void_p(int(v)) if v else None
        nat.check(self._lib.ldpc_debug_boundary_kernels(self.handle, int(batch), int(max_iters or 0), int(bool(saving)),
                                                        a(llr), a(posterior), a(bits), nat.ptr(o)),
                  "ldpc_debug_boundary_kernels")
        return {"vec": int(o[0]), "in_bytes": int(o[1]), "fused_in": bool(o[2]),
                "out_path": ("none", "layout", "last-rows")[int(o[3])], "out_bytes": int(o[4])}

    def launch_geometry(self, batch: int) -> dict:
        """the tile-count rules of a streaming decode of `batch` codewords (ldpc_debug_launch_geometry; host only): tile
        width and count, blocks per tile of the syndrome pass (1: the one-block kernel, 0: a layered schedule launches none),
        and cn_gather's XCD-affine tile count (0: tile-major) and padded grid.  NotImplementedError on an LDS-resident engine."""
        o = np.zeros(8, dtype=np.int64)
        nat.check(self._lib.ldpc_debug_launch_geometry(self.handle, int(batch), nat.ptr(o)), "ldpc_debug_launch_geometry")
        assert not o[5:].any()
        return {"vec": int(o[0]), "tiles": int(o[1]), "syndrome_chunks": int(o[2]), "gather_xcd_tiles": int(o[3]),
                "gather_tiles_padded": int(o[4])}

    # ------------------------------------------------------------------ weights
    def set_weights(self, beta: Optional[np.ndarray], alpha: Optional[np.ndarray],
                    oms_alpha: Optional[np.ndarray] = None):
        """Re-upload weight tables (same shapes) -- e.g. after loading a state_dict."""
        if beta is not None:
            beta = np.ascontiguousarray(beta, dtype=self.np_dtype).reshape(self._table_shapes[0])
        if alpha is not None:
            alpha = np.ascontiguousarray(alpha, dtype=self.np_dtype).reshape(self._table_shapes[1])
        if oms_alpha is not None:
            oms_alpha = np.ascontiguousarray(oms_alpha, dtype=self.np_dtype).reshape(self._table_shapes[2])
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            nat.check(self._lib.ldpc_decoder_set_weights(self.handle, nat.ptr(beta), nat.ptr(alpha),
                                                         nat.ptr(oms_alpha), C.c_void_p(stream.cuda_stream)),
                      "ldpc_decoder_set_weights")
            stream.synchronize()     # pageable host arrays: make the upload complete before they die
        if beta is not None:
            self._tables[0] = beta.copy()
        if alpha is not None:
            self._tables[1] = alpha.copy()
        if oms_alpha is not None:
            self._tables[2] = oms_alpha.copy()

    def set_quantizers(self, thresholds: np.ndarray):
        """Replace the quantiser tables of an RCQ engine (ldpc_decoder_set_quantizers): float32 [n_quantizers, n_levels], the
        shape it was created with.  Everything the native decoder derives from the threshold values is derived again, so
        the engine decodes and trains exactly as one created with this table; the handle, the plans and the weights stay.
        NotImplementedError on an engine without a quantiser, and when the mode is forced to 'pair' and the table does not
        admit that form (the engine then keeps its old table)."""
        if self.c2v_form != nat.C2V_RCQ:
            raise NotImplementedError("set_quantizers: the engine has no quantiser (RCQ decoders only)")
        thr = np.ascontiguousarray(thresholds, dtype=np.float32)
        if thr.shape != self._thresholds.shape:
            raise ValueError(f"thresholds must have shape {self._thresholds.shape}, got {thr.shape}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            nat.check(self._lib.ldpc_decoder_set_quantizers(self.handle, nat.ptr(thr), C.c_void_p(stream.cuda_stream)),
                      "ldpc_decoder_set_quantizers")
            stream.synchronize()     # pageable host array: make the upload complete before it dies
        self._thresholds = thr.copy()
        with self._ws_lock:          # the streaming form, and with it the workspace layout, may have changed
            self._ws.clear()
        return self

    def current_thresholds(self) -> Optional[np.ndarray]:
        """numpy copy of the quantiser table [n_quantizers, n_levels] the device holds (None: no quantiser)"""
        thr = getattr(self, "_thresholds", None)
        return None if thr is None else thr.copy()

    def current_tables(self):
        """(beta [T, Sb], alpha [T, Sa], oms_alpha [T, So] | None) numpy copies of the tables the device holds"""
        return tuple(self._tables)

    # ------------------------------------------------------------------ decode
    def workspace_bytes(self, batch: int) -> int:
        return int(self._lib.ldpc_decoder_workspace_bytes(self.handle, int(batch)))

    _WS_MAX = 4          # workspaces kept (one per recently used stream); a multi-GB buffer each on the big codes

    def _workspace(self, batch: int) -> torch.Tensor:
        """the current stream's scratch buffer (grown on demand, never shared between streams).  The cache is a small
        LRU: a caller cycling through short-lived torch streams does not pile up one buffer per stream -- an evicted buffer
        goes back to torch's caching allocator, which keeps it alive for the work already queued on its stream."""
        need = self.workspace_bytes(batch)
        key = torch.cuda.current_stream(self.device).cuda_stream
        with self._ws_lock:
            ws = self._ws.pop(key, None)
            if ws is None or ws.numel() < need:
                ws = None
                ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws                     # most recently used last
            while len(self._ws) > self._WS_MAX:
                self._ws.popitem(last=False)
            return ws

    def decode(self, llr: torch.Tensor, *, early_stop: bool = True, want_bits: bool = True,
               want_posterior: bool = True, want_packed: bool = False, max_iters: Optional[int] = None) -> DecodeResult:
        """llr: [B, n] tensor on this engine's GPU, dtype == engine dtype.  max_iters: run at most that many of the decoder's
        iterations (ldpc_decode_capped; a codeword open at the cap reports iterations = cap, success = False)."""
        if llr.device != self.device:
            raise ValueError(f"llr is on {llr.device}, engine on {self.device}")
        if llr.dtype != self.dtype:
            raise TypeError(f"llr dtype {llr.dtype} != engine dtype {self.dtype}")
        if llr.dim() != 2 or llr.shape[1] != self.graph.n:
            raise ValueError(f"llr must have shape [B, {self.graph.n}], got {tuple(llr.shape)}")
        llr = llr.contiguous()
        B, n = llr.shape
        dev = self.device
        bits = torch.empty((B, n), dtype=torch.int32, device=dev) if want_bits else None
        post = torch.empty((B, n), dtype=self.dtype, device=dev) if want_posterior else None
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        succ = torch.empty((B,), dtype=torch.uint8, device=dev)
        packed = torch.empty((B, (n + 7) // 8), dtype=torch.uint8, device=dev) if want_packed else None
        if B > 0:
            ws = self._workspace(B)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
                if max_iters is None:
                    nat.check(self._lib.ldpc_decode(self.handle, p(llr), B, int(bool(early_stop)), p(bits), p(post),
                                                    p(iters), p(succ), p(packed), p(ws), ws.numel(),
                                                    C.c_void_p(stream)), "ldpc_decode")
                else:
                    nat.check(self._lib.ldpc_decode_capped(self.handle, p(llr), B, int(bool(early_stop)), int(max_iters),
                                                           p(bits), p(post), p(iters), p(succ), p(packed), p(ws),
                                                           ws.numel(), C.c_void_p(stream)), "ldpc_decode_capped")
        return DecodeResult(bits, post, iters, succ.bool(), packed)

    def decode_iterative(self, received: torch.Tensor, *, modulation, rounds: int, demapper: Optional[str] = None,
                         prior_scale: float = 1.0, early_stop: bool = True, want_bits: bool = True,
                         want_posterior: bool = True, want_packed: bool = False, llr: Optional[torch.Tensor] = None) -> DecodeResult:
        """Iterative demapping with decoder feedback (BICM-ID) on received samples [B, S, 4] of a
        modulation.Constellation, fp32 engines only.  Round 1 is ``decode(demap(received))``.  Round r > 1 demaps again with the
        decoder's extrinsic as the a priori LLRs, ``demap(received, prior=posterior_{r-1}, prior_sub=llr_{r-1},
        prior_scale=prior_scale)``, and decodes those LLRs from scratch.  With early_stop a frame closes at the first round
        whose decode reports success and keeps that round's outputs; its `iterations` is the sum over the rounds it ran; a frame
        never closed has the last round's outputs and success False.  Without early_stop every frame runs every round and
        reports the last.  The result is per frame: the still-open frames are compacted between rounds, which changes nothing
        (a frame's demap and decode do not depend on its neighbours).  DecodeResult.rounds: int32 [B], rounds run.
        llr: round 1's LLRs where the caller already has them -- what ``sym_llr(want_received=True)`` returned beside the
        samples, i.e. ``demap(received)`` under the same demapper -- so that round 1 does not demap again; left unchanged."""
        if self.dtype != torch.float32:
            raise TypeError("decode_iterative needs an fp32 engine: the demapper's LLRs are fp32")
        if isinstance(rounds, bool) or not isinstance(rounds, (int, np.integer)) or int(rounds) < 1:
            raise ValueError(f"rounds must be an integer >= 1, got {rounds!r}")
        rounds, n, dev = int(rounds), self.graph.n, self.device
        if not _is_constellation(_check_modulation(modulation)):
            raise ValueError("decode_iterative needs a modulation.Constellation (Constellation.from_modulation gives a named "
                             "scheme's table)")
        if not isinstance(received, torch.Tensor) or received.device != dev:
            raise ValueError(f"received must be a tensor on the engine's device {dev}")
        kw = dict(early_stop=early_stop, want_bits=want_bits, want_posterior=True, want_packed=want_packed)
        own = llr is None                          # whether `llr` is this call's to overwrite
        if own:
            llr = demap(received, n, modulation=modulation, demapper=demapper)
        elif (not isinstance(llr, torch.Tensor) or llr.dtype != torch.float32 or llr.device != dev or not llr.is_contiguous()
              or received.dim() != 3 or tuple(llr.shape) != (int(received.shape[0]), n)):
            raise ValueError(f"llr must be a contiguous float32 tensor [batch, {n}] on the engine's device: demap(received)")
        res = self.decode(llr, **kw)
        B = int(llr.shape[0])
        out = DecodeResult(res.bits, res.posterior, res.iterations, res.success, res.packed_bits,
                           torch.ones((B,), dtype=torch.int32, device=dev))
        idx = None                                 # rows of `out` the current sub-batch holds; None: all of them
        for _ in range(1, rounds):
            if early_stop:                         # only the frames still open go on
                keep = torch.nonzero(~res.success, as_tuple=False).reshape(-1)
                if keep.numel() == 0:
                    break
                if keep.numel() != res.success.numel():
                    received = received.index_select(0, keep)
                    llr, own = llr.index_select(0, keep), True
                    res.posterior = res.posterior.index_select(0, keep)
                    idx = keep if idx is None else idx.index_select(0, keep)
            # the decoder's extrinsic, posterior - llr, formed in the kernel; the new LLRs take the old ones' place
            llr = demap(received, n, modulation=modulation, demapper=demapper, prior=res.posterior, prior_sub=llr,
                        prior_scale=prior_scale, out=llr if own else None)
            own = True
            res = self.decode(llr, **kw)
            rows = slice(None) if idx is None else idx
            for name in ("bits", "posterior", "packed_bits", "success"):
                if getattr(out, name) is not None:
                    getattr(out, name)[rows] = getattr(res, name)
            if early_stop:
                out.iterations[rows] += res.iterations
            else:
                out.iterations[rows] = res.iterations
            out.rounds[rows] += 1
        if not want_posterior:
            out.posterior = None
        return out

    # ------------------------------------------------------------------ on-device Monte-Carlo
    def _packed_codeword(self, codeword) -> Optional[torch.Tensor]:
        if codeword is None or isinstance(codeword, torch.Tensor):
            return codeword
        if isinstance(codeword, str):
            raise ValueError(f"codeword must be None, a 0/1 array, a packed uint8 tensor or (simulate) 'random', got {codeword!r}")
        return pack_codeword(codeword, self.graph.n, self.device)

    def encoder(self):
        """the codes.Encoder of this engine's graph (Encoder.from_graph, built once): what simulate(codeword="random") draws with"""
        enc = getattr(self, "_encoder", None)
        if enc is None:
            from codes import Encoder
            enc = self._encoder = Encoder.from_graph(self.graph)
        return enc

    def sim_diag_buffer(self, capture: int = 0) -> torch.Tensor:
        """a zeroed diag buffer for sim_count(diag=...) with room for `capture` frame-error records (int64 on this engine's GPU)"""
        return torch.zeros(sim_diag_words(self.iters, capture), dtype=torch.int64, device=self.device)

    def sim_count(self, state: torch.Tensor, packed_bits: torch.Tensor, iterations: torch.Tensor, *, max_frames: int,
                  max_errors: int, codeword=None, success: Optional[torch.Tensor] = None,
                  diag: Optional[torch.Tensor] = None, first_frame: int = 0, capture: int = 0,
                  rate_matching=None) -> torch.Tensor:
        """Fold one decoded block into `state` (int64 [8] on this engine's GPU, zeroed by the caller to start a point:
        frames, frame_errors, bit_errors, iterations, done, blocks_seen, 0, 0) with the reference's in-order stop rule
        (ldpc_sim_count).  packed_bits uint8 [B, ceil(n/8)] and iterations int32 [B] as decode(want_packed=True) returns
        them.  With `diag` (sim_diag_buffer(capture), kept over the blocks of a point) the diagnostics of the consumed frames
        are kept too (ldpc_sim_count_diag; parse_sim_diag unpacks them): `success` [B] as decode returns it, `first_frame` the
        stream index of the block's first frame.  With rate_matching the counters look at its count mask only
        (ldpc_sim_count_rm / _diag_rm).  codeword: None, one codeword for every frame, or a 2-D uint8 tensor [B, ceil(n/8)] of
        one packed codeword per frame (``encode_random``).  Asynchronous; returns `state`."""
        n = self.graph.n
        rm, rm_arg = _profile(rate_matching, n, self.device)
        if state.dtype != torch.int64 or state.shape != (8,) or state.device != self.device or not state.is_contiguous():
            raise ValueError("state must be a contiguous int64 tensor of 8 words on the engine's device")
        B = int(packed_bits.shape[0]) if packed_bits.dim() == 2 else -1
        if packed_bits.dtype != torch.uint8 or B < 0 or packed_bits.shape[1] != (n + 7) // 8 or packed_bits.device != self.device:
            raise ValueError(f"packed_bits must be uint8 [B, {(n + 7) // 8}] on the engine's device")
        if iterations.dtype != torch.int32 or iterations.shape != (B,) or iterations.device != self.device:
            raise ValueError("iterations must be int32 [B] on the engine's device")
        packed_bits, iterations = packed_bits.contiguous(), iterations.contiguous()
        if isinstance(codeword, torch.Tensor) and codeword.dim() == 2:
            # one codeword per frame: the code is linear, so the decisions XORed with the rows are counted against the
            # all-zero word (out of place: the caller's packed_bits stay as they are)
            packed_bits = torch.bitwise_xor(packed_bits, _codeword_rows(codeword, B, n, self.device))
            codeword = None
        cw = self._packed_codeword(codeword)
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        if diag is None:
            if success is not None or capture:
                raise ValueError("success and capture belong to the diagnostic counters: give diag (sim_diag_buffer)")
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream(self.device).cuda_stream
                args = (p(state), p(packed_bits), p(iterations), B, n, p(cw), int(max_frames), int(max_errors))
                if rm is None:
                    nat.check(self._lib.ldpc_sim_count(*args, C.c_void_p(stream)), "ldpc_sim_count")
                else:
                    nat.check(self._lib.ldpc_sim_count_rm(*args, rm_arg, C.c_void_p(stream)), "ldpc_sim_count_rm")
            return state
        capture = int(capture)
        if capture < 0:
            raise ValueError("capture must be >= 0")
        if (diag.dtype != torch.int64 or diag.shape != (sim_diag_words(self.iters, capture),) or diag.device != self.device
                or not diag.is_contiguous()):
            raise ValueError(f"diag must be a contiguous int64 tensor of {sim_diag_words(self.iters, capture)} words on the "
                             f"engine's device (sim_diag_buffer({capture}))")
        if success is None or success.dtype not in (torch.bool, torch.uint8) or success.shape != (B,) or success.device != self.device:
            raise ValueError("the diagnostic counters need success, bool or uint8 [B] on the engine's device")
        success = success.to(torch.uint8).contiguous()
        need = int(self._lib.ldpc_sim_count_diag_scratch_bytes(B))
        with torch.cuda.device(self.device):
            scratch = torch.empty(max(need, 4), dtype=torch.uint8, device=self.device)   # stream-ordered by the allocator
            stream = torch.cuda.current_stream(self.device).cuda_stream
            args = (p(state), p(diag), int(self.iters), capture, p(packed_bits), p(iterations), p(success), B, n, p(cw),
                    int(first_frame) & (2 ** 64 - 1), int(max_frames), int(max_errors), p(scratch), scratch.numel())
            if rm is None:
                nat.check(self._lib.ldpc_sim_count_diag(*args, C.c_void_p(stream)), "ldpc_sim_count_diag")
            else:
                nat.check(self._lib.ldpc_sim_count_diag_rm(*args, rm_arg, C.c_void_p(stream)), "ldpc_sim_count_diag_rm")
        return state

    def simulate(self, *, seed: int, max_frames: int, max_errors: int, stream_id: int = 0, first_frame: int = 0,
                 snr_db: Optional[float] = None, scale: Optional[float] = None, shift: Optional[float] = None,
                 codeword=None, block: int = 65536, poll_blocks: int = 4, diagnostics: bool = False,
                 capture: int = 0, rate_matching=None, modulation=None, amp: Optional[float] = None) -> dict:
        """One SNR point on the device (ldpc_simulate): blocks of `block` frames of the counter-based AWGN stream, early-stop
        decode, in-order error counters, one host round trip every `poll_blocks` blocks.  -> {frames, frame_errors,
        bit_errors, iterations, done, blocks_seen}; all but blocks_seen are independent of block and poll_blocks.
        With diagnostics (ldpc_simulate_diag) also undetected_errors (the decisions satisfy H and are not the codeword),
        detected_errors, iteration_histogram (np.int64 [T + 1] over the consumed frames), captured and error_frames: the
        first `capture` frame errors as a structured array (frame, wrong_bits, iterations, undetected) -- awgn_llr(1, n,
        first_frame=frame, ...) draws such a frame again.  rate_matching: the profile on the channel and the counters
        (ldpc_simulate_rm / _diag_rm).  codeword="random": a fresh codeword per frame, drawn on the device from the point's
        seed, stream_id and frame index with the encoder of this engine's graph (ldpc_simulate_enc); a recorded frame's
        codeword is ``encode_random(self.encoder(), 1, first_frame=frame, ...)``.  modulation: a modulation.Modulation -- the
        point runs on the symbol channel of ``sym_llr`` (ldpc_simulate_sym) at snr_db or `amp`; scale / shift and
        rate_matching do not apply to it.  Synchronous."""
        if modulation is not None:
            return self._simulate_sym(_check_modulation(modulation), seed=seed, max_frames=max_frames, max_errors=max_errors,
                                      stream_id=stream_id, first_frame=first_frame, snr_db=snr_db, amp=amp, scale=scale,
                                      shift=shift, codeword=codeword, block=block, poll_blocks=poll_blocks,
                                      diagnostics=diagnostics, capture=capture, rate_matching=rate_matching)
        if amp is not None:
            raise ValueError("amp belongs to a modulation: give snr_db or (scale, shift)")
        if (snr_db is None) == (scale is None or shift is None):
            raise ValueError("give either snr_db or both scale and shift")
        if snr_db is not None:
            scale, shift = awgn_scale_shift(snr_db)
        random = isinstance(codeword, str)
        if random and codeword != "random":
            raise ValueError(f"codeword must be None, a 0/1 array, a packed uint8 tensor or 'random', got {codeword!r}")
        ne = _NativeEncoder.get(self.encoder(), self.device) if random else None
        cw = None if random else self._packed_codeword(codeword)
        rm, rm_arg = _profile(rate_matching, self.graph.n, self.device)
        desc = nat.SimDesc()
        desc.seed, desc.stream_id = int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1)
        desc.first_frame = int(first_frame) & (2 ** 64 - 1)
        desc.scale, desc.shift = float(scale), float(shift)
        desc.codeword_packed = None if cw is None else cw.data_ptr()
        desc.max_frames, desc.max_errors = int(max_frames), int(max_errors)
        desc.block, desc.poll_blocks = int(block), int(poll_blocks)
        out = np.zeros(8, dtype=np.int64)
        capture = int(capture)
        if capture < 0 or (capture and not diagnostics):
            raise ValueError("capture must be >= 0 and needs diagnostics=True")
        words = np.zeros(sim_diag_words(self.iters, capture), dtype=np.int64) if diagnostics else None
        if random:
            need = int(self._lib.ldpc_simulate_enc_workspace_bytes(self.handle, max(int(block), 1), capture if diagnostics else -1))
        elif diagnostics:
            need = int(self._lib.ldpc_simulate_diag_workspace_bytes(self.handle, max(int(block), 1), capture))
        else:
            need = int(self._lib.ldpc_simulate_workspace_bytes(self.handle, max(int(block), 1)))
        ws = getattr(self, "_sim_ws", None)
        if ws is None or ws.numel() < need:
            self._sim_ws = None
            self._sim_ws = ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            tail = (C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream))
            if random:
                nat.check(self._lib.ldpc_simulate_enc(self.handle, C.byref(desc), ne.handle, rm_arg, capture if diagnostics else -1,
                                                      nat.ptr(out), nat.ptr(words), *tail), "ldpc_simulate_enc")
            elif rm is not None and diagnostics:
                nat.check(self._lib.ldpc_simulate_diag_rm(self.handle, C.byref(desc), rm_arg, capture, nat.ptr(out),
                                                          nat.ptr(words), *tail), "ldpc_simulate_diag_rm")
            elif rm is not None:
                nat.check(self._lib.ldpc_simulate_rm(self.handle, C.byref(desc), rm_arg, nat.ptr(out), *tail), "ldpc_simulate_rm")
            elif diagnostics:
                nat.check(self._lib.ldpc_simulate_diag(self.handle, C.byref(desc), capture, nat.ptr(out), nat.ptr(words),
                                                       C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream)),
                          "ldpc_simulate_diag")
            else:
                nat.check(self._lib.ldpc_simulate(self.handle, C.byref(desc), nat.ptr(out), C.c_void_p(ws.data_ptr()),
                                                  ws.numel(), C.c_void_p(stream)), "ldpc_simulate")
        res = {k: int(v) for k, v in zip(SIM_COUNTERS, out)}
        if diagnostics:
            res.update(parse_sim_diag(words, self.iters, capture))
            res["detected_errors"] = res["frame_errors"] - res["undetected_errors"]
        return res

    def _simulate_sym(self, mod, *, seed, max_frames, max_errors, stream_id, first_frame, snr_db, amp, scale, shift, codeword,
                      block, poll_blocks, diagnostics, capture, rate_matching) -> dict:
        """simulate(modulation=mod): one native call of ldpc_simulate_sym"""
        if rate_matching is not None:
            raise ValueError("rate matching together with a modulation is not provided")
        if scale is not None or shift is not None:
            raise ValueError("scale and shift belong to the BI-AWGN channel: with a modulation give snr_db or amp")
        amp = _symbol_amp(mod, snr_db, amp)
        random = isinstance(codeword, str)                     # (a float64 engine is refused by the native call)
        if random and codeword != "random":
            raise ValueError(f"codeword must be None, a 0/1 array, a packed uint8 tensor or 'random', got {codeword!r}")
        ne = _NativeEncoder.get(self.encoder(), self.device) if random else None
        cw = None if random else _channel_codeword(codeword, self.graph.n, self.device)
        mdesc, _keep = mod.native(amp, self.graph.n, self.device)
        desc = nat.SimDesc()
        desc.seed, desc.stream_id = int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 32 - 1)
        desc.first_frame = int(first_frame) & (2 ** 64 - 1)
        desc.scale, desc.shift = 0.0, 0.0
        desc.codeword_packed = None if cw is None else cw.data_ptr()
        desc.max_frames, desc.max_errors = int(max_frames), int(max_errors)
        desc.block, desc.poll_blocks = int(block), int(poll_blocks)
        out = np.zeros(8, dtype=np.int64)
        capture = int(capture)
        if capture < 0 or (capture and not diagnostics):
            raise ValueError("capture must be >= 0 and needs diagnostics=True")
        words = np.zeros(sim_diag_words(self.iters, capture), dtype=np.int64) if diagnostics else None
        need = int(self._lib.ldpc_simulate_sym_workspace_bytes(self.handle, max(int(block), 1), capture if diagnostics else -1))
        ws = getattr(self, "_sim_ws", None)
        if ws is None or ws.numel() < need:
            self._sim_ws = None
            self._sim_ws = ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            head = (self.handle, C.byref(desc), None if ne is None else ne.handle, C.byref(mdesc))
            tail = (capture if diagnostics else -1, nat.ptr(out), nat.ptr(words), C.c_void_p(ws.data_ptr()), ws.numel(),
                    C.c_void_p(stream))
            if _is_constellation(mod):
                from modulation import DEMAPPERS
                nat.check(self._lib.ldpc_simulate_con(*head, DEMAPPERS[mod.demapper], *tail), "ldpc_simulate_con")
            elif mod.demapper == "exact":
                nat.check(self._lib.ldpc_simulate_sym_dm(*head, nat.DEMAP_EXACT, *tail), "ldpc_simulate_sym_dm")
            else:
                nat.check(self._lib.ldpc_simulate_sym(*head, *tail), "ldpc_simulate_sym")
        res = {k: int(v) for k, v in zip(SIM_COUNTERS, out)}
        if diagnostics:
            res.update(parse_sim_diag(words, self.iters, capture))
            res["detected_errors"] = res["frame_errors"] - res["undetected_errors"]
        return res

    # ------------------------------------------------------------------ small host batches (the reference's call shape)
    HOST_BATCH_MAX = 64

    def decode_host(self, llr_host: torch.Tensor, *, early_stop: bool = True, want_posterior: bool = True):
        """Decode a SMALL batch that lives in host memory (the reference's own call: one CPU vector in, CPU results out)
        with one staged copy each way: pinned host buffers and device buffers are kept per engine, the LLRs go up in one
        async copy, ldpc_decode writes bits / posterior / iterations / success into ONE device block laid out for THIS
        batch size (a one-codeword call moves ~2n words back, not the 64-row block), that block comes back in one async
        copy, one stream synchronise.  -> (bits int32 [B, n], posterior | None, iterations int32 [B], success bool [B])
        as CPU tensors (fresh copies).  The staging buffers have their own lock (decode() on other threads is not
        blocked while this call waits for the device)."""
        if llr_host.dim() != 2 or llr_host.shape[1] != self.graph.n or llr_host.shape[0] > self.HOST_BATCH_MAX:
            raise ValueError(f"decode_host takes [B <= {self.HOST_BATCH_MAX}, {self.graph.n}] host tensors")
        B, n = llr_host.shape
        es = 4 if self.dtype == torch.float32 else 8
        with self._host_lock:
            st = getattr(self, "_host_stage", None)
            if st is None:
                Bm = self.HOST_BATCH_MAX
                total = (Bm * n * 4 + Bm * n * es + Bm * 4 + Bm + 1024 + 255) // 256 * 256
                st = {"h_in": torch.empty((Bm, n), dtype=self.dtype, pin_memory=True),
                      "d_in": torch.empty((Bm, n), dtype=self.dtype, device=self.device),
                      "d_out": torch.empty(total, dtype=torch.uint8, device=self.device),
                      "h_out": torch.empty(total, dtype=torch.uint8, pin_memory=True), "ws": None}
                self._host_stage = st
            # block layout for B rows: bits | posterior | iterations | success, each 256-byte aligned (posterior: its dtype)
            al = lambda x: (x + 255) // 256 * 256
            o_bits = 0
            o_post = al(B * n * 4)
            o_it = o_post + (al(B * n * es) if want_posterior else 0)
            o_ok = o_it + al(B * 4)
            used = o_ok + B
            st["h_in"][:B].copy_(llr_host)
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream(self.device)
                st["d_in"][:B].copy_(st["h_in"][:B], non_blocking=True)
                need = self.workspace_bytes(B)
                if st["ws"] is None or st["ws"].numel() < need:
                    st["ws"] = torch.empty(need, dtype=torch.uint8, device=self.device)
                base = st["d_out"].data_ptr()
                nat.check(self._lib.ldpc_decode(self.handle, C.c_void_p(st["d_in"].data_ptr()), B, int(bool(early_stop)),
                                                C.c_void_p(base + o_bits), C.c_void_p(base + o_post) if want_posterior else None,
                                                C.c_void_p(base + o_it), C.c_void_p(base + o_ok), None,
                                                C.c_void_p(st["ws"].data_ptr()), st["ws"].numel(),
                                                C.c_void_p(stream.cuda_stream)), "ldpc_decode")
                st["h_out"][:used].copy_(st["d_out"][:used], non_blocking=True)
                stream.synchronize()
            h = st["h_out"]
            bits = h[o_bits:o_bits + B * n * 4].view(torch.int32).view(B, n).clone()
            post = h[o_post:o_post + B * n * es].view(self.dtype).view(B, n).clone() if want_posterior else None
            iters = h[o_it:o_it + B * 4].view(torch.int32).clone()
            succ = h[o_ok:o_ok + B].clone().bool()
        return bits, post, iters, succ

    def decode_host_op(self, llr_host: torch.Tensor, *, early_stop: bool = True, want_posterior: bool = True) -> DecodeResult:
        """decode_host() through ``torch.ops.ldpc.decode_host`` -> DecodeResult of CPU tensors"""
        import torch_ops
        bits, post, iters, succ = torch.ops.ldpc.decode_host(llr_host, torch_ops.engine_handle(self), bool(early_stop),
                                                             bool(want_posterior))
        return DecodeResult(bits, post if want_posterior else None, iters, succ, None)

    def decode_op(self, llr: torch.Tensor, *, early_stop: bool = True, want_posterior: bool = True,
                  want_packed: bool = False) -> DecodeResult:
        """decode() entered through the registered PyTorch operator ``torch.ops.ldpc.decode`` (torch_ops.py) --
        the call the host decoder classes make"""
        import torch_ops
        bits, post, iters, succ, packed = torch.ops.ldpc.decode(llr, torch_ops.engine_handle(self), bool(early_stop),
                                                                bool(want_posterior), bool(want_packed))
        return DecodeResult(bits, post if want_posterior else None, iters, succ, packed if want_packed else None)

    # ------------------------------------------------------------------ gradients (training path)
    def _check_llr(self, llr: torch.Tensor) -> torch.Tensor:
        if llr.device != self.device:
            raise ValueError(f"llr is on {llr.device}, engine on {self.device}")
        if llr.dtype != self.dtype:
            raise TypeError(f"llr dtype {llr.dtype} != engine dtype {self.dtype}")
        if llr.dim() != 2 or llr.shape[1] != self.graph.n:
            raise ValueError(f"llr must have shape [B, {self.graph.n}], got {tuple(llr.shape)}")
        return llr.contiguous()

    def _train_workspace(self, batch: int) -> torch.Tensor:
        need = int(self._lib.ldpc_train_workspace_bytes(self.handle, batch))
        ws = getattr(self, "_train_ws", None)
        if ws is None or ws.numel() < need:
            self._train_ws = None
            self._train_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._train_ws

    def train_saved_bytes(self, batch: int) -> int:
        return int(self._lib.ldpc_train_saved_bytes(self.handle, max(int(batch), 1)))

    def decode_saving(self, llr: torch.Tensor, *, early_stop: bool = True):
        """decode() that also keeps every iteration's messages for backward(); returns (DecodeResult, saved).
        fp32 normalised min-sum decoders only (NotImplementedError otherwise)."""
        llr = self._check_llr(llr)
        B, n = llr.shape
        dev = self.device
        bits = torch.empty((B, n), dtype=torch.int32, device=dev)
        post = torch.empty((B, n), dtype=self.dtype, device=dev)
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        succ = torch.empty((B,), dtype=torch.uint8, device=dev)
        # the saved messages become a saved tensor of the autograd node (torch_ops.py): allocated per call, freed with the graph
        saved = torch.empty(int(self._lib.ldpc_train_saved_bytes(self.handle, max(B, 1))), dtype=torch.uint8, device=dev)
        if B > 0:
            ws = self._train_workspace(B)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                p = lambda t: C.c_void_p(t.data_ptr())
                nat.check(self._lib.ldpc_decode_saving(self.handle, p(llr), B, int(bool(early_stop)), p(bits), p(post),
                                                       p(iters), p(succ), p(saved), saved.numel(), p(ws), ws.numel(),
                                                       C.c_void_p(stream)), "ldpc_decode_saving")
        return DecodeResult(bits, post, iters, succ.bool(), None), saved

    def backward(self, saved: torch.Tensor, llr: torch.Tensor, iterations: torch.Tensor, grad_posterior: torch.Tensor,
                 want_grad_llr: bool = False):
        """(d loss/d beta [T, beta slots], d loss/d alpha [T, alpha slots], d loss/d oms_alpha [T, slots] | None)
        for a loss with d loss/d posterior = grad_posterior [B, n]; `saved`, `iterations` from decode_saving of the
        same llr with the same weight tables.  want_grad_llr: also return d loss/d llr [B, n]."""
        llr = self._check_llr(llr)
        B, n = llr.shape
        dev = self.device
        gp = grad_posterior.to(device=dev, dtype=torch.float32).contiguous()
        if gp.shape != llr.shape:
            raise ValueError(f"grad_posterior must have shape {tuple(llr.shape)}, got {tuple(gp.shape)}")
        iterations = iterations.to(device=dev, dtype=torch.int32).contiguous()
        if iterations.shape != (B,):
            raise ValueError("iterations must have one entry per codeword")
        gb = torch.zeros(self._table_shapes[0], dtype=torch.float32, device=dev)
        ga = torch.zeros(self._table_shapes[1], dtype=torch.float32, device=dev)
        goa = None if self._table_shapes[2] is None else torch.zeros(self._table_shapes[2], dtype=torch.float32, device=dev)
        gl = torch.zeros((B, n), dtype=torch.float32, device=dev) if want_grad_llr else None
        if B > 0:
            ws = self._train_workspace(B)
            with torch.cuda.device(dev):
                stream = torch.cuda.current_stream(dev).cuda_stream
                p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
                nat.check(self._lib.ldpc_backward(self.handle, p(saved), saved.numel(), p(llr), B, p(iterations), p(gp),
                                                  p(gb), p(ga), p(goa), p(gl), p(ws), ws.numel(), C.c_void_p(stream)),
                          "ldpc_backward")
        if want_grad_llr:
            return gb, ga, goa, gl
        return gb, ga, goa

    # ------------------------------------------------------------------ posterior joint training
    def train_joint_workspace_bytes(self, batch: int) -> int:
        return int(self._lib.ldpc_train_joint_workspace_bytes(self.handle, int(batch)))

    def train_joint_ste_workspace_bytes(self, batch: int) -> int:
        return int(self._lib.ldpc_train_joint_ste_workspace_bytes(self.handle, int(batch)))

    def train_joint_layered_workspace_bytes(self, batch: int) -> int:
        return int(self._lib.ldpc_train_joint_layered_workspace_bytes(self.handle, int(batch)))

    def train_joint_layered_ste_workspace_bytes(self, batch: int) -> int:
        return int(self._lib.ldpc_train_joint_layered_ste_workspace_bytes(self.handle, int(batch)))

    def train_joint_layered_ste(self, llr: torch.Tensor, targets: Optional[torch.Tensor] = None,
                                iteration_weights: Optional[torch.Tensor] = None, want_grads: bool = True,
                                want_grad_llr: bool = False, want_levels: bool = False) -> dict:
        """train_joint() of the quantised decoder under the paper's layered schedule (ldpc_train_joint_layered_ste): the
        fixed-T layered W-RCQ decode, unchanged, one iteration per launch, with the layered posterior-local gradients of J
        formed through the straight-through rule of include/ldpc_hip.h (iteration t's loss reaches beta_t and the LLRs
        through the check update that wrote each message; gradient 1 through the quantiser below its top level, 0 where
        the code saturated).  Same arguments and the same dict as train_joint_ste; "grad_alpha" (the table the schedule
        does not use) is all zero.  ``want_levels``: as in train_joint_ste (ldpc_train_joint_layered_ste_levels).
        NotImplementedError for every other decoder."""
        return self._train_joint(llr, targets, iteration_weights, want_grads, want_grad_llr,
                                 kind="layered_ste_levels" if want_levels else "layered_ste")

    def train_joint_layered(self, llr: torch.Tensor, targets: Optional[torch.Tensor] = None,
                            iteration_weights: Optional[torch.Tensor] = None, want_grads: bool = True,
                            want_grad_llr: bool = False) -> dict:
        """train_joint() of a layered normalised / offset min-sum decoder (ldpc_train_joint_layered): the fixed-T layered
        decode, unchanged, one iteration per launch, with the layered posterior-local gradients of J defined in
        include/ldpc_hip.h (iteration t's loss reaches beta_t, the check-side offset alpha_t and the LLRs through the
        check update alone).  Same arguments and the same dict as train_joint; "grad_alpha" (the variable-side table
        the schedule does not use) is all zero.  NotImplementedError for every other decoder."""
        return self._train_joint(llr, targets, iteration_weights, want_grads, want_grad_llr, kind="layered")

    def train_joint_ste(self, llr: torch.Tensor, targets: Optional[torch.Tensor] = None,
                        iteration_weights: Optional[torch.Tensor] = None, want_grads: bool = True,
                        want_grad_llr: bool = False, want_levels: bool = False) -> dict:
        """train_joint() of the quantised decoder (ldpc_train_joint_ste): the fp32 RCQ flooding decode, unchanged, with
        the posterior-local gradients of J formed through the straight-through rule of include/ldpc_hip.h (gradient 1
        through the quantiser below its top level, 0 where the code saturated).  Same arguments and the same dict as
        train_joint ("grad_oms_alpha" is always None); NotImplementedError for every other decoder.
        ``want_levels``: the call goes through ldpc_train_joint_ste_levels and the dict gains "grad_levels" [T, n_levels]:
        d J_t / d (reconstruction value of level l) in row t, the signed per-level sum of the seed over the codes the
        forward stored (include/ldpc_hip.h); every other entry is bit-identical to the call without it."""
        return self._train_joint(llr, targets, iteration_weights, want_grads, want_grad_llr,
                                 kind="ste_levels" if want_levels else "ste")

    def train_joint(self, llr: torch.Tensor, targets: Optional[torch.Tensor] = None,
                    iteration_weights: Optional[torch.Tensor] = None, want_grads: bool = True,
                    want_grad_llr: bool = False) -> dict:
        """Fixed-T decode with the loss on every iteration's posterior (ldpc_train_joint):
        J_t = mean BCEWithLogits(-posterior_t, targets), J = sum_t w_t J_t, and -- want_grads -- the posterior-local
        gradients of J (include/ldpc_hip.h).  targets [B, n] in [0, 1] (None: all zero), iteration_weights [T]
        (None: 1/T each).  fp32 normalised / offset min-sum decoders only (NotImplementedError otherwise).
        -> {"loss": 0-d, "loss_per_iter": [T], "bits": int32 [B, n], "posterior": [B, n] (of the last iteration),
            "grad_beta", "grad_alpha": [T, slots] | None, "grad_oms_alpha": [T, slots] | None, "grad_llr": [B, n] | None}
        Everything on this engine's device, fp32."""
        return self._train_joint(llr, targets, iteration_weights, want_grads, want_grad_llr, kind="minsum")

    # kind -> (entry point, its workspace-bytes function, the entry point takes grad_oms_alpha)
    _JOINT_ENTRY = {"minsum": ("ldpc_train_joint", "ldpc_train_joint_workspace_bytes", True),
                    "ste": ("ldpc_train_joint_ste", "ldpc_train_joint_ste_workspace_bytes", False),
                    "layered": ("ldpc_train_joint_layered", "ldpc_train_joint_layered_workspace_bytes", True),
                    "layered_ste": ("ldpc_train_joint_layered_ste", "ldpc_train_joint_layered_ste_workspace_bytes", False),
                    "ste_levels": ("ldpc_train_joint_ste_levels", "ldpc_train_joint_ste_levels_workspace_bytes", False),
                    "layered_ste_levels": ("ldpc_train_joint_layered_ste_levels",
                                           "ldpc_train_joint_layered_ste_levels_workspace_bytes", False)}

    def _train_joint(self, llr, targets, iteration_weights, want_grads, want_grad_llr, kind: str) -> dict:
        entry, ws_bytes, has_goa = self._JOINT_ENTRY[kind]
        want_levels = kind.endswith("_levels")      # those entry points take grad_levels after grad_llr
        llr = self._check_llr(llr)
        B, n = llr.shape
        dev = self.device
        T = self.iters
        if targets is not None:
            targets = targets.to(device=dev, dtype=torch.float32).contiguous()
            if targets.shape != llr.shape:
                raise ValueError(f"targets must have shape {tuple(llr.shape)}, got {tuple(targets.shape)}")
        if iteration_weights is None:
            w = torch.full((max(T, 1),), 1.0 / max(T, 1), dtype=torch.float32, device=dev)
        else:
            w = torch.as_tensor(iteration_weights).to(device=dev, dtype=torch.float32).contiguous()
            if w.shape != (T,):
                raise ValueError(f"iteration_weights must have shape ({T},), got {tuple(w.shape)}")
        lpi = torch.empty((T,), dtype=torch.float32, device=dev)
        bits = torch.empty((B, n), dtype=torch.int32, device=dev)
        post = torch.empty((B, n), dtype=torch.float32, device=dev)
        gb = torch.empty(self._table_shapes[0], dtype=torch.float32, device=dev) if want_grads else None
        ga = torch.empty(self._table_shapes[1], dtype=torch.float32, device=dev) if want_grads else None
        goa = (torch.empty(self._table_shapes[2], dtype=torch.float32, device=dev)
               if want_grads and has_goa and self._table_shapes[2] is not None else None)
        gl = torch.empty((B, n), dtype=torch.float32, device=dev) if want_grad_llr else None
        glv = None
        if want_levels:
            if self.c2v_form != nat.C2V_RCQ:
                raise NotImplementedError("want_levels: the engine has no quantiser (RCQ decoders only)")
            glv = torch.empty((T, self._thresholds.shape[1]), dtype=torch.float32, device=dev)
        ws = None
        if B > 0:
            need = int(getattr(self._lib, ws_bytes)(self.handle, B))
            ws = getattr(self, "_joint_ws", None)
            if ws is None or ws.numel() < need:
                self._joint_ws = None
                self._joint_ws = ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
            grads = (p(gb), p(ga), p(goa), p(gl)) if has_goa else (p(gb), p(ga), p(gl))
            if want_levels:
                grads += (p(glv),)
            nat.check(getattr(self._lib, entry)(self.handle, p(llr), p(targets), B, p(w), p(lpi), p(bits), p(post), *grads,
                                                p(ws), 0 if ws is None else ws.numel(), C.c_void_p(stream)), entry)
        return {"loss": (w[:T] * lpi).sum(), "loss_per_iter": lpi, "bits": bits, "posterior": post,
                "grad_beta": gb, "grad_alpha": ga, "grad_oms_alpha": goa, "grad_llr": gl,
                **({"grad_levels": glv} if want_levels else {})}

    def debug_sweep(self, batch: int, which: int, it: int):
        """Launch one CN (which=0) or VN (which=1) sweep on the state a previous
        decode(batch) left in the workspace -- bench.py's per-kernel timing hook."""
        ws = self._workspace(batch)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            nat.check(self._lib.ldpc_debug_sweep(self.handle, int(batch), int(which), int(it),
                                                 C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(stream)),
                      "ldpc_debug_sweep")

    def debug_resident_c2v(self, llr: torch.Tensor, *, early_stop: bool = True, max_iters: Optional[int] = None):
        """LDS-resident engine: decode `llr` and also return every codeword's C2V messages of its last executed
        iteration -> (c2v [B, E] dtype values in CSR edge order, posterior [B, n], iterations [B]).  max_iters: run at
        most that many of the decoder's iterations, as decode(max_iters=...).  Test hook (include/ldpc_hip_debug.h);
        RCQ decoders hold reconstructed values, see `codes_of` in tests/test_gpu_parity.py."""
        if max_iters is not None and int(max_iters) < 1:
            raise ValueError("max_iters must be >= 1")
        llr = self._check_llr(llr)
        B, n = llr.shape
        dev = self.device
        c2v = torch.zeros((B, self.graph.E), dtype=self.dtype, device=dev)
        post = torch.empty((B, n), dtype=self.dtype, device=dev)
        iters = torch.empty((B,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            p = lambda t: C.c_void_p(t.data_ptr())
            nat.check(self._lib.ldpc_debug_resident_c2v(self.handle, p(llr), B, int(bool(early_stop)),
                                                        0 if max_iters is None else int(max_iters), p(post), p(iters),
                                                        p(c2v), C.c_void_p(stream)), "ldpc_debug_resident_c2v")
        return c2v, post, iters

    def debug_c2v(self, batch: int, max_iters: Optional[int] = None) -> torch.Tensor:
        """Streaming engine: C2V state left by the last decode(batch): [B, E] uint8 quantiser codes (RCQ) or
        dtype values, CSR edge order.  max_iters: the cap that decode ran with (decode(max_iters=...)), None: uncapped.
        Test hook (per-edge code parity with the reference)."""
        out8 = np.zeros(8, dtype=np.int64)
        cap = 0 if max_iters is None else int(max_iters)
        nat.check(self._lib.ldpc_debug_workspace_layout(self.handle, int(batch), cap, nat.ptr(out8)),
                  "ldpc_debug_workspace_layout")
        vec, tiles, off = int(out8[0]), int(out8[1]), int(out8[4])
        W, E = 64 * vec, self.graph.E
        ws = self._workspace(batch)
        if self.c2v_form == nat.C2V_RCQ:
            raw = ws[off: off + tiles * E * W].view(tiles, E, W)
        else:
            es = 4 if self.dtype == torch.float32 else 8
            raw = ws[off: off + tiles * E * W * es].view(self.dtype).view(tiles, E, W)
        return raw.permute(0, 2, 1).reshape(tiles * W, E)[:batch].contiguous()
