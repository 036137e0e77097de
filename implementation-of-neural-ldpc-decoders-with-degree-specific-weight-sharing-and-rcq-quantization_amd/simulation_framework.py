"""
Batched Monte-Carlo driver -- the natural caller of the batched engine.
Mirrors the reference module of the same name: ``SimulationConfig``, ``SimulationResult``,
``LDPSimulator`` (``simulate_single_snr`` / ``simulate_decoder`` / ``simulate_multiple_decoders``
/ ``save_results`` / ``load_results``) and ``create_test_decoders``, same field names, return
tuples and JSON layout (simulation_framework.py:27-69, 85-208, 338-420).  Plotting and the
training hooks of the reference are out of scope.

What changes underneath: the reference draws ONE noise vector with numpy and decodes ONE frame per
Python call (simulation_framework.py:110-132).  Here a block of ``batch_frames`` frames is drawn on
the GPU (``torch.randn``), decoded in one engine call with per-codeword early exit, and the error /
iteration counters are reduced on the device.  The stop rule is the reference's, applied frame by
frame: frames are taken in order until ``max_frames`` frames or ``max_errors`` frame errors have
been seen, so a block is truncated at the frame that reaches the limit.

Channel convention (``SimulationConfig.llr_convention``):
  "decoder"   (default) all-zero codeword with positive mean LLR, llr = 2(1 + sigma z)/sigma^2 --
              consistent with every decoder's ``posterior < 0 -> 1`` decision;
  "reference" the literal recipe of simulate_awgn_channel (ldpc_decoder.py:286-302): bit 0 -> -1,
              i.e. NEGATIVE mean LLR, under which the reference's own simulations report FER = 1.0
              (SURVEY 8a-9).

Channel (``SimulationConfig.channel``):
  "torch"   (default) the ``torch.randn`` draw above, counters reduced with torch and the stop rule applied on the host;
  "device"  the native Monte-Carlo path: the counter-based AWGN stream of ``engine.awgn_llr`` (seed = ``config.seed``,
            stream_id = round(snr_db * 1000) mod 2^32, frame f the same noise whatever ``batch_frames`` is), the device-side
            counters of ``DecodeEngine.sim_count``, and on the LDS-resident engine the whole point in one native call
            (``DecodeEngine.simulate``).  ``SimulationConfig.codeword`` sends a codeword other than all-zero: a 0/1 array for
            every frame, or ``"random"`` for a fresh codeword per frame, encoded on the device from the point's seed, stream
            and frame index (``engine.encode_random`` with ``codes.Encoder.from_graph`` of the decoder's graph).
            ``SimulationConfig.diagnostics`` / ``capture_errors`` (this channel only) also count the undetected frame errors,
            bin the stop iterations and record the stream index of the first ``capture_errors`` frame errors of every point
            (``SimulationResult.undetected_errors`` / ``iteration_histograms`` / ``error_frames``);
            ``LDPSimulator.replay_errors`` draws and decodes recorded frames again.
            ``SimulationConfig.rate_matching`` (this channel only) punctures and shortens bits on the channel and restricts
            the error counters to its count mask; the bit error rate is then per counted bit.
            ``SimulationConfig.modulation`` (this channel only; a ``modulation.Modulation``) sends the bits as Gray-mapped BPSK /
            QPSK / 16- / 64- / 256-QAM symbols over AWGN or per-symbol Rayleigh fading and demaps them with the modulation's
            demapper, max-log or exact (``engine.sym_llr``, DESIGN.md sections 3j and 3l); ``snr_db`` is then Es/N0 of the symbol.  Not together with
            ``rate_matching``; from 16-QAM up it needs ``codeword="random"`` (or a codeword).  A ``modulation.Constellation``
            (8-PSK, APSK, any table of up to 64 labelled points) is taken the same way and always
            needs ``codeword="random"`` (or a codeword).
            ``SimulationConfig.iterative_demapping = K`` (this channel and a ``Constellation`` only; default 1) demaps every
            frame up to K times, each round after the first with the decoder's extrinsic as a priori LLRs scaled by
            ``demapping_feedback_scale`` (``DecodeEngine.decode_iterative``).  The average iteration count
            is then the sum over the rounds a frame ran.  Not together with ``diagnostics`` / ``capture_errors``.
"""

from __future__ import annotations

import json
import logging
import os
import threading
import time
import warnings
from concurrent.futures import ThreadPoolExecutor, as_completed
from dataclasses import InitVar, dataclass
from typing import Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from ldpc_decoder import BasicMinSumDecoder, LDPCCode
from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
from modulation import Constellation, Modulation
from rate_matching import RateMatching
from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder

logger = logging.getLogger(__name__)


@dataclass
class SimulationConfig:
    """Simulation configuration (reference fields first, same defaults except `device`)"""
    snr_range: Tuple[float, float] = (0.0, 6.0)
    snr_step: float = 0.5
    max_frames: int = 10000
    max_errors: int = 100
    min_frames: int = 1000
    parallel_workers: int = 4
    device: str = "cuda"
    save_results: bool = True
    results_dir: str = "simulation_results"
    # extensions
    batch_frames: int = 8192
    seed: int = 0
    llr_convention: str = "decoder"
    staged_early_stop: bool = True          # streaming engine: cap the block's first stage, finish stragglers as a small batch
    stage_min_block: int = 1024             # ... only for blocks of at least this many frames
    channel: str = "torch"                  # "torch": torch.randn draw, host stop rule; "device": the native Monte-Carlo path
    codeword: Optional[np.ndarray] = None   # 0/1 array of length n sent instead of the all-zero codeword, or "random": a fresh
    #                                         codeword per frame from the device encoder (channel="device" only)
    poll_blocks: int = 4                    # channel="device", resident engine: blocks between two looks at the counters
    diagnostics: bool = False               # channel="device": undetected errors, stop-iteration histogram, failing frames
    capture_errors: int = 0                 # ... record the first so many frame errors of every point (implies diagnostics)
    rate_matching: Optional[RateMatching] = None   # channel="device": punctured / shortened bits and the counters' mask
    # channel="device": Gray-mapped symbols over AWGN or Rayleigh fading, max-log demapper.  An init-only argument kept as a
    # plain attribute: the dataclass fields (and with them repr, ==, the reference's field list) stay the twenty above
    modulation: InitVar[Optional[Modulation]] = None
    # channel="device" with a modulation.Constellation: demapping rounds per frame (1: demap once, today's path; K > 1:
    # iterative demapping with decoder feedback, DecodeEngine.decode_iterative) and the scale of the fed-back extrinsic.
    # Init-only and kept as plain attributes, as `modulation` is
    iterative_demapping: InitVar[int] = 1
    demapping_feedback_scale: InitVar[float] = 1.0

    def __post_init__(self, modulation=None, iterative_demapping=1, demapping_feedback_scale=1.0):
        self.modulation = modulation
        if isinstance(iterative_demapping, bool) or not isinstance(iterative_demapping, (int, np.integer)) \
                or int(iterative_demapping) < 1:
            raise ValueError(f"iterative_demapping must be an integer >= 1, got {iterative_demapping!r}")
        self.iterative_demapping = int(iterative_demapping)
        if isinstance(demapping_feedback_scale, (bool, str)) or not np.isscalar(demapping_feedback_scale) \
                or not np.isreal(demapping_feedback_scale) or not np.isfinite(demapping_feedback_scale):
            raise ValueError(f"demapping_feedback_scale must be a finite number, got {demapping_feedback_scale!r}")
        self.demapping_feedback_scale = float(demapping_feedback_scale)
        if self.iterative_demapping > 1:
            if self.channel != "device" or not isinstance(self.modulation, Constellation):
                raise ValueError("iterative_demapping > 1 needs channel='device' and a modulation.Constellation "
                                 "(Constellation.from_modulation gives a named scheme's table)")
            if self.diagnostics or int(self.capture_errors) > 0:
                raise ValueError("iterative_demapping > 1 together with diagnostics or capture_errors is not provided: the "
                                 "stop-iteration histogram has T + 1 bins and the iterations summed over the rounds do not "
                                 "fit it (DESIGN.md section 3n)")
        if self.modulation is not None:
            if not isinstance(self.modulation, Modulation):
                raise ValueError("modulation must be a modulation.Modulation")
            if self.channel != "device":
                raise ValueError("modulation needs channel='device'")
            if self.rate_matching is not None:
                raise ValueError("rate_matching together with modulation is not provided (DESIGN.md section 3j)")
            if self.llr_convention != "decoder":
                raise ValueError("modulation maps bit 0 to the positive half: llr_convention must be 'decoder'")
            if isinstance(self.modulation, Constellation) and self.codeword is None:
                raise ValueError(f"{self.modulation.scheme}: a constellation table has no guaranteed symmetry, so the all-zero "
                                 f"codeword says nothing about the others: set codeword=\"random\" (or give a codeword)")
            if self.modulation.bits_per_symbol >= 4 and self.codeword is None:
                raise ValueError(f"{self.modulation.scheme} with the all-zero codeword sends one corner point only and its bit "
                                 f"channels are not output-symmetric: set codeword=\"random\" (or give a codeword)")
        if self.rate_matching is not None:
            if not isinstance(self.rate_matching, RateMatching):
                raise ValueError("rate_matching must be a rate_matching.RateMatching")
            if self.channel != "device":
                raise ValueError("rate_matching needs channel='device'")
        if self.channel not in ("torch", "device"):
            raise ValueError(f"channel must be 'torch' or 'device', got {self.channel!r}")
        if isinstance(self.codeword, str) and self.codeword != "random":
            raise ValueError(f"codeword must be None, a 0/1 array or 'random', got {self.codeword!r}")
        if self.codeword is not None and self.channel != "device":
            raise ValueError("a codeword other than all-zero needs channel='device'")
        if int(self.capture_errors) < 0:
            raise ValueError("capture_errors must be >= 0")
        if (self.diagnostics or int(self.capture_errors) > 0) and self.channel != "device":
            raise ValueError("diagnostics and capture_errors need channel='device'")


class SimulationResult:
    """Container for simulation results (same attributes as the reference's)"""

    def __init__(self, decoder_name: str, snr_values: List[float]):
        self.decoder_name = decoder_name
        self.snr_values = snr_values
        self.frame_error_rates: List[float] = []
        self.bit_error_rates: List[float] = []
        self.average_iterations: List[float] = []
        self.simulation_times: List[float] = []
        self.total_frames: List[int] = []
        self.total_errors: List[int] = []
        # per SNR point, filled only by a run with diagnostics: undetected frame errors, frames per stop iteration (T + 1
        # bins), the recorded frame errors (engine.ERROR_FRAME_DTYPE: frame, wrong_bits, iterations, undetected)
        self.undetected_errors: List[int] = []
        self.iteration_histograms: List[List[int]] = []
        self.error_frames: List[np.ndarray] = []

    def add_diagnostics(self, snr_idx: int, undetected_errors: int, iteration_histogram, error_frames):
        import engine as _engine
        while len(self.undetected_errors) <= snr_idx:
            self.undetected_errors.append(0)
            self.iteration_histograms.append([])
            self.error_frames.append(np.empty(0, dtype=_engine.ERROR_FRAME_DTYPE))
        self.undetected_errors[snr_idx] = int(undetected_errors)
        self.iteration_histograms[snr_idx] = [int(v) for v in iteration_histogram]
        self.error_frames[snr_idx] = np.asarray(error_frames, dtype=_engine.ERROR_FRAME_DTYPE)

    def add_result(self, snr_idx: int, fer: float, ber: float, avg_iter: float, sim_time: float,
                   total_frames: int, total_errors: int):
        for lst, zero in ((self.frame_error_rates, 0.0), (self.bit_error_rates, 0.0), (self.average_iterations, 0.0),
                          (self.simulation_times, 0.0), (self.total_frames, 0), (self.total_errors, 0)):
            while len(lst) <= snr_idx:
                lst.append(zero)
        self.frame_error_rates[snr_idx] = fer
        self.bit_error_rates[snr_idx] = ber
        self.average_iterations[snr_idx] = avg_iter
        self.simulation_times[snr_idx] = sim_time
        self.total_frames[snr_idx] = total_frames
        self.total_errors[snr_idx] = total_errors


def frames_to_count(frame_error: np.ndarray, frames_so_far: int, errors_so_far: int,
                    max_frames: int, max_errors: int) -> int:
    """How many frames of a block the reference's loop ``while total_frames < max_frames and
    frame_errors < max_errors`` (simulation_framework.py:110) would still have simulated: frames are
    consumed in order and the loop stops right after the frame that reaches either limit."""
    room = max(0, max_frames - frames_so_far)
    take = min(len(frame_error), room)
    need = max_errors - errors_so_far
    if need <= 0:
        return 0
    cum = np.cumsum(frame_error[:take].astype(np.int64))
    hit = np.nonzero(cum >= need)[0]
    if hit.size:
        take = int(hit[0]) + 1
    return take


def _engine_of(decoder, device):
    """the batched engine behind a host decoder object (fp32)"""
    if isinstance(decoder, BasicMinSumDecoder):
        return decoder._engine(torch.float32, device)
    if hasattr(decoder, "_get_engine"):
        return decoder._get_engine(device)
    raise TypeError(f"{type(decoder).__name__} is not one of this package's decoders")


def _decode_block(eng, llr: torch.Tensor, cap):
    """Early-stop decode of one block -> (bits, iterations), exactly what eng.decode(llr, early_stop=True) returns.
    The streaming engine freezes whole 256-codeword tiles only, so a block whose codewords stop after 6 iterations on average
    but has a straggler in every tile costs all T iterations.  With `cap` (chosen by _next_cap from the previous block) the
    block runs in two stages: every codeword up to `cap` iterations (ldpc_decode_capped: the decoder's own per-iteration tables),
    then the few still open ones again from their LLRs as a small batch with the full iteration count.  A codeword's decode does
    not depend on its neighbours in the batch, and a codeword that stops within the cap stops at the same iteration with the
    same decisions either way: the result is identical to the one-stage decode.
    The decisions come back bit-packed (uint8 [B, ceil(n/8)], the multi-GPU wire format): the driver only counts them, and the
    engine then stores neither int32 decision rows nor posterior rows."""
    kw = dict(early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
    if cap is None:
        res = eng.decode(llr, **kw)
        return res.packed_bits, res.iterations
    res = eng.decode(llr, max_iters=int(cap), **kw)
    packed, iters = res.packed_bits, res.iterations
    open_idx = torch.nonzero(~res.success, as_tuple=False).reshape(-1)
    if open_idx.numel():
        rest = eng.decode(llr.index_select(0, open_idx).contiguous(), **kw)
        packed.index_copy_(0, open_idx, rest.packed_bits)
        iters.index_copy_(0, open_idx, rest.iterations)
    return packed, iters


def _decode_block_flags(eng, llr: torch.Tensor, cap):
    """_decode_block that also returns the success flags (bool [B]) -> (packed, iterations, success): a codeword still open at
    the cap takes all three from its full decode"""
    kw = dict(early_stop=True, want_bits=False, want_posterior=False, want_packed=True)
    res = eng.decode(llr, **kw) if cap is None else eng.decode(llr, max_iters=int(cap), **kw)
    packed, iters, success = res.packed_bits, res.iterations, res.success
    if cap is not None:
        open_idx = torch.nonzero(~success, as_tuple=False).reshape(-1)
        if open_idx.numel():
            rest = eng.decode(llr.index_select(0, open_idx).contiguous(), **kw)
            packed.index_copy_(0, open_idx, rest.packed_bits)
            iters.index_copy_(0, open_idx, rest.iterations)
            success.index_copy_(0, open_idx, rest.success)
    return packed, iters, success


_POPCOUNT = {}


def _ones_per_frame(packed: torch.Tensor, n: int) -> torch.Tensor:
    """number of set decision bits of every frame (int64 [B]) from the bit-packed rows"""
    lut = _POPCOUNT.get(packed.device)
    if lut is None:
        lut = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.int16, device=packed.device)
        _POPCOUNT[packed.device] = lut
    if n % 8:                                       # bits past n in the last byte do not belong to the codeword
        packed = packed.clone()
        packed[:, -1] &= (1 << (n % 8)) - 1
    return lut[packed.to(torch.int64)].sum(dim=1, dtype=torch.int64)


def _next_cap(eng, iters: torch.Tensor, min_block: int = 1024):
    """Iteration cap for the next block from this block's stop iterations: the cap c minimising c + open(c) * (T + 2), the cost
    in full-block iterations of stage one plus the restart of the codewords still open after c (open(c) = share with more than c
    iterations; one that never converges counts as open for every c < T).  None when the engine stops codeword by codeword
    anyway (LDS-resident) or when staging would not save a quarter of the block's work."""
    info = eng.info()
    T = int(eng.iters)
    if info["engine"] != "stream" or T < 4 or iters.numel() < min_block:
        return None
    hist = torch.bincount(iters.to(torch.int64).clamp_(0, T), minlength=T + 1).to(torch.float64)
    open_after = 1.0 - torch.cumsum(hist, 0) / float(iters.numel())            # open_after[c] = share with iterations > c
    c = torch.arange(T + 1, dtype=torch.float64, device=open_after.device)
    cost = c + open_after * (T + 2.0)
    cost[0] = float("inf")
    best = int(torch.argmin(cost[:T]).item()) if T > 1 else T
    return best if float(cost[best]) <= 0.75 * T else None


class LDPSimulator:
    """LDPC decoder simulator on the batched GPU engine"""

    def __init__(self, config: SimulationConfig):
        self.config = config
        self.results: Dict[str, SimulationResult] = {}
        self._last = threading.local()          # diagnostics of the calling thread's last point (simulate_decoder collects them)
        self._warned_punctured_zero = False     # the all-zero-codeword warning is issued once per simulator
        if config.save_results:
            os.makedirs(config.results_dir, exist_ok=True)

    # ------------------------------------------------------------------------------ one SNR point
    def _draw_llr(self, gen: torch.Generator, frames: int, n: int, snr_db: float, device) -> torch.Tensor:
        snr_linear = 10 ** (snr_db / 10)
        noise_power = 1 / snr_linear
        z = torch.randn((frames, n), generator=gen, device=device, dtype=torch.float32)
        symbol = 1.0 if self.config.llr_convention == "decoder" else -1.0      # all-zero codeword
        # llr = 2 * (symbol + sigma * z) / sigma^2 (simulation_framework.py:95-103 of the reference), as ONE scale-and-shift in
        # place: two passes over the block instead of four element-wise kernels with a temporary each
        return z.mul_(2.0 * (noise_power ** 0.5) / noise_power).add_(2.0 * symbol / noise_power)

    def simulate_single_snr(self, decoder: Callable, code: LDPCCode, snr_db: float, max_frames: int,
                            max_errors: int) -> Tuple[float, float, float, float, int, int]:
        """-> fer, ber, avg_iterations, simulation_time, total_frames, total_errors (frame errors)"""
        start_time = time.time()
        from engine import _require_gpu
        device = _require_gpu(self.config.device)
        eng = _engine_of(decoder, device)
        self._last.diagnostics = None
        if self.config.channel == "device":
            rm = self.config.rate_matching
            if rm is not None and rm.n != code.n:
                raise ValueError(f"rate_matching is a profile of n = {rm.n}, the code has n = {code.n}")
            if rm is not None and rm.n_punctured and self.config.codeword is None and not self._warned_punctured_zero:
                self._warned_punctured_zero = True
                warnings.warn("punctured bits with the all-zero codeword: a punctured bit that is never recovered keeps posterior "
                              "0, decides 0 and counts as correct -- send random codewords (SimulationConfig.codeword = 'random') or a "
                              "nonzero one (e.g. codes.staircase_encode)", UserWarning, stacklevel=2)
            c = self._simulate_device(eng, code.n, float(snr_db), int(max_frames), int(max_errors))
            if "iteration_histogram" in c:
                self._last.diagnostics = c
            frames = c["frames"]
            counted = code.n if rm is None else rm.n_counted
            return (c["frame_errors"] / frames if frames > 0 else 0.0,
                    c["bit_errors"] / (frames * counted) if frames > 0 and counted > 0 else 0.0,
                    c["iterations"] / frames if frames > 0 else 0.0, time.time() - start_time, frames, c["frame_errors"])
        gen = torch.Generator(device=device)
        gen.manual_seed(int(self.config.seed) * 1_000_003 + int(round(snr_db * 1000)))
        frame_errors = bit_errors = total_iterations = total_frames = 0
        block = max(1, int(self.config.batch_frames))
        cap = None                                                              # iteration cap of the next block's first stage
        while total_frames < max_frames and frame_errors < max_errors:
            frames = min(block, max_frames - total_frames)
            llr = self._draw_llr(gen, frames, code.n, float(snr_db), device)
            packed, iters = _decode_block(eng, llr, cap)
            cap = _next_cap(eng, iters, int(self.config.stage_min_block)) if self.config.staged_early_stop else None
            wrong = _ones_per_frame(packed, code.n)                             # all-zero codeword was sent: every 1 is an error
            ferr = wrong > 0
            take = frames_to_count(ferr.cpu().numpy(), total_frames, frame_errors, max_frames, max_errors)
            frame_errors += int(ferr[:take].sum().item())
            bit_errors += int(wrong[:take].sum().item())
            total_iterations += int(iters[:take].sum().item())
            total_frames += take
        fer = frame_errors / total_frames if total_frames > 0 else 0.0
        ber = bit_errors / (total_frames * code.n) if total_frames > 0 else 0.0
        avg_iterations = total_iterations / total_frames if total_frames > 0 else 0.0
        return fer, ber, avg_iterations, time.time() - start_time, total_frames, frame_errors

    def _simulate_device(self, eng, n: int, snr_db: float, max_frames: int, max_errors: int) -> dict:
        """channel="device": the counters {frames, frame_errors, bit_errors, iterations, ...} of one SNR point.  The
        LDS-resident engine stops codeword by codeword, so the whole point runs in one native call; on the streaming engine
        the loop stays here so that _decode_block's staged early stop still applies -- the same stream, the same counters.
        With cfg.diagnostics / capture_errors the dict also has the keys DecodeEngine.simulate(diagnostics=True) adds."""
        import engine as _engine
        cfg = self.config
        capture = int(cfg.capture_errors)
        diagnostics = bool(cfg.diagnostics) or capture > 0
        scale, shift = _engine.awgn_scale_shift(snr_db, cfg.llr_convention)
        stream_id = int(round(snr_db * 1000)) % (1 << 32)
        block = max(1, int(cfg.batch_frames))
        random = isinstance(cfg.codeword, str)            # "random": a fresh codeword per frame
        cw = "random" if random else None if cfg.codeword is None else _engine.pack_codeword(cfg.codeword, n, eng.device)
        rm = cfg.rate_matching
        mod = cfg.modulation

        def draw(frames, first, cw):                       # the block's LLRs: the symbol channel under a modulation
            if mod is not None:
                return _engine.sym_llr(frames, n, seed=int(cfg.seed), stream_id=stream_id, first_frame=first, modulation=mod,
                                       snr_db=snr_db, codeword=cw, device=eng.device)
            return _engine.awgn_llr(frames, n, seed=int(cfg.seed), stream_id=stream_id, first_frame=first, scale=scale,
                                    shift=shift, codeword=cw, device=eng.device, rate_matching=rm)

        if cfg.iterative_demapping > 1:
            # iterative demapping: the Python block loop on every engine -- the samples of the same stream, rounds of
            # demap and decode on them, the same counters fed with the iterations summed over the rounds
            state = torch.zeros(8, dtype=torch.int64, device=eng.device)
            drawn, host = 0, [0] * 8
            while drawn < max_frames and not host[4]:
                frames = min(block, max_frames - drawn)
                if random:
                    cw = _engine.encode_random(eng.encoder(), frames, seed=int(cfg.seed), stream_id=stream_id,
                                               first_frame=drawn, device=eng.device)
                llr, rec = _engine.sym_llr(frames, n, seed=int(cfg.seed), stream_id=stream_id, first_frame=drawn, modulation=mod,
                                         snr_db=snr_db, codeword=cw, device=eng.device, want_received=True)
                res = eng.decode_iterative(rec, modulation=mod, rounds=cfg.iterative_demapping,
                                           prior_scale=cfg.demapping_feedback_scale, early_stop=True, want_bits=False,
                                           want_posterior=False, want_packed=True, llr=llr)
                eng.sim_count(state, res.packed_bits, res.iterations, max_frames=max_frames, max_errors=max_errors,
                              codeword=cw)
                host = state.tolist()
                drawn += frames
            return dict(zip(_engine.SIM_COUNTERS, host))
        if eng.info()["engine"] == "resident":
            if mod is not None:
                return eng.simulate(seed=int(cfg.seed), stream_id=stream_id, snr_db=snr_db, modulation=mod, codeword=cw,
                                    max_frames=max_frames, max_errors=max_errors, block=block,
                                    poll_blocks=max(1, int(cfg.poll_blocks)), diagnostics=diagnostics, capture=capture)
            return eng.simulate(seed=int(cfg.seed), stream_id=stream_id, scale=scale, shift=shift, codeword=cw,
                                max_frames=max_frames, max_errors=max_errors, block=block,
                                poll_blocks=max(1, int(cfg.poll_blocks)), diagnostics=diagnostics, capture=capture,
                                rate_matching=rm)
        state = torch.zeros(8, dtype=torch.int64, device=eng.device)
        diag = eng.sim_diag_buffer(capture) if diagnostics else None
        drawn, cap, host = 0, None, [0] * 8
        while drawn < max_frames and not host[4]:
            frames = min(block, max_frames - drawn)
            if random:                                                          # the block's codeword rows
                cw = _engine.encode_random(eng.encoder(), frames, seed=int(cfg.seed), stream_id=stream_id, first_frame=drawn,
                                           device=eng.device)
            llr = draw(frames, drawn, cw)
            if diagnostics:
                packed, iters, success = _decode_block_flags(eng, llr, cap)
                eng.sim_count(state, packed, iters, max_frames=max_frames, max_errors=max_errors, codeword=cw,
                              success=success, diag=diag, first_frame=drawn, capture=capture, rate_matching=rm)
            else:
                packed, iters = _decode_block(eng, llr, cap)
                eng.sim_count(state, packed, iters, max_frames=max_frames, max_errors=max_errors, codeword=cw,
                              rate_matching=rm)
            cap = _next_cap(eng, iters, int(cfg.stage_min_block)) if cfg.staged_early_stop else None
            host = state.tolist()                                               # the one read of the block
            drawn += frames
        res = dict(zip(_engine.SIM_COUNTERS, host))
        if diagnostics:
            res.update(_engine.parse_sim_diag(diag.cpu().numpy(), int(eng.iters), capture))
            res["detected_errors"] = res["frame_errors"] - res["undetected_errors"]
        return res

    def replay_errors(self, decoder, code: LDPCCode, snr_db: float, frames) -> dict:
        """Draw the listed frames of the point at `snr_db` again -- stream indices, e.g. error_frames["frame"] of a run with
        this configuration (same seed, convention, codeword and rate_matching; channel="device") -- and decode them with early stop.
        -> {frames, llr [F, n], bits int32 [F, n], posterior [F, n], iterations int32 [F], success bool [F]} on the device.
        Under iterative_demapping > 1 the frames go through the same rounds (DecodeEngine.decode_iterative): llr is round 1's,
        iterations the sum over the rounds, and the dict also has `rounds` int32 [F] and `received` [F, S, 4], the samples.
        A frame has the same noise whatever block it was drawn in, so this reproduces the recorded failure exactly.  Under
        codeword="random" each frame's codeword is drawn again too and the dict has `codewords`: uint8 [F, ceil(n/8)], packed."""
        import engine as _engine
        cfg = self.config
        if cfg.channel != "device":
            raise ValueError("replay_errors needs channel='device': only the counter-based stream can draw a frame again")
        eng = _engine_of(decoder, _engine._require_gpu(cfg.device))
        scale, shift = _engine.awgn_scale_shift(float(snr_db), cfg.llr_convention)
        stream_id = int(round(float(snr_db) * 1000)) % (1 << 32)
        random = isinstance(cfg.codeword, str)
        cw = None if random or cfg.codeword is None else _engine.pack_codeword(cfg.codeword, code.n, eng.device)
        frames = [int(f) for f in np.asarray(frames).reshape(-1)]
        words = [_engine.encode_random(eng.encoder(), 1, seed=int(cfg.seed), stream_id=stream_id, first_frame=f,
                                       device=eng.device) for f in frames] if random else [cw] * len(frames)
        if cfg.iterative_demapping > 1:                    # the samples again, and the rounds on them
            pairs = [_engine.sym_llr(1, code.n, seed=int(cfg.seed), stream_id=stream_id, first_frame=f, modulation=cfg.modulation,
                                     snr_db=float(snr_db), codeword=c, device=eng.device, want_received=True)
                     for f, c in zip(frames, words)]
            S = cfg.modulation.symbols(code.n)
            llr = (torch.cat([p[0] for p in pairs], dim=0) if pairs else
                   torch.empty((0, code.n), dtype=torch.float32, device=eng.device))
            rec = (torch.cat([p[1] for p in pairs], dim=0) if pairs else
                   torch.empty((0, S, 4), dtype=torch.float32, device=eng.device))
            with torch.no_grad():
                res = eng.decode_iterative(rec, modulation=cfg.modulation, rounds=cfg.iterative_demapping,
                                           prior_scale=cfg.demapping_feedback_scale, early_stop=True, llr=llr)
            out = {"frames": frames, "llr": llr, "bits": res.bits, "posterior": res.posterior, "iterations": res.iterations,
                   "success": res.success, "rounds": res.rounds, "received": rec}
            if random:
                out["codewords"] = (torch.cat(words, dim=0) if words else
                                    torch.empty((0, (code.n + 7) // 8), dtype=torch.uint8, device=eng.device))
            return out
        if cfg.modulation is not None:                     # the symbol channel draws a frame again just the same
            rows = [_engine.sym_llr(1, code.n, seed=int(cfg.seed), stream_id=stream_id, first_frame=f, modulation=cfg.modulation,
                                    snr_db=float(snr_db), codeword=c, device=eng.device) for f, c in zip(frames, words)]
        else:
            rows = [_engine.awgn_llr(1, code.n, seed=int(cfg.seed), stream_id=stream_id, first_frame=f, scale=scale, shift=shift,
                                     codeword=c, device=eng.device, rate_matching=cfg.rate_matching)
                    for f, c in zip(frames, words)]
        llr = torch.cat(rows, dim=0) if rows else torch.empty((0, code.n), dtype=torch.float32, device=eng.device)
        with torch.no_grad():
            res = eng.decode(llr, early_stop=True)
        out = {"frames": frames, "llr": llr, "bits": res.bits, "posterior": res.posterior, "iterations": res.iterations,
               "success": res.success}
        if random:
            out["codewords"] = (torch.cat(words, dim=0) if words else
                                torch.empty((0, (code.n + 7) // 8), dtype=torch.uint8, device=eng.device))
        return out

    # ------------------------------------------------------------------------------ sweeps
    def simulate_decoder(self, decoder: Union[Callable, torch.nn.Module], code: LDPCCode,
                         decoder_name: str) -> SimulationResult:
        logger.info(f"Starting simulation for {decoder_name}")
        snr_values = np.arange(self.config.snr_range[0], self.config.snr_range[1] + self.config.snr_step,
                               self.config.snr_step)
        result = SimulationResult(decoder_name, snr_values.tolist())
        for snr_idx, snr_db in enumerate(snr_values):
            fer, ber, avg_iter, sim_time, total_frames, total_errors = self.simulate_single_snr(
                decoder, code, snr_db, self.config.max_frames, self.config.max_errors)
            result.add_result(snr_idx, fer, ber, avg_iter, sim_time, total_frames, total_errors)
            d = getattr(self._last, "diagnostics", None)
            if d is not None:
                result.add_diagnostics(snr_idx, d["undetected_errors"], d["iteration_histogram"], d["error_frames"])
            logger.info(f"SNR {snr_db:.1f}dB: FER={fer:.2e}, BER={ber:.2e}, Avg Iter={avg_iter:.1f}, Time={sim_time:.1f}s")
        self.results[decoder_name] = result
        return result

    def simulate_multiple_decoders(self, decoders: Dict[str, Union[Callable, torch.nn.Module]],
                                   code: LDPCCode) -> Dict[str, SimulationResult]:
        """one worker thread per decoder, as the reference does (each decoder owns its engine and
        workspace; the GPU serialises the kernels)"""
        logger.info(f"Starting simulation for {len(decoders)} decoders")
        results: Dict[str, SimulationResult] = {}
        if self.config.parallel_workers > 1:
            with ThreadPoolExecutor(max_workers=self.config.parallel_workers) as executor:
                futures = {executor.submit(self.simulate_decoder, dec, code, name): name for name, dec in decoders.items()}
                for future in as_completed(futures):
                    name = futures[future]
                    try:
                        results[name] = future.result()
                        logger.info(f"Completed simulation for {name}")
                    except Exception as e:            # the reference logs and carries on (simulation_framework.py:203-208)
                        logger.error(f"Error simulating {name}: {e}")
        else:
            for name, dec in decoders.items():
                results[name] = self.simulate_decoder(dec, code, name)
        if self.config.save_results:
            self.save_results(results, "simulation_results.json")
        return results

    # ------------------------------------------------------------------------------ persistence
    def save_results(self, results: Dict[str, SimulationResult], filename: str):
        serializable = {name: {"decoder_name": r.decoder_name, "snr_values": r.snr_values,
                               "frame_error_rates": r.frame_error_rates, "bit_error_rates": r.bit_error_rates,
                               "average_iterations": r.average_iterations, "simulation_times": r.simulation_times,
                               "total_frames": r.total_frames, "total_errors": r.total_errors}
                        for name, r in results.items()}
        for name, r in results.items():                  # diagnostics: only where a run filled them
            if getattr(r, "iteration_histograms", None):
                serializable[name]["undetected_errors"] = [int(v) for v in r.undetected_errors]
                serializable[name]["iteration_histograms"] = [[int(v) for v in h] for h in r.iteration_histograms]
                serializable[name]["error_frames"] = [[[int(v) for v in rec] for rec in np.asarray(e).tolist()]
                                                      for e in r.error_frames]
        os.makedirs(self.config.results_dir, exist_ok=True)
        filepath = f"{self.config.results_dir}/{filename}"
        with open(filepath, "w") as f:
            json.dump(serializable, f, indent=2)
        logger.info(f"Results saved to {filepath}")

    def load_results(self, filename: str) -> Dict[str, SimulationResult]:
        filepath = f"{self.config.results_dir}/{filename}"
        with open(filepath, "r") as f:
            data = json.load(f)
        results = {}
        for name, d in data.items():
            r = SimulationResult(d["decoder_name"], d["snr_values"])
            r.frame_error_rates = d["frame_error_rates"]
            r.bit_error_rates = d["bit_error_rates"]
            r.average_iterations = d["average_iterations"]
            r.simulation_times = d["simulation_times"]
            r.total_frames = d["total_frames"]
            r.total_errors = d["total_errors"]
            if "iteration_histograms" in d:
                import engine as _engine
                r.undetected_errors = d["undetected_errors"]
                r.iteration_histograms = d["iteration_histograms"]
                r.error_frames = [np.array([tuple(rec) for rec in e], dtype=_engine.ERROR_FRAME_DTYPE) for e in d["error_frames"]]
            results[name] = r
        logger.info(f"Results loaded from {filepath}")
        return results


def create_test_decoders(code: LDPCCode) -> Dict[str, Union[Callable, torch.nn.Module]]:
    """the reference's comparison set (simulation_framework.py:384-420)"""
    decoders: Dict[str, Union[Callable, torch.nn.Module]] = {}
    decoders["Basic MinSum"] = BasicMinSumDecoder(code, factor=0.7)
    decoders["N-NMS"] = NeuralMinSumDecoder(code, max_iterations=10)
    decoders["N-OMS"] = NeuralOffsetMinSumDecoder(code, max_iterations=10)
    for weight_type in [1, 2, 3, 4]:
        decoders[f"N-2D-NMS Type {weight_type}"] = Neural2DMinSumDecoder(code, weight_sharing_type=weight_type,
                                                                         max_iterations=10)
    decoders["N-2D-OMS Type 2"] = Neural2DOffsetMinSumDecoder(code, weight_sharing_type=2, max_iterations=10)
    quantizer_params = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]
    decoders["RCQ MinSum"] = RCQMinSumDecoder(code, bc=3, bv=8, quantizer_params=quantizer_params, max_iterations=10)
    decoders["W-RCQ Type 2"] = WeightedRCQDecoder(code, bc=3, bv=8, quantizer_params=quantizer_params,
                                                  weight_sharing_type=2, max_iterations=10)
    return decoders
