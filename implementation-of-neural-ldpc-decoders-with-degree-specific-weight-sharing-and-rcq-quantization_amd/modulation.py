"""
Symbol modulation for the on-device Monte-Carlo path: Gray-mapped BPSK / QPSK / 16- / 64- / 256-QAM of unit average energy over
AWGN or per-symbol Rayleigh fading, demapped with the max-log rule or the exact log-MAP rule (ldpc_channel_sym /
ldpc_channel_sym_dm of include/ldpc_hip.h; the definition is in INTEGRATION.md 6f, 6h and DESIGN.md 3j, 3l).  ``Modulation`` is the host-side description; ``engine.sym_llr``,
``DecodeEngine.simulate(modulation=...)`` and ``SimulationConfig(channel="device", modulation=...)`` take it, and so do the
training draw ``engine.sym_llr_mix`` and ``PosteriorJointTrainer(modulation=...)`` (ldpc_channel_sym_mix).
``engine.demap`` turns received samples into LLRs (ldpc_demap_sym); ``Modulation.normalise_received`` brings physical
samples into its layout.
"""

from __future__ import annotations

import math
import threading
from typing import Optional

import numpy as np

SCHEMES = {"bpsk": 1, "qpsk": 2, "qam16": 4, "qam64": 6, "qam256": 8}
FADINGS = {None: 0, "rayleigh": 1}
DEMAPPERS = {"maxlog": 0, "exact": 1}     # LDPC_DEMAP_MAXLOG, LDPC_DEMAP_EXACT
MAX_SYMBOLS = 1 << 29      # the symbol index shares a Philox counter word with a two-bit stream tag


def axis_bits(bits_per_symbol: int) -> int:
    """h: label bits per axis (BPSK has one axis of one bit)"""
    return 1 if bits_per_symbol == 1 else bits_per_symbol // 2


def half_spacing(bits_per_symbol: int) -> float:
    """d: half the distance between neighbouring points of the unit-energy constellation"""
    if bits_per_symbol == 1:
        return 1.0
    return math.sqrt(3.0 / (2.0 * (4.0 ** axis_bits(bits_per_symbol) - 1.0)))


class Modulation:
    """``Modulation(scheme, fading=None, interleaver=None, demapper="maxlog")``: scheme "bpsk" | "qpsk" | "qam16" | "qam64" |
    "qam256", fading None | "rayleigh" (independent per symbol, known to the receiver), interleaver an integer permutation
    ``pos`` of 0 .. n-1: transmit index t = s * m + k (bit k of symbol s) carries the codeword bit of variable pos[t]; None is
    the identity.  demapper "maxlog" | "exact": the rule that turns a received sample into LLRs -- the max-log rule, or the
    exact log-MAP rule (max-log plus the log-sum-exp correction; the same thing for BPSK and QPSK).  Callers read
    ``modulation.demapper``."""

    def __init__(self, scheme: str, fading: Optional[str] = None, interleaver=None, demapper: str = "maxlog"):
        if not isinstance(scheme, str) or scheme not in SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(SCHEMES)}, got {scheme!r} (PSK above 4 points and APSK are not "
                             f"provided)")
        if fading not in FADINGS:
            raise ValueError(f"fading must be None or 'rayleigh', got {fading!r} (block fading is not provided)")
        if not isinstance(demapper, str) or demapper not in DEMAPPERS:
            raise ValueError(f"demapper must be 'maxlog' or 'exact', got {demapper!r}")
        self.scheme = scheme
        self.fading = fading
        self.demapper = demapper
        self.bits_per_symbol = SCHEMES[scheme]
        self.interleaver = None
        if interleaver is not None:
            pos = np.asarray(interleaver)
            if pos.ndim != 1 or pos.size < 1 or not np.issubdtype(pos.dtype, np.integer):
                raise ValueError("interleaver must be a 1-D integer array")
            if not np.array_equal(np.sort(pos.astype(np.int64)), np.arange(pos.size)):
                raise ValueError(f"interleaver must be a permutation of 0 .. {pos.size - 1}")
            self.interleaver = np.ascontiguousarray(pos.astype(np.int32))
        self._device = {}
        self._lock = threading.Lock()

    def __repr__(self):
        return (f"Modulation({self.scheme!r}, fading={self.fading!r}, interleaver="
                f"{None if self.interleaver is None else f'<permutation of {self.interleaver.size}>'}"
                f"{'' if self.demapper == 'maxlog' else f', demapper={self.demapper!r}'})")

    def amp(self, snr_db: float) -> float:
        """the constellation's half-spacing over the per-dimension noise standard deviation at Es/N0 = snr_db, in double:
        1 / sqrt(N0) for BPSK (real noise of variance N0), d / sqrt(N0 / 2) for the complex schemes"""
        n0 = 10.0 ** (-float(snr_db) / 10.0)
        if self.bits_per_symbol == 1:
            return 1.0 / math.sqrt(n0)
        return half_spacing(self.bits_per_symbol) / math.sqrt(n0 / 2.0)

    def amp_table(self, snr_db) -> np.ndarray:
        """float32 [K]: ``amp`` of each of the K points of snr_db (Es/N0), computed in double and then cast -- entry p is exactly
        the value ``engine.sym_llr(snr_db=snr_db[p])`` hands the kernel; the table of ``engine.sym_llr_mix``"""
        snr = np.asarray(snr_db, dtype=np.float64)
        if snr.ndim != 1:
            raise ValueError("snr_db must be a 1-D sequence of SNR points")
        return np.array([self.amp(float(s)) for s in snr], dtype=np.float64).astype(np.float32)

    def symbols(self, n: int) -> int:
        """S = ceil(n / m): symbols of a frame of n bits"""
        return (int(n) + self.bits_per_symbol - 1) // self.bits_per_symbol

    def check(self, n: int):
        n = int(n)
        if self.interleaver is not None and self.interleaver.size != n:
            raise ValueError(f"the interleaver permutes {self.interleaver.size} positions, the frame has n = {n}")
        if self.symbols(n) >= MAX_SYMBOLS:
            raise NotImplementedError(f"a frame of {self.symbols(n)} symbols: the symbol index must stay below 2^29")

    def native(self, amp: float, n: int, device):
        """the ldpc_modulation struct for a frame of n bits on `device` (the interleaver is uploaded once per device and kept);
        returned with the tensor it points into, which must outlive the call"""
        import torch
        import _native as nat
        self.check(n)
        amp = float(amp)
        if not (math.isfinite(amp) and amp >= 0.0):
            raise ValueError("amp must be finite and >= 0")
        pos = None
        if self.interleaver is not None:
            key = str(device)
            with self._lock:
                pos = self._device.get(key)
                if pos is None:
                    pos = self._device[key] = torch.from_numpy(self.interleaver).to(device)
        desc = nat.ModulationDesc()
        desc.bits_per_symbol, desc.fading, desc.amp = self.bits_per_symbol, FADINGS[self.fading], amp
        desc.position = None if pos is None else pos.data_ptr()
        return desc, pos

    def normalise_received(self, y, gain=None, *, snr_db: Optional[float] = None, noise_var: Optional[float] = None):
        """physical samples -> the float32 [B, S, 4] = (vI, vQ, e, 0) layout of ``engine.demap``: v in units of the
        per-dimension noise standard deviation, e the gain times the half-spacing in the same units.  y: complex [B, S]
        received samples y = h x + noise of unit-energy symbols x (a torch tensor or an array; the result is a torch tensor on
        y's device); gain: the channel coefficients h, complex or real [B, S] (None: 1).  Give exactly one of snr_db (Es/N0
        with Es = 1) and noise_var (N0).  With sigma = sqrt(N0 / 2) (BPSK: sqrt(N0), real noise) and y' = y conj(h) / |h|:
        (vI, vQ) = (Re y', Im y') / sigma (BPSK: vQ = 0), e = |h| d / sigma, d the half-spacing (BPSK: 1).  |h| = 0 gives e = 0,
        an erasure, and v = y / sigma.  Computed in double, then cast."""
        import torch
        if (snr_db is None) == (noise_var is None):
            raise ValueError("give exactly one of snr_db (Es/N0) and noise_var (N0)")
        n0 = 10.0 ** (-float(snr_db) / 10.0) if noise_var is None else float(noise_var)
        if not (math.isfinite(n0) and n0 > 0.0):
            raise ValueError("the noise variance N0 must be finite and > 0")
        y = torch.as_tensor(y)
        if y.dim() != 2:
            raise ValueError("y must be [B, S]: one received sample per symbol")
        y = y.to(torch.complex128)
        if gain is None:
            h = torch.ones_like(y)
        else:
            h = torch.as_tensor(gain).to(y.device)
            if tuple(h.shape) != tuple(y.shape):
                raise ValueError(f"gain must have y's shape {tuple(y.shape)}, got {tuple(h.shape)}")
            h = h.to(torch.complex128)
        bpsk = self.bits_per_symbol == 1
        sigma = math.sqrt(n0) if bpsk else math.sqrt(n0 / 2.0)
        mag = h.abs()
        live = mag > 0
        rot = torch.where(live, h.conj() / torch.where(live, mag, torch.ones_like(mag)), torch.ones_like(h))
        yr = y * rot
        out = torch.zeros(tuple(y.shape) + (4,), dtype=torch.float64, device=y.device)
        out[..., 0] = yr.real / sigma
        if not bpsk:
            out[..., 1] = yr.imag / sigma
        out[..., 2] = mag * (half_spacing(self.bits_per_symbol) / sigma)
        return out.to(torch.float32)
