"""
Symbol modulation for the on-device Monte-Carlo path: Gray-mapped BPSK / QPSK / 16- / 64- / 256-QAM of unit average energy over
AWGN or per-symbol Rayleigh fading, demapped with the max-log rule (ldpc_channel_sym of include/ldpc_hip.h; the definition is in
INTEGRATION.md 6f and DESIGN.md 3j).  ``Modulation`` is the host-side description; ``engine.sym_llr``,
``DecodeEngine.simulate(modulation=...)`` and ``SimulationConfig(channel="device", modulation=...)`` take it, and so do the
training draw ``engine.sym_llr_mix`` and ``PosteriorJointTrainer(modulation=...)`` (ldpc_channel_sym_mix).
"""

from __future__ import annotations

import math
import threading
from typing import Optional

import numpy as np

SCHEMES = {"bpsk": 1, "qpsk": 2, "qam16": 4, "qam64": 6, "qam256": 8}
FADINGS = {None: 0, "rayleigh": 1}
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
    """``Modulation(scheme, fading=None, interleaver=None)``: scheme "bpsk" | "qpsk" | "qam16" | "qam64" | "qam256", fading
    None | "rayleigh" (independent per symbol, known to the receiver), interleaver an integer permutation ``pos`` of 0 .. n-1:
    transmit index t = s * m + k (bit k of symbol s) carries the codeword bit of variable pos[t]; None is the identity."""

    def __init__(self, scheme: str, fading: Optional[str] = None, interleaver=None):
        if not isinstance(scheme, str) or scheme not in SCHEMES:
            raise ValueError(f"scheme must be one of {sorted(SCHEMES)}, got {scheme!r} (PSK above 4 points and APSK are not "
                             f"provided)")
        if fading not in FADINGS:
            raise ValueError(f"fading must be None or 'rayleigh', got {fading!r} (block fading is not provided)")
        self.scheme = scheme
        self.fading = fading
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
                f"{None if self.interleaver is None else f'<permutation of {self.interleaver.size}>'})")

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
