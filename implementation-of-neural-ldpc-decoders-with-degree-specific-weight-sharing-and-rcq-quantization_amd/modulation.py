"""
Symbol modulation for the on-device Monte-Carlo path: Gray-mapped BPSK / QPSK / 16- / 64- / 256-QAM of unit average energy over
AWGN or per-symbol Rayleigh fading, demapped with the max-log rule or the exact log-MAP rule (ldpc_channel_sym /
ldpc_channel_sym_dm of include/ldpc_hip.h; the definition is in INTEGRATION.md 6f, 6h and DESIGN.md 3j, 3l).  ``Modulation`` is the host-side description; ``engine.sym_llr``,
``DecodeEngine.simulate(modulation=...)`` and ``SimulationConfig(channel="device", modulation=...)`` take it, and so do the
training draw ``engine.sym_llr_mix`` and ``PosteriorJointTrainer(modulation=...)`` (ldpc_channel_sym_mix).
``engine.demap`` turns received samples into LLRs (ldpc_demap_sym); ``Modulation.normalise_received`` brings physical
samples into its layout.

``Constellation`` is a Modulation whose points are given as a table of up to 64 labelled points -- 8-PSK, APSK, any labelling,
rotated, shaped or learned sets -- demapped jointly over all points (ldpc_channel_con, ldpc_channel_con_mix, ldpc_demap_con,
ldpc_simulate_con).  Everything that takes a Modulation takes it.
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
            raise ValueError(f"scheme must be one of {sorted(SCHEMES)}, got {scheme!r} (PSK above 4 points, APSK and any other "
                             f"labelled point set: modulation.Constellation)")
        self.scheme = scheme
        self.bits_per_symbol = SCHEMES[scheme]
        self._init_channel(fading, interleaver, demapper)

    def _init_channel(self, fading, interleaver, demapper):
        if fading not in FADINGS:
            raise ValueError(f"fading must be None or 'rayleigh', got {fading!r} (block fading is not provided)")
        if not isinstance(demapper, str) or demapper not in DEMAPPERS:
            raise ValueError(f"demapper must be 'maxlog' or 'exact', got {demapper!r}")
        self.fading = fading
        self.demapper = demapper
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

    def _uploaded(self, what: str, host, device):
        """a host table on `device`: uploaded once per device and kept (None stays None)"""
        import torch
        if host is None:
            return None
        key = (what, str(device))
        with self._lock:
            dev = self._device.get(key)
            if dev is None:
                dev = self._device[key] = torch.from_numpy(host).to(device)
        return dev

    def native(self, amp: float, n: int, device):
        """the ldpc_modulation struct for a frame of n bits on `device` (the interleaver is uploaded once per device and kept);
        returned with the tensor it points into, which must outlive the call"""
        import _native as nat
        self.check(n)
        amp = float(amp)
        if not (math.isfinite(amp) and amp >= 0.0):
            raise ValueError("amp must be finite and >= 0")
        pos = self._uploaded("position", self.interleaver, device)
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


MAX_POINTS = 64            # ldpc_constellation: 1 .. 6 bits per symbol


class Constellation(Modulation):
    """``Constellation(points, fading=None, interleaver=None, demapper="maxlog", name=None)``: a constellation given as a table
    of M = 2, 4, ..., 64 labelled points in the plane, demapped jointly over all points (ldpc_channel_con of
    include/ldpc_hip.h).  points: complex [M], or real [M, 2] = (I, Q); entry l is the point
    that the symbol with label l = sum_k b_k 2^k sends (bit k of the symbol at bit k) -- the labelling is the order of the table.
    The points must be finite and not all zero; duplicates are the caller's choice.  The table is normalised to unit mean
    energy in double and then cast to float32: ``self.points`` (float32 [M, 2]) is what every path uses.  fading, interleaver
    and demapper as in ``Modulation``, of which this is a subclass: whatever takes a Modulation takes a Constellation.  A table
    has no guaranteed symmetry, so simulations and training on it need codeword="random" or an explicit codeword."""

    def __init__(self, points, fading: Optional[str] = None, interleaver=None, demapper: str = "maxlog",
                 name: Optional[str] = None):
        pts = np.asarray(points)
        if pts.dtype == object or not (np.issubdtype(pts.dtype, np.number) or pts.dtype == np.bool_):
            raise ValueError("points must be a numeric array: complex [M], or real [M, 2]")
        if np.iscomplexobj(pts):
            if pts.ndim != 1:
                raise ValueError(f"complex points must be 1-D [M], got shape {pts.shape}")
            xy = np.stack([pts.real, pts.imag], axis=-1).astype(np.float64)
        else:
            if pts.ndim != 2 or pts.shape[1] != 2:
                raise ValueError(f"real points must be [M, 2] = (I, Q), got shape {pts.shape}")
            xy = pts.astype(np.float64)
        count = xy.shape[0]
        if count < 2 or count > MAX_POINTS or count & (count - 1):
            raise ValueError(f"the number of points must be a power of two in 2 .. {MAX_POINTS}, got {count}")
        if not np.isfinite(xy).all():
            raise ValueError("points must be finite")
        energy = float((xy * xy).sum(axis=1).mean())
        if not energy > 0.0:
            raise ValueError("points must not all be zero")
        if name is not None and not isinstance(name, str):
            raise ValueError("name must be a string or None")
        self.scheme = name or "constellation"
        self.bits_per_symbol = count.bit_length() - 1
        self.points = np.ascontiguousarray((xy / math.sqrt(energy)).astype(np.float32))
        self._init_channel(fading, interleaver, demapper)

    def __repr__(self):
        return (f"Constellation(<{self.points.shape[0]} points>, fading={self.fading!r}, interleaver="
                f"{None if self.interleaver is None else f'<permutation of {self.interleaver.size}>'}"
                f"{'' if self.demapper == 'maxlog' else f', demapper={self.demapper!r}'}"
                f"{'' if self.scheme == 'constellation' else f', name={self.scheme!r}'})")

    @property
    def complex_points(self) -> np.ndarray:
        """complex128 [M]: the float32 table as complex numbers"""
        return self.points[:, 0].astype(np.float64) + 1j * self.points[:, 1].astype(np.float64)

    def amp(self, snr_db: float) -> float:
        """1 / sigma at Es/N0 = snr_db, sigma = sqrt(N0 / 2) the per-dimension noise standard deviation (complex noise for
        every m, m = 1 included): sqrt(2 * 10^(snr_db / 10)), in double"""
        return math.sqrt(2.0 * 10.0 ** (float(snr_db) / 10.0))

    def native(self, amp: float, n: int, device):
        """the ldpc_constellation struct for a frame of n bits on `device` (table and interleaver are uploaded once per device
        and kept); returned with the tensors it points into, which must outlive the call"""
        import _native as nat
        self.check(n)
        amp = float(amp)
        if not (math.isfinite(amp) and amp >= 0.0):
            raise ValueError("amp must be finite and >= 0")
        pos = self._uploaded("position", self.interleaver, device)
        tab = self._uploaded("points", self.points, device)
        desc = nat.ConstellationDesc()
        desc.bits_per_symbol, desc.fading, desc.amp = self.bits_per_symbol, FADINGS[self.fading], amp
        desc.position = None if pos is None else pos.data_ptr()
        desc.points = tab.data_ptr()
        return desc, (pos, tab)

    def normalise_received(self, y, gain=None, *, snr_db: Optional[float] = None, noise_var: Optional[float] = None):
        """physical samples -> the float32 [B, S, 4] = (vI, vQ, e, 0) layout of ``engine.demap``.  y: complex [B, S] samples
        y = h x + noise of points x of this (unit-energy) table; gain: h, complex or real [B, S] (None: 1).  Give exactly one
        of snr_db (Es/N0 with Es = 1) and noise_var (N0).  With sigma = sqrt(N0 / 2): (vI, vQ) = y conj(h) / |h| / sigma and
        e = |h| / sigma.  |h| = 0 gives e = 0, an erasure, and v = y / sigma.  Computed in double, then cast."""
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
        sigma = math.sqrt(n0 / 2.0)
        mag = h.abs()
        live = mag > 0
        rot = torch.where(live, h.conj() / torch.where(live, mag, torch.ones_like(mag)), torch.ones_like(h))
        yr = y * rot
        out = torch.zeros(tuple(y.shape) + (4,), dtype=torch.float64, device=y.device)
        out[..., 0] = yr.real / sigma
        out[..., 1] = yr.imag / sigma
        out[..., 2] = mag / sigma
        return out.to(torch.float32)

    # ------------------------------------------------------------------ factories
    @classmethod
    def psk(cls, M: int, phase: Optional[float] = None, **kwargs) -> "Constellation":
        """Gray-labelled M-PSK: position j = 0 .. M-1 at angle phase + 2 pi j / M carries label j ^ (j >> 1), so neighbouring
        points differ in one bit.  phase: the angle of position 0, default pi / M.  kwargs: fading, interleaver, demapper, name."""
        M = int(M)
        if M < 2 or M > MAX_POINTS or M & (M - 1):
            raise ValueError(f"M must be a power of two in 2 .. {MAX_POINTS}, got {M}")
        phi0 = math.pi / M if phase is None else float(phase)
        j = np.arange(M)
        pts = np.empty(M, dtype=np.complex128)
        pts[j ^ (j >> 1)] = np.exp(1j * (phi0 + 2.0 * math.pi * j / M))
        kwargs.setdefault("name", f"psk{M}")
        return cls(pts, **kwargs)

    @classmethod
    def apsk(cls, ring_sizes, radii, phases=None, labels=None, **kwargs) -> "Constellation":
        """APSK: rings from the inner to the outer one, ring r of ring_sizes[r] points at radius radii[r] (> 0, any common
        scale: the table is normalised), counter-clockwise from angle phases[r] (default pi / ring_sizes[r]) in steps of
        2 pi / ring_sizes[r].  The label of a point is its running index over the rings in that order, or labels[index] when
        `labels`, a permutation of 0 .. M-1, is given.  These are NOT the DVB-S2 bit maps (nor any other standard's): whoever
        wants a standard's labelling passes that standard's table to ``Constellation``.  kwargs as for ``psk``."""
        sizes = [int(v) for v in ring_sizes]
        rad = [float(v) for v in radii]
        if not sizes or any(v < 1 for v in sizes):
            raise ValueError("ring_sizes must be a non-empty sequence of positive integers")
        if len(rad) != len(sizes) or not all(math.isfinite(v) and v > 0.0 for v in rad):
            raise ValueError("radii must hold one finite radius > 0 per ring")
        if phases is None:
            ph = [math.pi / v for v in sizes]
        else:
            ph = [float(v) for v in phases]
            if len(ph) != len(sizes) or not all(math.isfinite(v) for v in ph):
                raise ValueError("phases must hold one finite angle per ring")
        M = sum(sizes)
        if M < 2 or M > MAX_POINTS or M & (M - 1):
            raise ValueError(f"the rings must hold a power of two in 2 .. {MAX_POINTS} points in all, got {M}")
        run = np.concatenate([r * np.exp(1j * (p + 2.0 * math.pi * np.arange(k) / k)) for k, r, p in zip(sizes, rad, ph)])
        if labels is None:
            pts = run
        else:
            lab = np.asarray(labels)
            if lab.ndim != 1 or lab.size != M or not np.issubdtype(lab.dtype, np.integer) or \
                    not np.array_equal(np.sort(lab.astype(np.int64)), np.arange(M)):
                raise ValueError(f"labels must be a permutation of 0 .. {M - 1}")
            pts = np.empty(M, dtype=np.complex128)
            pts[lab.astype(np.int64)] = run
        kwargs.setdefault("name", "apsk" + "+".join(str(v) for v in sizes))
        return cls(pts, **kwargs)

    @classmethod
    def from_modulation(cls, modulation: Modulation, **kwargs) -> "Constellation":
        """the table of an existing scheme of at most 6 bits per symbol ("bpsk" .. "qam64"), with its fading, interleaver and
        demapper: for cross-checks of the joint rule against the separable one.  (BPSK: this channel's noise is complex and
        snr_db means Es/N0 with N0 / 2 per dimension, where Modulation("bpsk") has real noise of variance N0.)"""
        if not isinstance(modulation, Modulation) or isinstance(modulation, Constellation):
            raise ValueError("from_modulation takes a modulation.Modulation of a named scheme")
        m = modulation.bits_per_symbol
        if m > 6:
            raise ValueError(f"{modulation.scheme!r} has {2 ** m} points: a table holds at most {MAX_POINTS}")
        h = axis_bits(m)
        lab = np.arange(2 ** m)

        def axis(first):                    # integer amplitude of the axis whose label bits are bits first .. first + h - 1
            run, i = np.zeros_like(lab), np.zeros_like(lab)
            for k in range(h):
                run = run ^ ((lab >> (first + k)) & 1)
                i = (i << 1) | run
            return ((2 ** h - 1) - 2 * i).astype(np.float64)

        pts = axis(0) + 1j * (axis(h) if m > 1 else 0.0)
        kwargs.setdefault("fading", modulation.fading)
        kwargs.setdefault("interleaver", modulation.interleaver)
        kwargs.setdefault("demapper", modulation.demapper)
        kwargs.setdefault("name", modulation.scheme)
        return cls(pts * half_spacing(m), **kwargs)
