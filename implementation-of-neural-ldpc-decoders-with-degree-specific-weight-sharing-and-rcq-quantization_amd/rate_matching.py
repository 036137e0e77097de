"""
Rate matching: which of a code's n variable nodes are punctured (not sent), which are shortened (known to the receiver)
and which bits the error counters look at -- the profile behind ``ldpc_rate_match`` of include/ldpc_hip.h.

The device channel (``engine.awgn_llr(..., rate_matching=rm)``) gives a punctured bit the LLR ``+0.0`` -- an erasure to the
min-sum kernels -- and a shortened bit ``s_j * short_llr``; every transmitted position holds the plain draw bit for bit,
because the noise counter stays on the variable index.  ``expand`` does the same scatter for rows a
user received elsewhere; ``where`` is the channel rule restated in torch.
"""

from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

import _native as nat


def _as_mask(what: str, value, n: int) -> np.ndarray:
    """an index array or a boolean mask of length n -> bool [n]"""
    a = np.asarray(value)
    if a.dtype == np.bool_:
        if a.shape != (n,):
            raise ValueError(f"{what}: a boolean mask must have length {n}, got shape {a.shape}")
        return a.copy()
    mask = np.zeros(n, dtype=bool)
    if a.size == 0:
        return mask
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must be a 1-D array of indices or a boolean mask of length {n}")
    if a.min() < 0 or a.max() >= n:
        raise ValueError(f"{what}: indices must be in 0 .. {n - 1}")
    if np.unique(a).size != a.size:
        raise ValueError(f"{what}: an index is listed twice")
    mask[a] = True
    return mask


def pack_mask(mask: np.ndarray) -> np.ndarray:
    """bool [n] -> uint8 [ceil(n/8)], bit j at byte j/8, bit j%8 (the decoders' packed format); pad bits zero"""
    return np.packbits(np.asarray(mask, dtype=np.uint8), bitorder="little")


class RateMatching:
    """RateMatching(n, punctured=(), shortened=(), count=None, short_llr=None).

    punctured, shortened, count: index arrays or boolean masks of length n; count=None counts all n bits.  A bit cannot be
    both punctured and shortened.  short_llr, the LLR magnitude of a shortened bit, is required (finite, > 0) exactly when
    something is shortened: the right magnitude depends on the decoder's quantiser, so there is no default."""

    def __init__(self, n: int, punctured=(), shortened=(), count=None, short_llr: Optional[float] = None):
        n = int(n)
        if n < 1:
            raise ValueError("n must be >= 1")
        self.n = n
        self.punctured = _as_mask("punctured", punctured, n)
        self.shortened = _as_mask("shortened", shortened, n)
        self.count = None if count is None else _as_mask("count", count, n)
        if (self.punctured & self.shortened).any():
            raise ValueError("a bit cannot be both punctured and shortened")
        if self.shortened.any():
            if short_llr is None:
                raise ValueError("short_llr is required when bits are shortened")
            short_llr = float(short_llr)
            if not (math.isfinite(short_llr) and short_llr > 0):
                raise ValueError(f"short_llr must be finite and > 0, got {short_llr!r}")
            if short_llr > float(np.finfo(np.float32).max):
                raise ValueError(f"short_llr must be finite in float32, got {short_llr!r}")
        elif short_llr is not None:
            raise ValueError("short_llr is given and nothing is shortened")
        self.short_llr = short_llr
        self.transmitted = ~(self.punctured | self.shortened)
        self._packed = {}
        self._native = {}

    @property
    def n_punctured(self) -> int:
        return int(self.punctured.sum())

    @property
    def n_shortened(self) -> int:
        return int(self.shortened.sum())

    @property
    def n_transmitted(self) -> int:
        return int(self.transmitted.sum())

    @property
    def n_counted(self) -> int:
        """bits the error counters look at (the denominator of a bit error rate)"""
        return self.n if self.count is None else int(self.count.sum())

    def effective_rate(self, k: int) -> float:
        """(k - shortened) / n_transmitted: information bits that carry data over bits sent"""
        if self.n_transmitted == 0:
            raise ValueError("no bit is transmitted")
        return (int(k) - self.n_shortened) / self.n_transmitted

    # ------------------------------------------------------------------ device side
    def packed(self, device):
        """the cached device masks (punctured, shortened, count): uint8 [ceil(n/8)] tensors, None where the native profile
        takes NULL (nothing punctured / nothing shortened / all bits counted)"""
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        got = self._packed.get(dev)
        if got is None:
            up = lambda m, use: torch.from_numpy(pack_mask(m)).to(dev) if use else None
            got = (up(self.punctured, self.punctured.any()), up(self.shortened, self.shortened.any()),
                   up(self.count, self.count is not None))
            self._packed[dev] = got
        return got

    def native(self, device) -> "nat.RateMatch":
        """the cached ldpc_rate_match of this profile on `device`; the struct points into the cached masks, and both live as
        long as this object"""
        got = self._native.get(device)
        if got is None:
            p, s, c = self.packed(device)
            ptr = lambda t: None if t is None else t.data_ptr()
            got = nat.RateMatch(punctured_packed=ptr(p), shortened_packed=ptr(s), count_packed=ptr(c),
                                short_llr=float(self.short_llr) if s is not None else 0.0)
            self._native[device] = got
        return got

    # ------------------------------------------------------------------ torch side
    def _signs(self, codeword, like: torch.Tensor) -> torch.Tensor:
        """s_j = +1 / -1 for codeword bit 0 / 1, as a row of `like`'s dtype and device"""
        if codeword is None:
            return torch.ones(self.n, dtype=like.dtype, device=like.device)
        c = np.asarray(codeword)
        if c.shape != (self.n,) or not np.isin(c, (0, 1)).all():
            raise ValueError(f"codeword must be a 0/1 array of length {self.n}")
        return torch.from_numpy(1.0 - 2.0 * c.astype(np.float64)).to(device=like.device, dtype=like.dtype)

    def where(self, llr: torch.Tensor, codeword=None) -> torch.Tensor:
        """the channel rule on a plain draw [B, n]: +0.0 where punctured, s_j * short_llr where shortened, llr elsewhere"""
        if llr.dim() != 2 or llr.shape[1] != self.n:
            raise ValueError(f"llr must be [B, {self.n}]")
        out = llr.clone()
        dev = llr.device
        if self.punctured.any():
            out[:, torch.from_numpy(self.punctured).to(dev)] = 0.0
        if self.shortened.any():
            idx = torch.from_numpy(self.shortened).to(dev)
            out[:, idx] = (self._signs(codeword, llr) * self.short_llr)[idx]
        return out

    def expand(self, tx_llr: torch.Tensor, codeword=None) -> torch.Tensor:
        """received rows [B, n_transmitted] -- the transmitted bits in ascending variable order -- scattered into [B, n] with
        +0.0 at the punctured and s_j * short_llr at the shortened positions (codeword: the shortened bits' values; None:
        all zero).  Plain torch, for users with real received data."""
        if tx_llr.dim() != 2 or tx_llr.shape[1] != self.n_transmitted:
            raise ValueError(f"tx_llr must be [B, {self.n_transmitted}]")
        out = torch.zeros((tx_llr.shape[0], self.n), dtype=tx_llr.dtype, device=tx_llr.device)
        out[:, torch.from_numpy(self.transmitted).to(tx_llr.device)] = tx_llr
        if self.shortened.any():
            idx = torch.from_numpy(self.shortened).to(tx_llr.device)
            out[:, idx] = (self._signs(codeword, tx_llr) * self.short_llr)[idx]
        return out

    def __repr__(self):
        return (f"RateMatching(n={self.n}, punctured={self.n_punctured}, shortened={self.n_shortened}, "
                f"counted={self.n_counted}, short_llr={self.short_llr})")

