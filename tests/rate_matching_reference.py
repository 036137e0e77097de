"""
numpy restatement of rate matching (ldpc_rate_match of include/ldpc_hip.h): the channel rule on a plain
draw, the masked wrong-bit count, and the masked counters as philox_reference.sim_fold / sim_diag_reference.sim_fold_diag on
that count.  Not a test module; tests/test_rate_matching_host.py and tests/test_gpu_rate_matching.py import it.
"""
import numpy as np

import philox_reference as ref
import sim_diag_reference as dref


def unpack(packed, n):
    """uint8 [ceil(n/8)] -> bool [n]; None -> None.  Bits at and beyond n are dropped, whatever they hold."""
    if packed is None:
        return None
    return np.unpackbits(np.asarray(packed, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def apply(llr, punctured=None, shortened=None, short_llr=None, codeword=None):
    """the channel rule on a plain draw [B, n] (any float dtype, kept): +0.0 where punctured, s_j * short_llr where
    shortened (a bit in both masks is shortened), the draw itself elsewhere.  Masks: bool [n] or None."""
    out = np.array(llr, copy=True)
    n = out.shape[1]
    if punctured is not None:
        out[:, np.asarray(punctured, dtype=bool)] = 0.0
    if shortened is not None and np.asarray(shortened).any():
        s = np.ones(n) if codeword is None else 1.0 - 2.0 * np.asarray(codeword, dtype=np.float64)
        idx = np.asarray(shortened, dtype=bool)
        out[:, idx] = (s * np.float32(short_llr)).astype(out.dtype)[idx]
    return out


def plain_llr(batch, n, seed, stream_id, first_frame, scale, shift, codeword=None):
    """float32 [batch, n]: the plain channel with the normals of philox_reference (log / sincos in float64, so the last bit
    of an LLR can differ from the device's fp32 draw)"""
    z = ref.awgn_normals(batch, n, seed, stream_id, first_frame)
    s = np.ones(n) if codeword is None else 1.0 - 2.0 * np.asarray(codeword, dtype=np.float64)
    return (s[None, :] * (z * np.float32(scale) + np.float32(shift))).astype(np.float32)


def wrong_bits(packed, n, codeword_packed=None, count_packed=None):
    """popcount((packed XOR codeword) AND count) over bits < n per row of uint8 [B, ceil(n/8)]"""
    p = np.asarray(packed, dtype=np.uint8)
    if codeword_packed is not None:
        p = p ^ np.asarray(codeword_packed, dtype=np.uint8)[None, :]
    if count_packed is not None:
        p = p & np.asarray(count_packed, dtype=np.uint8)[None, :]
    return np.unpackbits(p, axis=1, bitorder="little")[:, :n].sum(axis=1, dtype=np.int64)


def sim_fold(state, packed, iterations, n, max_frames, max_errors, codeword_packed=None, count_packed=None):
    """ldpc_sim_count_rm on a state of 8 python ints"""
    return ref.sim_fold(state, wrong_bits(packed, n, codeword_packed, count_packed), iterations, max_frames, max_errors)


def sim_fold_diag(state, diag, packed, iterations, success, first_frame, n, T, capture, max_frames, max_errors,
                  codeword_packed=None, count_packed=None):
    """ldpc_sim_count_diag_rm -> (state, diag)"""
    return dref.sim_fold_diag(state, diag, wrong_bits(packed, n, codeword_packed, count_packed), iterations, success,
                              first_frame, T, capture, max_frames, max_errors)
