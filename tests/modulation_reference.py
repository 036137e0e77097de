"""
numpy restatement of the symbol channel (include/ldpc_hip.h "symbol channel") on top of
tests/philox_reference.py: the Gray labelling, the counter word 0x40000000 | s, the fading gain g and the normals z in float64
from exact fp32 uniforms, and the fp32 max-log demapper exactly as defined -- every multiply and add rounded to fp32 on its
own -- applied to given (vI, vQ, e).  Not a test module; tests/test_modulation_host.py and the GPU tests import it.
"""
import numpy as np

import philox_reference as ref

SCHEMES = {"bpsk": 1, "qpsk": 2, "qam16": 4, "qam64": 6, "qam256": 8}
SYM_TAG = 0x40000000
F32 = np.float32


def axis_bits(m):
    return 1 if m == 1 else m // 2


def half_spacing(m):
    """d of the unit-energy constellation (float64)"""
    return 1.0 if m == 1 else np.sqrt(3.0 / (2.0 * (4.0 ** axis_bits(m) - 1.0)))


def level_index(bits):
    """gray_to_binary of label bits [..., h], b_0 first (the most significant): the running XOR"""
    bits = np.asarray(bits, dtype=np.int64)
    run = np.bitwise_xor.accumulate(bits, axis=-1)
    h = bits.shape[-1]
    return (run << np.arange(h - 1, -1, -1)).sum(axis=-1)


def amplitude(bits):
    """integer amplitude a = (2^h - 1) - 2 i of label bits [..., h]"""
    h = np.asarray(bits).shape[-1]
    return (2 ** h - 1) - 2 * level_index(bits)


def level_labels(h):
    """int [2^h, h]: label bits (b_0 first) of level i = 0 .. 2^h - 1, i.e. of amplitudes (2^h - 1) - 2 i"""
    i = np.arange(2 ** h)
    gray = i ^ (i >> 1)
    return (gray[:, None] >> np.arange(h - 1, -1, -1)[None, :]) & 1


def symbol_bits(codeword_bits, m, pos=None):
    """0/1 [batch, n] codeword bits (variable order) -> transmitted bits [batch, S, m]: transmit index t = s m + k carries
    variable pos[t]; pad bits are 0"""
    c = np.asarray(codeword_bits, dtype=np.int64)
    batch, n = c.shape
    S = (n + m - 1) // m
    tx = c if pos is None else c[:, np.asarray(pos)]
    out = np.zeros((batch, S * m), dtype=np.int64)
    out[:, :n] = tx
    return out.reshape(batch, S, m)


def sent_amplitudes(sym_bits, m):
    """int [batch, S, 2]: (aI, aQ); aQ = 0 for m = 1"""
    h = axis_bits(m)
    aI = amplitude(sym_bits[..., :h])
    aQ = amplitude(sym_bits[..., h:2 * h]) if m > 1 else np.zeros_like(aI)
    return np.stack([aI, aQ], axis=-1)


def symbol_words(batch, S, seed, stream_id=0, first_frame=0):
    """uint32 [batch, S, 4]: the Philox words of symbol s of frame first_frame + b (third counter word 0x40000000 | s)"""
    f = (np.uint64(first_frame) + np.arange(batch, dtype=np.uint64))[:, None]
    s = np.arange(S, dtype=np.uint64)[None, :] | np.uint64(SYM_TAG)
    seed = int(seed) & (2 ** 64 - 1)
    x = ref.philox4x32_10(f & ref.MASK, f >> np.uint64(32), s, np.uint64(int(stream_id) & 0xFFFFFFFF),
                          np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32))
    return np.stack(x, axis=-1)


def symbol_normals(words):
    """float64 [batch, S, 2] = (zI, zQ): u and theta exact in fp32, log / sqrt / sin / cos in float64"""
    u = ref.uniform(words)
    r = np.sqrt(-2.0 * np.log(u[..., 0].astype(np.float64)))
    theta = (ref.TWO_PI_F32 * u[..., 1]).astype(np.float64)
    return np.stack([r * np.cos(theta), r * np.sin(theta)], axis=-1)


def fading_gain(words):
    """float64 [batch, S]: g = sqrt(-log(u(x2))), u exact in fp32"""
    u = ref.uniform(words)[..., 2].astype(np.float64)
    return np.sqrt(-np.log(u))


def demap_axis(v, e, h):
    """fp32 [..., h]: the axis LLRs of received v at gain e, exactly as the kernel rounds them"""
    v, e = np.asarray(v, dtype=F32), np.asarray(e, dtype=F32)
    L = 2 ** h
    amps = ((L - 1) - 2 * np.arange(L)).astype(F32)
    ec = (e[..., None] * amps).astype(F32)                     # e * (float)a'
    t = (v[..., None] - ec).astype(F32)
    D = (t * t).astype(F32)
    labels = level_labels(h)
    out = np.empty(v.shape + (h,), dtype=F32)
    for k in range(h):
        m1 = D[..., labels[:, k] == 1].min(axis=-1)
        m0 = D[..., labels[:, k] == 0].min(axis=-1)
        out[..., k] = F32(0.5) * (m1 - m0).astype(F32)
    return out


def demap(received, m):
    """fp32 [batch, S, m]: the LLRs of the symbols' bits from received [batch, S, 4] = (vI, vQ, e, 0)"""
    received = np.asarray(received, dtype=F32)
    h = axis_bits(m)
    out = demap_axis(received[..., 0], received[..., 2], h)
    if m > 1:
        out = np.concatenate([out, demap_axis(received[..., 1], received[..., 2], h)], axis=-1)
    return out


def to_variables(sym_llr, n, pos=None):
    """[batch, S, m] in transmit order -> [batch, n] in variable order: llr[:, pos[t]] = transmit LLR t"""
    batch = sym_llr.shape[0]
    tx = sym_llr.reshape(batch, -1)[:, :n]
    if pos is None:
        return tx
    out = np.empty_like(tx)
    out[:, np.asarray(pos)] = tx
    return out


def constellation(m):
    """(complex points [2^m] of the unit-energy constellation, label bits [2^m, m]) over all labels"""
    labels = (np.arange(2 ** m)[:, None] >> np.arange(m)[None, :]) & 1            # bit k of the symbol at column k
    a = sent_amplitudes(labels[None, :, :], m)[0]
    d = half_spacing(m)
    return d * (a[:, 0] + 1j * a[:, 1]), labels


def brute_force_maxlog(v, e, m):
    """float64 [..., m]: 0.5 (min_{x: b_k = 1} |v - e x|^2 - min_{x: b_k = 0} |v - e x|^2) over all 2^m points, with x in
    integer-amplitude units (v complex, e real): the joint max-log demapper the separable one must equal"""
    labels = (np.arange(2 ** m)[:, None] >> np.arange(m)[None, :]) & 1
    a = sent_amplitudes(labels[None, :, :], m)[0].astype(np.float64)
    pts = a[:, 0] + 1j * a[:, 1]
    v = np.asarray(v, dtype=np.complex128)
    e = np.asarray(e, dtype=np.float64)
    D = np.abs(v[..., None] - e[..., None] * pts) ** 2
    out = np.empty(v.shape + (m,), dtype=np.float64)
    for k in range(m):
        out[..., k] = 0.5 * (D[..., labels[:, k] == 1].min(axis=-1) - D[..., labels[:, k] == 0].min(axis=-1))
    return out
