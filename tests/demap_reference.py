"""
numpy restatement of the exact (log-MAP) demapper of include/ldpc_hip.h "symbol channel / demappers", on top of
tests/modulation_reference.py: the fp32 rule exactly as defined (every operation rounded to fp32 on its own, the sums in
ascending level index, each set normalised by its own minimum), the float64 correction from the fp32 distances, a brute-force
float64 log-sum-exp over all 2^m constellation points, and the error bounds the tests share.  Not a test module;
tests/test_demap_host.py and the GPU tests import it.
"""
import numpy as np

import modulation_reference as mref

F32 = np.float32
EPS = 2.0 ** -23                     # an fp32 ulp is at most this fraction of the value


def distances(v, e, h):
    """fp32 [..., 2^h]: D(a') = (v - e * (float)a')^2 as sym_axis forms them, level index ascending"""
    v, e = np.asarray(v, dtype=F32), np.asarray(e, dtype=F32)
    L = 2 ** h
    amps = ((L - 1) - 2 * np.arange(L)).astype(F32)
    ec = (e[..., None] * amps).astype(F32)
    t = (v[..., None] - ec).astype(F32)
    return (t * t).astype(F32)


def exact_axis(v, e, h):
    """fp32 [..., h]: the exact rule, rounded as the kernel rounds it (numpy's fp32 exp and log stand in for expf and logf)"""
    D = distances(v, e, h)
    labels = mref.level_labels(h)
    out = np.empty(D.shape[:-1] + (h,), dtype=F32)
    for k in range(h):
        m, S = [], []
        for b in (0, 1):
            cols = np.flatnonzero(labels[:, k] == b)               # ascending level index
            mb = D[..., cols].min(axis=-1)
            s = np.zeros(mb.shape, dtype=F32)
            for c in cols:
                x = (D[..., c] - mb).astype(F32)
                s = (s + np.exp((F32(-0.5) * x).astype(F32)).astype(F32)).astype(F32)
            m.append(mb)
            S.append(s)
        corr = (np.log(S[0]).astype(F32) - np.log(S[1]).astype(F32)).astype(F32)
        ml = (F32(0.5) * (m[1] - m[0]).astype(F32)).astype(F32)
        out[..., k] = (ml + corr).astype(F32)
    return out


def correction64(v, e, h):
    """float64 [..., h]: c_k = log S_0 - log S_1 in float64 from the restated fp32 distances"""
    D = distances(v, e, h).astype(np.float64)
    labels = mref.level_labels(h)
    out = np.empty(D.shape[:-1] + (h,), dtype=np.float64)
    for k in range(h):
        logs = []
        for b in (0, 1):
            Db = D[..., labels[:, k] == b]
            logs.append(np.log(np.exp(-0.5 * (Db - Db.min(axis=-1, keepdims=True))).sum(axis=-1)))
        out[..., k] = logs[0] - logs[1]
    return out


def exact(received, m):
    """fp32 [batch, S, m]: exact_axis on (vI, e) and (vQ, e) of received [batch, S, 4]"""
    received = np.asarray(received, dtype=F32)
    h = mref.axis_bits(m)
    out = exact_axis(received[..., 0], received[..., 2], h)
    if m > 1:
        out = np.concatenate([out, exact_axis(received[..., 1], received[..., 2], h)], axis=-1)
    return out


def correction(received, m):
    """float64 [batch, S, m]: correction64 per axis"""
    received = np.asarray(received, dtype=F32)
    h = mref.axis_bits(m)
    out = correction64(received[..., 0], received[..., 2], h)
    if m > 1:
        out = np.concatenate([out, correction64(received[..., 1], received[..., 2], h)], axis=-1)
    return out


def brute_force_exact(v, e, m):
    """float64 [..., m]: log sum_{x: b_k = 0} exp(-|v - e x|^2 / 2) - log sum_{x: b_k = 1} exp(-|v - e x|^2 / 2) over all 2^m
    points x in integer-amplitude units (v complex, e real): the joint log-MAP demapper that the per-axis rule must equal"""
    labels = (np.arange(2 ** m)[:, None] >> np.arange(m)[None, :]) & 1
    a = mref.sent_amplitudes(labels[None, :, :], m)[0].astype(np.float64)
    pts = a[:, 0] + 1j * a[:, 1]
    v = np.asarray(v, dtype=np.complex128)
    e = np.asarray(e, dtype=np.float64)
    D = np.abs(v[..., None] - e[..., None] * pts) ** 2
    out = np.empty(v.shape + (m,), dtype=np.float64)
    for k in range(m):
        lse = []
        for b in (0, 1):
            Db = D[..., labels[:, k] == b]
            mn = Db.min(axis=-1, keepdims=True)
            lse.append(-0.5 * mn[..., 0] + np.log(np.exp(-0.5 * (Db - mn)).sum(axis=-1)))
        out[..., k] = lse[0] - lse[1]
    return out


def ulp32(x):
    """float64: the spacing of fp32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def correction_tolerance(h):
    """An absolute bound on |c_k (fp32 arithmetic) - c_k (float64 arithmetic)| from the same fp32 distances, for expf and logf
    good to 1 ulp (HIP documents both at 1 ulp; 2 ulp is taken for each to be on the safe side, as G_RTOL of
    tests/test_gpu_channel_sym.py does, and every other rounding is counted as a whole ulp, EPS = 2^-23 of the value).
    A set has T = 2^h / 2 terms.
      x = D - m_b is rounded once: a term exp(-x / 2) moves by at most (x / 2) EPS exp(-x / 2) <= EPS / e (y exp(-y) <= 1 / e),
        the term of the minimum has x = 0 exactly: (T - 1) EPS / e in all, relative to S >= 1
      expf at 2 ulp: every term, so the sum, by 2 EPS relative
      T - 1 additions, each rounding a partial sum <= S: (T - 1) EPS relative
    so S is off by rel_S = ((T - 1) (1 + 1 / e) + 2) EPS relative and log S by the same amount absolute (11.6 EPS = 1.4e-6 for
    h = 4).  logf at 2 ulp of a value <= log T adds 2 ulp32(log T), the subtraction of the two logs rounds a value <= log T
    once more:  2 (rel_S + 2 ulp32(log T)) + ulp32(log T)  = 4.0e-6 for h = 4, 2.6e-6 for h = 3, 1.2e-6 for h = 2.
    The rounding of the final sum 0.5f * (m1 - m0) + c_k, at most ulp32(llr), is added by the caller."""
    T = 2 ** h // 2
    if T == 1:
        return 0.0
    rel_s = ((T - 1) * (1.0 + 1.0 / np.e) + 2.0) * EPS
    u = float(ulp32(np.log(T)))
    return 2.0 * (rel_s + 2.0 * u) + u
