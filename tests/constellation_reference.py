"""
numpy restatement of the constellation channel (include/ldpc_hip.h "constellation channel") on top of
tests/philox_reference.py and tests/modulation_reference.py, whose frame layout, counter words, normals and fading gain it
uses unchanged: the labels, the fp32 joint rule exactly as defined -- every multiply and add rounded to fp32 on its own, the
candidates in ascending label order -- applied to given (vI, vQ, e), the exact rule's correction in float64 from the fp32
distances, a float64 brute force of both rules, and the error bounds the tests share.  Not a test module;
tests/test_constellation_host.py and the GPU tests import it.

A table is float32 [2^m, 2] = (xI, xQ), entry l the point of label l = sum_k b_k 2^k: ``Constellation.points``.
"""
import numpy as np

import modulation_reference as mref

F32 = np.float32
EPS = 2.0 ** -23                     # an fp32 ulp is at most this fraction of the value


def bits_of(table):
    return int(np.asarray(table).shape[0]).bit_length() - 1


def label_bits(m):
    """int [2^m, m]: bit k of label c at column k"""
    return (np.arange(2 ** m)[:, None] >> np.arange(m)[None, :]) & 1


def labels_of(sym_bits):
    """transmitted bits [..., m] (mref.symbol_bits) -> labels l = sum_k b_k 2^k"""
    sym_bits = np.asarray(sym_bits, dtype=np.int64)
    return (sym_bits << np.arange(sym_bits.shape[-1])).sum(axis=-1)


def sent_points(table, sym_bits):
    """float32 [..., 2]: the table entry of each symbol's label"""
    return np.asarray(table, dtype=F32)[labels_of(sym_bits)]


def received32(table, sym_bits, e, z):
    """float32 [..., 2]: v = (e * x_l) + z with both operations rounded to fp32 (e fp32 [...], z fp32 [..., 2])"""
    x = sent_points(table, sym_bits)
    e, z = np.asarray(e, dtype=F32), np.asarray(z, dtype=F32)
    return ((e[..., None] * x).astype(F32) + z).astype(F32)


def received64(table, sym_bits, e, z):
    """float64 [..., 2]: v = e * x_l + z in float64 from the fp32 table"""
    x = sent_points(table, sym_bits).astype(np.float64)
    return np.asarray(e, dtype=np.float64)[..., None] * x + np.asarray(z, dtype=np.float64)


def distances(received, table):
    """fp32 [..., 2^m]: D_c = (tI * tI) + (tQ * tQ), tI = vI - (e * xI_c), tQ = vQ - (e * xQ_c), of received [..., 4]"""
    r = np.asarray(received, dtype=F32)
    t = np.asarray(table, dtype=F32)
    vI, vQ, e = r[..., 0, None], r[..., 1, None], r[..., 2, None]
    tI = (vI - (e * t[:, 0]).astype(F32)).astype(F32)
    tQ = (vQ - (e * t[:, 1]).astype(F32)).astype(F32)
    return ((tI * tI).astype(F32) + (tQ * tQ).astype(F32)).astype(F32)


def _minima(D, m, k):
    lab = label_bits(m)[:, k]
    return D[..., lab == 0].min(axis=-1), D[..., lab == 1].min(axis=-1)


def demap(received, table):
    """fp32 [..., m]: the max-log LLRs 0.5f * (m_1 - m_0) of received [..., 4] = (vI, vQ, e, 0), as the kernel rounds them"""
    m = bits_of(table)
    D = distances(received, table)
    out = np.empty(D.shape[:-1] + (m,), dtype=F32)
    for k in range(m):
        m0, m1 = _minima(D, m, k)
        out[..., k] = (F32(0.5) * (m1 - m0).astype(F32)).astype(F32)
    return out


def exact(received, table):
    """fp32 [..., m]: the exact rule, rounded as the kernel rounds it (numpy's fp32 exp and log stand in for expf and logf)"""
    m = bits_of(table)
    D = distances(received, table)
    lab = label_bits(m)
    out = np.empty(D.shape[:-1] + (m,), dtype=F32)
    for k in range(m):
        mins, sums = [], []
        for b in (0, 1):
            cols = np.flatnonzero(lab[:, k] == b)                  # ascending label
            mb = D[..., cols].min(axis=-1)
            s = np.zeros(mb.shape, dtype=F32)
            for c in cols:
                x = (D[..., c] - mb).astype(F32)
                s = (s + np.exp((F32(-0.5) * x).astype(F32)).astype(F32)).astype(F32)
            mins.append(mb)
            sums.append(s)
        corr = (np.log(sums[0]).astype(F32) - np.log(sums[1]).astype(F32)).astype(F32)
        ml = (F32(0.5) * (mins[1] - mins[0]).astype(F32)).astype(F32)
        out[..., k] = (ml + corr).astype(F32)
    return out


def correction(received, table):
    """float64 [..., m]: log S_0 - log S_1 in float64 arithmetic from the restated fp32 distances"""
    m = bits_of(table)
    D = distances(received, table).astype(np.float64)
    lab = label_bits(m)
    out = np.empty(D.shape[:-1] + (m,), dtype=np.float64)
    for k in range(m):
        logs = []
        for b in (0, 1):
            Db = D[..., lab[:, k] == b]
            logs.append(np.log(np.exp(-0.5 * (Db - Db.min(axis=-1, keepdims=True))).sum(axis=-1)))
        out[..., k] = logs[0] - logs[1]
    return out


def _distances64(v, e, table):
    pts = np.asarray(table, dtype=np.float64)
    pts = pts[:, 0] + 1j * pts[:, 1]
    v = np.asarray(v, dtype=np.complex128)
    e = np.asarray(e, dtype=np.float64)
    return np.abs(v[..., None] - e[..., None] * pts) ** 2


def brute_force_maxlog(v, e, table):
    """float64 [..., m]: 0.5 (min_{b_k = 1} |v - e x|^2 - min_{b_k = 0} |v - e x|^2) over the table (v complex, e real)"""
    m = bits_of(table)
    D = _distances64(v, e, table)
    out = np.empty(D.shape[:-1] + (m,), dtype=np.float64)
    for k in range(m):
        m0, m1 = _minima(D, m, k)
        out[..., k] = 0.5 * (m1 - m0)
    return out


def brute_force_exact(v, e, table):
    """float64 [..., m]: log sum_{b_k = 0} exp(-|v - e x|^2 / 2) - log sum_{b_k = 1} exp(-|v - e x|^2 / 2) over the table"""
    m = bits_of(table)
    D = _distances64(v, e, table)
    lab = label_bits(m)
    out = np.empty(D.shape[:-1] + (m,), dtype=np.float64)
    for k in range(m):
        lse = []
        for b in (0, 1):
            Db = D[..., lab[:, k] == b]
            mn = Db.min(axis=-1, keepdims=True)
            lse.append(-0.5 * mn[..., 0] + np.log(np.exp(-0.5 * (Db - mn)).sum(axis=-1)))
        out[..., k] = lse[0] - lse[1]
    return out


def to_variables(sym_llr, n, pos=None):
    return mref.to_variables(sym_llr, n, pos)


def ulp32(x):
    """float64: the spacing of fp32 at |x|"""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(F32)).astype(np.float64)


def distance_tolerance(received, table):
    """float64 [...]: a bound on |D_c (fp32) - D_c (float64 arithmetic on the same fp32 v, e, x)|, over all c, per sample.
    Every fp32 operation is off by at most EPS = 2^-23 of its result (half that under round-to-nearest; a whole ulp is taken).
    With R = max |coordinate| of the table and Dm = the largest D_c of the sample, |e x| <= e R and |t| <= sqrt(Dm):
      e * x rounds once:                      |d(e x)| <= EPS e R
      t = v - (e x) carries that and rounds:  |dt| <= EPS (e R + sqrt(Dm))                                     =: dt
      q = t * t:                              |dq| <= 2 |t| dt + EPS t^2
      D = qI + qQ:                            |dD| <= 2 (|tI| + |tQ|) dt + EPS (tI^2 + tQ^2) + EPS D
                                                   <= 2 sqrt(2 Dm) dt + 2 EPS Dm          (|tI| + |tQ| <= sqrt(2 D))
    to first order in EPS; the second-order terms are below EPS times this and 1 % is added for them."""
    r = np.asarray(received, dtype=np.float64)
    R = float(np.abs(np.asarray(table, dtype=np.float64)).max())
    Dm = distances(received, table).astype(np.float64).max(axis=-1)
    dt = EPS * (r[..., 2] * R + np.sqrt(Dm))
    return 1.01 * (2.0 * np.sqrt(2.0 * Dm) * dt + 2.0 * EPS * Dm)


def llr_tolerance(received, table):
    """float64 [...]: a bound on |fp32 max-log LLR - float64 brute force| from the same fp32 (v, e, table).  A minimum of
    perturbed values lies within the largest perturbation of the minimum of the true ones, so m_1 - m_0 is off by at most
    2 dD (distance_tolerance), its own rounding adds EPS |m_1 - m_0| <= EPS Dm, and the multiplication by 0.5f is exact:
    dD + 0.5 EPS Dm.  The same bound holds for log sum exp(-D / 2) of either set, which is 1-Lipschitz in max |d(D / 2)|: the
    exact rule with float64 sums moves by at most dD as well."""
    Dm = distances(received, table).astype(np.float64).max(axis=-1)
    return distance_tolerance(received, table) + 0.5 * EPS * Dm


def correction_tolerance(m):
    """An absolute bound on |c_k (fp32 arithmetic) - c_k (float64 arithmetic)| from the same fp32 distances, derived as
    tests/demap_reference.correction_tolerance derives it, for the joint rule's sets of T = 2^(m-1) terms: expf and logf
    good to 1 ulp (HIP documents both at 1 ulp; 2 ulp is taken for each to be on the safe side) and every other rounding
    counted as a whole ulp, EPS = 2^-23 of the value.
      x = D_c - m_b is rounded once: a term exp(-x / 2) moves by at most (x / 2) EPS exp(-x / 2) <= EPS / e (y exp(-y) <= 1 / e);
        the term of the minimum has x = 0 exactly: (T - 1) EPS / e in all, relative to S >= 1
      -0.5f * x is exact (a power of two)
      expf at 2 ulp: every term, so the sum, by 2 EPS relative
      T - 1 additions, each rounding a partial sum <= S: (T - 1) EPS relative
    so S is off by rel_S = ((T - 1) (1 + 1 / e) + 2) EPS relative and log S by the same amount absolute.  logf at 2 ulp of a
    value <= log T adds 2 ulp32(log T); the subtraction of the two logs rounds a value <= log T once more:
        2 (rel_S + 2 ulp32(log T)) + ulp32(log T)
    = 0 for m = 1 (T = 1: both sums are 1.0f), 1.1e-6 for m = 2, 2.1e-6 for m = 3, 4.0e-6 for m = 4, 6.6e-6 for m = 5 and
    1.2e-5 for m = 6.  The rounding of the final sum 0.5f * (m_1 - m_0) + c_k, at most ulp32(llr), is added by the caller."""
    T = 2 ** (m - 1)
    if T == 1:
        return 0.0
    rel_s = ((T - 1) * (1.0 + 1.0 / np.e) + 2.0) * EPS
    u = float(ulp32(np.log(T)))
    return 2.0 * (rel_s + 2.0 * u) + u
