"""
numpy restatement of the demapper with a priori LLRs (include/ldpc_hip.h "ldpc_demap_con_prior") on top of
tests/constellation_reference.py, whose labels, fp32 distances D_c and frame layout it uses unchanged: the a priori LLRs of a
symbol's bits, the fp32 rule exactly as defined -- every operation rounded to fp32 on its own, A_c by the one-add recursion,
the candidates in ascending label order -- a float64 brute force of both rules, and the error bounds the tests share.  Not a
test module; tests/test_demap_prior_host.py and the GPU tests import it.

    La_k  = prior_scale * (prior[j_k] - prior_sub[j_k])        (+0.0f for a pad bit)
    A_c   = A_{c without its highest set bit} + La_{that bit},  A_0 = 0.0f
    Lam_c = D_c + (2.0f * A_c)
    M_b(k) = min over c with bit k of c equal to b of Lam_c
    max-log:  llr_k = 0.5f * (M_1 - M_0) - La_k
    exact:    S_b = sum_{c: bit k = b, ascending c} expf(-0.5f * (Lam_c - M_b))
              llr_k = (0.5f * (M_1 - M_0) + (logf(S_0) - logf(S_1))) - La_k
"""
import numpy as np

import constellation_reference as cref

F32 = cref.F32
EPS = cref.EPS


def apriori(prior, prior_sub=None, prior_scale=1.0):
    """fp32 [batch, n]: prior_scale * (prior - prior_sub), the subtraction and the product each rounded to fp32"""
    la = np.asarray(prior, dtype=F32)
    if prior_sub is not None:
        la = (la - np.asarray(prior_sub, dtype=F32)).astype(F32)
    return (F32(prior_scale) * la).astype(F32)


def symbol_priors(la, m, pos=None):
    """fp32 [batch, n] in variable order -> [batch, S, m] in transmit order: bit k of symbol s carries variable pos[s m + k];
    the pad bits of the last symbol get +0.0f"""
    la = np.asarray(la, dtype=F32)
    batch, n = la.shape
    S = (n + m - 1) // m
    out = np.zeros((batch, S * m), dtype=F32)
    out[:, :n] = la if pos is None else la[:, np.asarray(pos)]
    return out.reshape(batch, S, m)


def label_sums(la_sym):
    """fp32 [..., 2^m]: A_c of la_sym [..., m] by the recursion A_c = A_{c without its highest set bit} + La_{that bit}"""
    la_sym = np.asarray(la_sym, dtype=F32)
    m = la_sym.shape[-1]
    A = np.zeros(la_sym.shape[:-1] + (2 ** m,), dtype=F32)
    for c in range(1, 2 ** m):
        h = c.bit_length() - 1
        A[..., c] = (A[..., c - (1 << h)] + la_sym[..., h]).astype(F32)
    return A


def metrics(received, table, la_sym):
    """fp32 [..., 2^m]: Lam_c = D_c + (2.0f * A_c)"""
    D = cref.distances(received, table)
    return (D + (F32(2.0) * label_sums(la_sym)).astype(F32)).astype(F32)


def demap(received, table, la_sym):
    """fp32 [..., m]: the max-log extrinsic LLRs, as the kernel rounds them"""
    m = cref.bits_of(table)
    la_sym = np.asarray(la_sym, dtype=F32)
    Lam = metrics(received, table, la_sym)
    out = np.empty(Lam.shape[:-1] + (m,), dtype=F32)
    for k in range(m):
        m0, m1 = cref._minima(Lam, m, k)
        out[..., k] = ((F32(0.5) * (m1 - m0).astype(F32)).astype(F32) - la_sym[..., k]).astype(F32)
    return out


def exact(received, table, la_sym):
    """fp32 [..., m]: the exact rule, rounded as the kernel rounds it (numpy's fp32 exp and log stand in for expf and logf);
    one bit per symbol is the max-log rule"""
    m = cref.bits_of(table)
    if m == 1:
        return demap(received, table, la_sym)
    la_sym = np.asarray(la_sym, dtype=F32)
    Lam = metrics(received, table, la_sym)
    lab = cref.label_bits(m)
    out = np.empty(Lam.shape[:-1] + (m,), dtype=F32)
    for k in range(m):
        mins, sums = [], []
        for b in (0, 1):
            cols = np.flatnonzero(lab[:, k] == b)                  # ascending label
            mb = Lam[..., cols].min(axis=-1)
            s = np.zeros(mb.shape, dtype=F32)
            for c in cols:
                x = (Lam[..., c] - mb).astype(F32)
                s = (s + np.exp((F32(-0.5) * x).astype(F32)).astype(F32)).astype(F32)
            mins.append(mb)
            sums.append(s)
        corr = (np.log(sums[0]).astype(F32) - np.log(sums[1]).astype(F32)).astype(F32)
        ml = (F32(0.5) * (mins[1] - mins[0]).astype(F32)).astype(F32)
        out[..., k] = ((ml + corr).astype(F32) - la_sym[..., k]).astype(F32)
    return out


def exact64(received, table, la_sym):
    """float64 [..., m]: (ml + (log S_0 - log S_1)) - La_k with ml = 0.5f * (M_1 - M_0) as fp32 rounds it and the correction
    and both outer operations in float64 arithmetic from the restated fp32 Lam_c: what the device's exact rule is compared
    with, as restated max-log + cref.correction is for the rule without priors"""
    m = cref.bits_of(table)
    Lam32 = metrics(received, table, la_sym)
    Lam = Lam32.astype(np.float64)
    lab = cref.label_bits(m)
    out = np.empty(Lam.shape[:-1] + (m,), dtype=np.float64)
    for k in range(m):
        m0, m1 = cref._minima(Lam32, m, k)
        ml = (F32(0.5) * (m1 - m0).astype(F32)).astype(F32).astype(np.float64)
        logs = []
        for b in (0, 1):
            Lb = Lam[..., lab[:, k] == b]
            logs.append(np.log(np.exp(-0.5 * (Lb - Lb.min(axis=-1, keepdims=True))).sum(axis=-1)))
        out[..., k] = ml + (logs[0] - logs[1]) - np.asarray(la_sym, dtype=np.float64)[..., k]
    return out


def to_variables(sym_llr, n, pos=None):
    return cref.to_variables(sym_llr, n, pos)


def _scores64(v, e, table, la_sym):
    """float64 [..., 2^m]: -D_c / 2 - sum_j b_j(c) La_j, the log-probability of candidate c up to a constant"""
    m = cref.bits_of(table)
    D = cref._distances64(v, e, table)
    la = np.asarray(la_sym, dtype=np.float64)
    return -0.5 * D - (la[..., None, :] * cref.label_bits(m)).sum(axis=-1)


def brute_force_exact(v, e, table, la_sym):
    """float64 [..., m]: log sum_{b_k = 0} exp(score_c) - log sum_{b_k = 1} exp(score_c) - La_k (v complex, e real)"""
    m = cref.bits_of(table)
    sc = _scores64(v, e, table, la_sym)
    lab = cref.label_bits(m)
    out = np.empty(sc.shape[:-1] + (m,), dtype=np.float64)
    for k in range(m):
        lse = []
        for b in (0, 1):
            sb = sc[..., lab[:, k] == b]
            mx = sb.max(axis=-1, keepdims=True)
            lse.append(mx[..., 0] + np.log(np.exp(sb - mx).sum(axis=-1)))
        out[..., k] = lse[0] - lse[1] - np.asarray(la_sym, dtype=np.float64)[..., k]
    return out


def brute_force_maxlog(v, e, table, la_sym):
    """float64 [..., m]: max_{b_k = 0} score_c - max_{b_k = 1} score_c - La_k"""
    m = cref.bits_of(table)
    sc = _scores64(v, e, table, la_sym)
    lab = cref.label_bits(m)
    out = np.empty(sc.shape[:-1] + (m,), dtype=np.float64)
    for k in range(m):
        out[..., k] = (sc[..., lab[:, k] == 0].max(axis=-1) - sc[..., lab[:, k] == 1].max(axis=-1)
                       - np.asarray(la_sym, dtype=np.float64)[..., k])
    return out


def llr_tolerance(received, table, la_sym):
    """float64 [...]: a bound on |fp32 max-log extrinsic LLR - float64 brute force| from the same fp32 (v, e, table, La), per
    sample and for every bit of it.  EPS = 2^-23 bounds the relative rounding of one fp32 operation (a whole ulp is taken, as
    in cref.llr_tolerance).  With Dm the sample's largest D_c, dD = cref.distance_tolerance and SA = sum_j |La_j|:
      A_c: the first add (to 0.0f) is exact, each of the at most m - 1 others rounds a partial sum <= SA:  |dA| <= (m - 1) EPS SA
      2.0f * A_c is exact;  Lam_c = D_c + 2 A_c rounds a value in [-2 SA, Dm + 2 SA]:
                                     |dLam| <= dD + 2 (m - 1) EPS SA + EPS (Dm + 2 SA) = dD + EPS (Dm + 2 m SA)
      M_1 - M_0: each minimum moves by at most the largest perturbation, the difference, at most Dm + 4 SA, rounds once, and
                 the product with 0.5f is exact:       dLam + 0.5 EPS (Dm + 4 SA)
      the final subtraction rounds a value <= 0.5 Dm + 2 SA + |La_k| <= 0.5 Dm + 3 SA:   EPS (0.5 Dm + 3 SA)
    in all dD + EPS (2 Dm + (2 m + 5) SA), to first order; 1 % is added for the second-order terms.  log sum exp(-Lam / 2) of
    a set is 1-Lipschitz in max |d(Lam / 2)|, so the exact rule with float64 sums moves by no more than the max-log rule."""
    m = cref.bits_of(table)
    Dm = cref.distances(received, table).astype(np.float64).max(axis=-1)
    SA = np.abs(np.asarray(la_sym, dtype=np.float64)).sum(axis=-1)
    return cref.distance_tolerance(received, table) + 1.01 * EPS * (2.0 * Dm + (2.0 * m + 5.0) * SA)


def exact_tolerance(received, table, la_sym):
    """float64 [...]: llr_tolerance plus cref.correction_tolerance(m) -- the sums over Lam_c - M_b >= 0 are the sums that
    bound was derived for, with Lam in the place of D -- plus the one rounding more the exact rule has, of
    0.5f * (M_1 - M_0) + correction, a value of at most 0.5 Dm + 2 SA + (m - 1) log 2."""
    m = cref.bits_of(table)
    Dm = cref.distances(received, table).astype(np.float64).max(axis=-1)
    SA = np.abs(np.asarray(la_sym, dtype=np.float64)).sum(axis=-1)
    return (llr_tolerance(received, table, la_sym) + cref.correction_tolerance(m)
            + 1.01 * EPS * (0.5 * Dm + 2.0 * SA + (m - 1) * np.log(2.0)))


def device_exact_tolerance(m, want, la):
    """float64: a bound on |device exact LLR - exact64| where exact64 is `want` and the bit's prior `la`:
    cref.correction_tolerance(m) for the correction (expf, logf and the order-fixed sums against float64 from the same fp32
    Lam_c), one ulp for the add t = 0.5f * (M_1 - M_0) + correction and one for the subtraction t - La_k.  |t| <= |want| + |la|
    and the result is `want`; ulp32 is taken at |want| + |la| for both, which is at least either."""
    mag = np.abs(np.asarray(want, dtype=np.float64)) + np.abs(np.asarray(la, dtype=np.float64))
    return cref.correction_tolerance(m) + 2.0 * cref.ulp32(mag)


# ------------------------------------------------------------------ the tables the tests share (raw points, label = index)
def sp_psk8():
    """complex [8]: set-partitioned 8-PSK, label l at angle 2 pi l / 8 (natural binary labels: bit 0 splits the circle into
    two QPSK sets, bit 1 each of those into antipodal pairs)"""
    return np.exp(2j * np.pi * np.arange(8) / 8)


def sp_qam16():
    """complex [16]: a set-partitioned 16-point square grid.  With (x, y) in 0 .. 3 the label bits are b0 = (x + y) & 1,
    b1 = x & 1, b2 = ((x >> 1) + (y >> 1)) & 1, b3 = (x >> 1) & 1: every bit that is known doubles the squared distance
    inside the remaining set"""
    pts = np.empty(16, dtype=np.complex128)
    for x in range(4):
        for y in range(4):
            b = ((x + y) & 1, x & 1, ((x >> 1) + (y >> 1)) & 1, (x >> 1) & 1)
            pts[sum(v << k for k, v in enumerate(b))] = (2 * x - 3) + 1j * (2 * y - 3)
    return pts


def random_table(count, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=count) + 1j * rng.normal(size=count)
