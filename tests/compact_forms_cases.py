"""
Case list shared by tests/test_compact_forms.py (host: the oracle alone) and tests/test_gpu_compact_forms.py (GPU): the
decoder families that reach each of the eight compact fixed-T kernels (resident_decode<2, FORM, BPC, NL, 495, 0, float,
false, true, true>), their seeded weights, the codes and the inputs.

The inputs are a permuted mix of a low and a high SNR, chosen on the CPU so that the oracle decodes part of every batch
(tests/test_compact_forms.py asserts it): the compact plan's own syndrome then has to answer True and False, and both for
the two codewords of one workgroup.  Not a test module (no test_ prefix): nothing here needs a GPU.
"""
import os
import zlib
from collections import namedtuple

import numpy as np
import torch

from test_gpu_compact_checks import make_code as checks_code
from test_gpu_compact_grid import make_code as grid_code

QP3 = [(3.0, 1.3), (5.0, 1.3), (7.0, 1.3)]                 # bc = 3, every tau_0 == 0 (test_gpu_parity.QP)
QP3_G0 = [(3.0, 0.0), (5.0, 1.3), (7.0, 1.3)]              # gamma = 0: tau_j = C for every j, so tau_0 != 0
QPN = [(4.0, 1.2), (6.0, 1.0), (9.0, 0.8)]                 # bc = 4 / 5 (test_rcq_code_pair_form_edge_cases)
QPN_G0 = [(4.0, 0.0), (6.0, 1.0), (9.0, 0.8)]

# kind: the oracle restatement (test_gpu_parity.oracle_capped kinds, plus "edge" / "edge-offset" for one weight per edge);
# arg: sharing type; bc / qp: the quantiser; kernel: what ldpc_debug_resident_kernel must report for the fixed-T decode --
# (FORM, BPC, NL, unit_alpha, rcq_zero0, oms_alpha)
Family = namedtuple("Family", "kind arg bc qp kernel")
FAMILIES = {
    # NMS, one beta slot per check
    "n2d-3": Family("neural2d", 3, 0, None, ("NMS", True, 0, True, False, False)),
    "n2d-4": Family("neural2d", 4, 0, None, ("NMS", True, 0, False, False, False)),
    # NMS, beta slot per edge
    "n2d-1": Family("neural2d", 1, 0, None, ("NMS", False, 0, True, False, False)),
    "edge": Family("edge", 0, 0, None, ("NMS", False, 0, True, False, False)),
    # OMS, one beta slot per check, a check-side alpha per edge
    "oms2d-2": Family("offset", 2, 0, None, ("OMS", True, 0, True, False, True)),
    "oms2d-3": Family("offset", 3, 0, None, ("OMS", True, 0, True, False, True)),
    "oms2d-4": Family("offset", 4, 0, None, ("OMS", True, 0, True, False, True)),
    # OMS, beta slot per edge; the edge-weight decoder has no check-side alpha table
    "oms2d-1": Family("offset", 1, 0, None, ("OMS", False, 0, True, False, True)),
    "edge-oms": Family("edge-offset", 0, 0, None, ("OMS", False, 0, True, False, False)),
    # RCQ, 4 levels, one beta slot per check
    "wrcq3-2": Family("wrcq", 2, 3, QP3, ("RCQ", True, 4, False, True, False)),
    "wrcq3-3": Family("wrcq", 3, 3, QP3, ("RCQ", True, 4, True, True, False)),
    "wrcq3-4": Family("wrcq", 4, 3, QP3, ("RCQ", True, 4, False, True, False)),
    "rcq3-g0": Family("rcq", 0, 3, QP3_G0, ("RCQ", True, 4, True, False, False)),
    # RCQ, 4 levels, beta slot per edge
    "wrcq3-1": Family("wrcq", 1, 3, QP3, ("RCQ", False, 4, True, True, False)),
    # RCQ, run-time level count (8 and 16 levels), one beta slot per check
    "wrcq4-2": Family("wrcq", 2, 4, QPN, ("RCQ", True, 0, False, True, False)),
    "wrcq5-2": Family("wrcq", 2, 5, QPN, ("RCQ", True, 0, False, True, False)),
    "wrcq4-2-g0": Family("wrcq", 2, 4, QPN_G0, ("RCQ", True, 0, False, False, False)),
    # RCQ, run-time level count, beta slot per edge
    "wrcq4-1": Family("wrcq", 1, 4, QPN, ("RCQ", False, 0, True, True, False)),
    # RCQ, 32 and 128 levels: the threshold loop well past the register path; at 128 the negative codes use bit 7
    "wrcq6-2": Family("wrcq", 2, 6, QPN, ("RCQ", True, 0, False, True, False)),
    "wrcq8-2": Family("wrcq", 2, 8, QPN, ("RCQ", True, 0, False, True, False)),
    "wrcq8-1": Family("wrcq", 1, 8, QPN, ("RCQ", False, 0, True, True, False)),
}
# the eight instantiations (FORM, BPC, NL) and a family of each for the cases run once per instantiation
INSTANTIATIONS = {
    ("NMS", True, 0): "n2d-4", ("NMS", False, 0): "edge", ("OMS", True, 0): "oms2d-2", ("OMS", False, 0): "edge-oms",
    ("RCQ", True, 4): "wrcq3-2", ("RCQ", False, 4): "wrcq3-1", ("RCQ", True, 0): "wrcq5-2", ("RCQ", False, 0): "wrcq4-1",
}
# every (FORM, BPC, NL, unit_alpha, rcq_zero0, oms_alpha) the matrix must have run on the compact plan: the eight
# instantiations, unit_alpha on and off for NMS and RCQ, rcq_zero0 on and off for both level counts, oms_alpha present and
# absent
COVERAGE = [
    ("NMS", True, 0, True, False, False), ("NMS", True, 0, False, False, False),
    ("NMS", False, 0, True, False, False),
    ("OMS", True, 0, True, False, True),
    ("OMS", False, 0, True, False, True), ("OMS", False, 0, True, False, False),
    ("RCQ", True, 4, False, True, False), ("RCQ", True, 4, True, True, False), ("RCQ", True, 4, True, False, False),
    ("RCQ", False, 4, True, True, False),
    ("RCQ", True, 0, False, True, False), ("RCQ", True, 0, False, False, False),
    ("RCQ", False, 0, True, True, False),
]

SMALL_CODES = ["tails", "fallback", "spread"]
CODES = SMALL_CODES + ["ira"]
B_FULL = 37                                 # odd: the last workgroup holds one real codeword
T_FULL = 10

# (low, high) SNR in dB of a case's inputs; DEFAULT_SNR unless the (family, code) is listed.  Chosen on the
# CPU from the oracle's success counts alone (tests/test_compact_forms.py holds the condition)
DEFAULT_SNR = (3.0, 5.0)
SNR = {
    ("oms2d-2", "fallback"): (2.5, 5.0), ("oms2d-3", "fallback"): (2.5, 5.0), ("oms2d-4", "fallback"): (2.5, 5.0),
    ("oms2d-1", "fallback"): (2.5, 5.0),
    ("wrcq3-2", "tails"): (3.0, 6.0), ("wrcq3-2", "spread"): (3.0, 6.0), ("wrcq3-2", "ira"): (3.0, 7.0),
    ("wrcq3-3", "tails"): (3.0, 6.0), ("wrcq3-3", "spread"): (3.0, 7.0), ("wrcq3-3", "ira"): (3.0, 7.0),
    ("wrcq3-4", "tails"): (3.0, 6.0), ("wrcq3-4", "fallback"): (3.0, 6.0), ("wrcq3-4", "ira"): (3.0, 6.0),
    ("rcq3-g0", "ira"): (3.0, 6.0),
    ("wrcq3-1", "tails"): (3.0, 6.0), ("wrcq3-1", "spread"): (3.0, 6.0), ("wrcq3-1", "ira"): (3.0, 7.0),
    ("wrcq4-2", "spread"): (3.0, 6.0), ("wrcq4-2", "ira"): (3.0, 7.0),
    ("wrcq5-2", "spread"): (3.0, 6.0), ("wrcq5-2", "ira"): (3.0, 6.0),
    ("wrcq4-2-g0", "tails"): (3.0, 6.0), ("wrcq4-2-g0", "spread"): (3.0, 6.0), ("wrcq4-2-g0", "ira"): (3.0, 7.0),
    ("wrcq4-1", "tails"): (3.0, 6.0), ("wrcq4-1", "spread"): (3.0, 6.0), ("wrcq4-1", "ira"): (3.0, 6.0),
    ("wrcq6-2", "spread"): (3.0, 6.0),
}


def snr_of(family, codename):
    return SNR.get((family, codename), DEFAULT_SNR)


def make_code(name, T=T_FULL):
    return checks_code(name, T) if name in ("tails", "fallback", "ira") else grid_code(name, T)


def seed_of(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def llrs_mix(seed, B, n, snr):
    """the channel formula of test_gpu_compact_checks.llrs: half the batch at snr[0], half at snr[1], permuted"""
    rng = np.random.default_rng(seed)
    out = []
    for db in snr:
        s2 = 10.0 ** (-db / 10.0)
        out.append((2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32))
    x = np.concatenate([out[0][: B - B // 2], out[1][: B // 2]])
    return x[rng.permutation(B)]


def oracle_graph(oracle_mod, code):
    g = code.tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


def fill(params, rng, lo, hi):
    with torch.no_grad():
        for p in params.values():
            p.fill_(float(np.float32(rng.uniform(lo, hi))))


def build_decoder(family, code, T, seed):
    """-> (decoder with seeded weights in the ranges of test_gpu_parity, oracle keyword arguments of its weights).
    Weighted RCQ decoders with at least four beta parameters get one negative and one zero beta (sign of beta * min, all-zero
    magnitudes), as test_rcq_code_pair_form_edge_cases gives them.  With fewer (sharing type 4, which has none; T = 1 on a code of
    two check degrees; small-T property cases) they get neither: the T = 10 matrix is where every RCQ instantiation meets both."""
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    f = FAMILIES[family]
    rng = np.random.default_rng(seed)
    if f.kind == "rcq":
        return RCQMinSumDecoder(code, f.bc, 8, f.qp, T), dict(bc=f.bc, qp=f.qp)
    if f.kind in ("edge", "edge-offset"):
        dec = (NeuralOffsetMinSumDecoder if f.kind == "edge-offset" else NeuralMinSumDecoder)(code, max_iterations=T)
        fill(dec.beta_weights, rng, *((0.0, 0.6) if f.kind == "edge-offset" else (0.5, 1.0)))
        return dec, dict(beta={k: float(v.item()) for k, v in dec.beta_weights.items()})
    if f.kind == "neural2d":
        dec = Neural2DMinSumDecoder(code, weight_sharing_type=f.arg, max_iterations=T)
    elif f.kind == "offset":
        dec = Neural2DOffsetMinSumDecoder(code, weight_sharing_type=f.arg, max_iterations=T)
    else:
        dec = WeightedRCQDecoder(code, f.bc, 8, f.qp, weight_sharing_type=f.arg, max_iterations=T)
    offset = f.kind == "offset"
    fill(dec.beta_weights, rng, *((0.0, 0.6) if offset else (0.5, 1.0)))
    fill(dec.alpha_weights, rng, *((0.0, 0.3) if offset else (0.8, 1.2)))
    keys = sorted(dec.beta_weights.keys())
    if f.kind == "wrcq" and len(keys) >= 4:
        with torch.no_grad():
            dec.beta_weights[keys[len(keys) // 3]].fill_(-0.6)
            dec.beta_weights[keys[2 * len(keys) // 3]].fill_(0.0)
    wkw = dict(wtype=f.arg, beta={k: float(v.item()) for k, v in dec.beta_weights.items()},
               alpha={k: float(v.item()) for k, v in dec.alpha_weights.items()})
    if f.kind == "wrcq":
        wkw.update(bc=f.bc, qp=f.qp)
    return dec, wkw


def oracle_run(oracle_mod, og, family, wkw, llr, t, T):
    """the CPU oracle's fixed-T decode of t (<= T) iterations with the T-iteration decoder's tables
    -> (bits, posterior, iterations, success)"""
    from test_gpu_parity import oracle_capped
    kind = FAMILIES[family].kind
    if kind in ("edge", "edge-offset"):        # rows 0 .. t-1 of the [T][E] table: the dictionary holds every iteration
        return oracle_mod.neural_minsum(og, llr, t, wkw["beta"], offset=kind == "edge-offset", early_stop=False)
    return oracle_capped(oracle_mod, og, llr, kind, t, T, early_stop=False, **wkw)


Case = namedtuple("Case", "family code T B cap")


def case_id(c):
    return f"{c.family}-{c.code}-T{c.T}-B{c.B}" + (f"-cap{c.cap}" if c.cap else "")


def default_cases():
    """Every family at T = 10, B = 37 on the three small codes; on the (1998,1512) code one family per instantiation (the
    suite's time budget); T = 1 for every family on one of the codes in turn; per instantiation one decode at
    B = 1 and one capped at 8 of the 10 iterations (iteration 8 runs the last quantiser, whose levels are distinct in every
    family here, so that the per-edge codes can be read back from the reconstructed values)."""
    cases = [Case(f, c, T_FULL, B_FULL, 0) for f in FAMILIES for c in SMALL_CODES]
    cases += [Case(f, "ira", T_FULL, B_FULL, 0) for f in INSTANTIATIONS.values()]
    cases += [Case(f, CODES[k % len(CODES)], 1, B_FULL, 0) for k, f in enumerate(FAMILIES)]
    for k, f in enumerate(INSTANTIATIONS.values()):
        cases.append(Case(f, SMALL_CODES[k % 3], T_FULL, 1, 0))
        cases.append(Case(f, SMALL_CODES[(k + 1) % 3], T_FULL, B_FULL, 8))
    return cases


def case_inputs(c):
    code = make_code(c.code, c.T)
    # one input batch per (family, code, B): the capped case decodes the inputs of the full one
    llr = llrs_mix(seed_of("llr", c.family, c.code, c.B), c.B, code.n, snr_of(c.family, c.code))
    return code, llr


_expect = {}


def expected(oracle_mod, c):
    """oracle outputs of a case, computed once per process (the GPU file asks for each at most once per engine form)"""
    if c not in _expect:
        code, llr = case_inputs(c)
        _, wkw = build_decoder(c.family, code, c.T, seed_of("w", c.family, c.code, c.T))
        _expect[c] = oracle_run(oracle_mod, oracle_graph(oracle_mod, code), c.family, wkw, llr, c.cap or c.T, c.T)
    return _expect[c]


# ---- seeded property test: random graphs that qualify for the compact plan -----------------------------------------------
PROPERTY_SEED_BASE = 4100
PROPERTY_SEEDS = 6            # default of LDPC_FUZZ_SEEDS here (test_gpu_parity reads the same variable, default 12)


def property_seeds():
    return [PROPERTY_SEED_BASE + k for k in range(int(os.environ.get("LDPC_FUZZ_SEEDS", PROPERTY_SEEDS)))]


def property_graph(seed):
    """a random graph in the compact plan's range (m <= 495 checks, n <= 2048 variables of degree 0..8, at most 512 of
    degree > 4, about 11 edges per check at most) from the generator of tests/test_compact_layout.py
    -> (H, check_ptr, var_idx, n)"""
    from test_compact_layout import random_code
    rng = np.random.default_rng(seed)
    n = int(rng.integers(64, 2049))
    m = int(rng.integers(max(8, n // 6), min(496, n)))
    dv_seq = rng.choice(9, size=n, p=rng.dirichlet(np.ones(9) * 0.5))
    dv_seq[dv_seq > 4] = np.where(np.arange((dv_seq > 4).sum()) < 512, dv_seq[dv_seq > 4], 3)
    dv_seq = np.minimum(dv_seq, m)
    while dv_seq.sum() > 11 * m:                    # keep the checks narrow enough for the compact slot area
        dv_seq = np.maximum(dv_seq - 1, np.minimum(dv_seq, 1))
    H, cp, vi = random_code(rng, n, m, dv_seq)
    return H, cp, vi, n


def property_case(seed):
    """-> (code, family, T, B, llr) of a seed: the family from FAMILIES, T in 1..8, B in 1..70, the 3 / 5 dB mix"""
    from ldpc_decoder import LDPCCode
    H, _, _, n = property_graph(seed)
    rng = np.random.default_rng(seed_of("property", seed))
    family = sorted(FAMILIES)[int(rng.integers(len(FAMILIES)))]
    T, B = int(rng.integers(1, 9)), int(rng.integers(1, 71))
    code = LDPCCode(n=n, k=max(n - H.shape[0], 1), H=H, max_iterations=T)
    return code, family, T, B, llrs_mix(seed_of("property-llr", seed), B, n, DEFAULT_SNR)


# ---- a decode that fails ONLY in the last, partly filled check wave ------------------------------------------------------
# The 20-80 % success mix does not promise a codeword whose unsatisfied checks all sit in the plan's last check wave; these
# inputs are built to be one.  Checks are placed by descending degree, 64 to a wave, so on `tails` the last wave is the 20
# checks of degree 4.  A word x that every check accepts but ONE of the last wave (GF(2) null space of the other rows), sent with strong LLRs,
# is a fixed point of every decoder here: the lone unsatisfied check cannot outvote the checks that agree.
LAST_WAVE_CODE = "tails"
LAST_WAVE_B = 13                                 # crafted words at the even rows; the all-zero codeword, as strong, at the odd ones


def last_wave_checks(code):
    """the checks of the plan's last check wave, which must be partly filled and a whole degree class of its own"""
    dc = np.diff(code.tanner_graph().check_ptr)
    m = len(dc)
    assert m % 64
    order = np.argsort(-dc, kind="stable")
    last = np.sort(order[m - m % 64:])
    assert dc[last].max() < np.delete(dc, last).min()
    return last


def _gf2_nullspace(A):
    """basis of {x : A x = 0 over GF(2)} as rows, by row reduction"""
    A = (np.asarray(A) & 1).astype(np.uint8)
    rows, n = A.shape
    pivots, r = [], 0
    for c in range(n):
        hit = np.flatnonzero(A[r:, c])
        if len(hit) == 0:
            continue
        A[[r, r + hit[0]]] = A[[r + hit[0], r]]
        others = np.flatnonzero(A[:, c])
        others = others[others != r]
        A[others] ^= A[r]
        pivots.append(c)
        r += 1
        if r == rows:
            break
    free = [c for c in range(n) if c not in set(pivots)]
    basis = np.zeros((len(free), n), np.uint8)
    for k, f in enumerate(free):
        basis[k, f] = 1
        basis[k, pivots] = A[:len(pivots), f]
    return basis


def last_wave_inputs(code, seed):
    """-> (llr [LAST_WAVE_B, n], the sent words [LAST_WAVE_B, n]): every even row violates one check of the last wave and no other, every odd row is the all-zero codeword"""
    H = np.asarray(code.H).astype(np.uint8)
    last = last_wave_checks(code)
    rng = np.random.default_rng(seed)
    words = np.zeros((LAST_WAVE_B, code.n), np.uint8)
    for row, c in zip(range(0, LAST_WAVE_B, 2), rng.permutation(last)):
        basis = _gf2_nullspace(np.delete(H, c, axis=0))                 # every check but c accepts these words
        basis = basis[(basis @ H[c] % 2) == 1]
        words[row] = basis[np.argmin(basis.sum(axis=1))]                # the lightest one: few variables pull the other way
    mag = rng.uniform(10.0, 14.0, size=words.shape)
    return np.where(words == 1, -mag, mag).astype(np.float32), words


def last_wave_case(oracle_mod, family):
    """-> (llr, oracle outputs, rows whose unsatisfied checks -- oracle's bits -- all lie in the last check wave)"""
    key = ("last-wave", family)
    if key not in _expect:
        code = make_code(LAST_WAVE_CODE, T_FULL)
        llr, _ = last_wave_inputs(code, seed_of("last-wave"))
        _, wkw = build_decoder(family, code, T_FULL, seed_of("w", family, LAST_WAVE_CODE, T_FULL))
        want = oracle_run(oracle_mod, oracle_graph(oracle_mod, code), family, wkw, llr, T_FULL, T_FULL)
        syndrome = np.asarray(code.H) @ want[0].T % 2
        last = last_wave_checks(code)
        confined = (np.delete(syndrome, last, axis=0).sum(axis=0) == 0) & (syndrome[last].sum(axis=0) > 0)
        _expect[key] = (llr, want, np.flatnonzero(confined))
    return _expect[key]
