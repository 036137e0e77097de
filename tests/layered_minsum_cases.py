"""
Codes, decoder families and inputs of the layered min-sum tests (tests/test_layered_minsum_host.py on the CPU,
tests/test_gpu_layered_minsum.py on the GPU): both files decode the SAME input sets, so what the host test establishes
about them (the restatement decodes between 20 % and 80 % of every set: both answers of the syndrome, and frozen rows
beside live ones in one wave, occur) holds for the GPU comparison.
"""
import copy
import functools

import numpy as np
import torch

import layered_minsum_reference as ref

LANE_WIDTHS = (1, 2, 4, 8, 16, 32, 64)


def awgn(rng, B, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return (2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((B, n))) / s2).astype(np.float32)


def wide_check_code():
    """checks of degree 129, 100, 64, ... beside ordinary ones (the construction of tests/test_gpu_layered_weighted.py):
    wider than a wavefront, so the streaming kernel runs"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(2024)
    n, degs = 420, [129, 100, 64, 40, 33, 6, 6, 5, 7, 6, 6, 3, 1, 6, 6, 6, 16, 17, 32, 6, 6, 6, 6, 2]
    H = np.zeros((len(degs), n), dtype=np.int64)
    load = np.zeros(n, dtype=np.int64)
    for i, dc in enumerate(degs):
        pick = rng.choice(np.flatnonzero(load < 8), size=dc, replace=False)
        H[i, pick] = 1
        load[pick] += 1
    return LDPCCode(n=n, k=n - len(degs), H=H, max_iterations=8)


def lane_width_code(lw):
    """random graph whose widest check has exactly `lw` edges (it fills the row of the LDS kernel: LW = lw), with a
    degree-1 check, a degree-0 check and random degrees in between; an odd number of checks and of variables"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(9000 + lw)
    n = 2 * lw + 11
    degs = [lw, 1, 0] + [int(rng.integers(1, lw + 1)) for _ in range(10)]
    order = rng.permutation(len(degs))
    H = np.zeros((len(degs), n), dtype=np.int64)
    for row, i in enumerate(order):
        H[row, rng.choice(n, size=degs[i], replace=False)] = 1
    return LDPCCode(n=n, k=n - len(degs), H=H, max_iterations=10)


@functools.lru_cache(maxsize=None)
def load(name):
    """code by name; the iteration count is a decoder argument (``with_iterations``)"""
    import codes
    from ldpc_decoder import create_test_ldpc_code
    if name == "toy":
        return create_test_ldpc_code()
    if name == "wide":
        return wide_check_code()
    if name.startswith("lw"):
        return lane_width_code(int(name[2:]))
    return codes.load_code(name, 10)


def with_iterations(code, T):
    """the same code (and the same cached graph object) under another ``max_iterations``"""
    code.tanner_graph()                       # compiled once, shared by the copy (it carries the cache entry along)
    out = copy.copy(code)
    out.max_iterations = T
    return out


# ---- decoder families: name -> (constructor, form).  make() returns the decoder and the per-edge tables the restatement takes
FAMILIES = ("basic", "n2d1", "n2d2", "n2d3", "n2d4", "n2d_oms", "edge_nms", "edge_oms")
SHARED_FAMILIES = ("basic", "n2d1", "n2d2", "n2d3", "n2d4", "n2d_oms")     # those whose parameter count does not grow with E


def form_of(family):
    return ref.OMS if family in ("n2d_oms", "edge_oms") else ref.NMS


def randomise(dec, rng, offset_form):
    """seeded values in place of the init draws: betas with one exactly-zero and one negative slot per decoder (normalised
    form), a non-zero check-side alpha (offset form); the variable-side alphas of the normalised form are set too -- the
    layered schedule must ignore them"""
    with torch.no_grad():
        betas = list(dec.beta_weights.values())
        for p in betas:
            p.fill_(float(np.float32(rng.uniform(0.05, 0.45) if offset_form else rng.uniform(0.45, 0.95))))
        if not offset_form and len(betas) >= 3:
            betas[int(rng.integers(len(betas)))].fill_(0.0)
            betas[int(rng.integers(len(betas)))].mul_(-1.0)
        for p in getattr(dec, "alpha_weights", {}).values():
            p.fill_(float(np.float32(rng.uniform(0.02, 0.2) if offset_form else rng.uniform(0.3, 1.7))))


def edge_tables(dec, family, T):
    """(beta_e [T, E], a_e [T, E] | None) of the decoder's CURRENT parameters, in CSR edge order"""
    g = dec.code.tanner_graph()
    rows = max(T, 1)
    if family == "basic":
        return np.full((rows, g.E), dec.factor, dtype=np.float32), None
    if family.startswith("edge"):
        return dec.weight_table()[:, :g.E], None
    layout = dec._sharing_layout()
    beta, alpha = dec.weight_tables()
    beta_e = beta[:, layout.beta_slot]
    if family == "n2d_oms":
        return beta_e, alpha[:, layout.alpha_edge_slot]
    return beta_e, None


def make(family, code, T, seed, schedule="layered"):
    """-> decoder with seeded, randomised weights (under ``schedule``)"""
    from ldpc_decoder import BasicMinSumDecoder
    from neural_2d_decoder import Neural2DMinSumDecoder, Neural2DOffsetMinSumDecoder
    from neural_minsum_decoder import NeuralMinSumDecoder, NeuralOffsetMinSumDecoder
    kw = {} if schedule is None else {"schedule": schedule}
    if family == "basic":
        return BasicMinSumDecoder(with_iterations(code, T), 0.7, **kw)
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    if family.startswith("n2d") and family != "n2d_oms":
        dec = Neural2DMinSumDecoder(code, int(family[3]), T, **kw)
    elif family == "n2d_oms":
        dec = Neural2DOffsetMinSumDecoder(code, 2, T, **kw)
    elif family == "edge_nms":
        dec = NeuralMinSumDecoder(code, T, **kw)
    else:
        dec = NeuralOffsetMinSumDecoder(code, T, **kw)
    randomise(dec, rng, form_of(family) == ref.OMS)
    return dec


# ---- input sets: name -> (code, family, T, seed, [(frames, snr_db), ...]).  Row 0 starts with three exact zeros and row 1 is
# rounded to integers (ties).  The SNR mixes are tuned so that the restatement decodes 20-80 % of each set (host test).
INPUT_SETS = {
    "toy": ("toy", "n2d2", 10, 1, [(30, -9.0), (10, 3.0)]),
    "small": ("small_96_48", "basic", 10, 2, [(67, 1.5)]),
    "small_oms": ("small_96_48", "n2d_oms", 10, 3, [(67, 1.5)]),
    "ira": ("ira_1998_1512", "basic", 10, 4, [(64, 4.0), (64, 5.0)]),
    "dvbs2": ("dvbs2_like_16200_7200", "basic", 3, 5, [(4, 0.0), (4, 5.0)]),
    "wide": ("wide", "basic", 6, 6, [(35, 3.0), (35, 9.0)]),
}
for _lw in LANE_WIDTHS:
    INPUT_SETS[f"lw{_lw}"] = (f"lw{_lw}", "n2d_oms" if _lw in (4, 32) else "n2d1", 10, 20 + _lw, [(12, -2.0), (11, 6.0)])


@functools.lru_cache(maxsize=None)
def input_llr(name):
    code_name, _, _, seed, mix = INPUT_SETS[name]
    code = load(code_name)
    rng = np.random.default_rng(1000 + seed)
    llr = np.concatenate([awgn(rng, b, code.n, snr) for b, snr in mix])
    llr = llr[rng.permutation(llr.shape[0])]
    llr[0, :3] = 0.0
    llr[1] = np.round(llr[1])
    llr.setflags(write=False)
    return llr


_REFERENCE = {}


def reference(name, family=None, T=None, early_stop=True, max_iters=None, rows=None, seed=None):
    """the restatement's result for an input set (default: under the set's own family and T), computed once per argument
    tuple and shared between the tests; the arrays are read-only.  -> (bits, P, iterations, success, R)"""
    code_name, fam0, T0, seed0, _ = INPUT_SETS[name]
    family, T, seed = family or fam0, T0 if T is None else T, seed0 if seed is None else seed
    key = (name, family, T, early_stop, max_iters, rows, seed)
    if key not in _REFERENCE:
        code = load(code_name)
        dec = make(family, code, T, seed)
        beta_e, a_e = edge_tables(dec, family, T)
        llr = input_llr(name) if rows is None else input_llr(name)[:rows]
        out = ref.restate(code.tanner_graph(), llr, T, form_of(family), beta_e, a_e, early_stop, max_iters)
        for a in out:
            a.setflags(write=False)
        _REFERENCE[key] = out
    return _REFERENCE[key]
