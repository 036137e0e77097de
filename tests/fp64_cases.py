"""
Codes, weight tables, inputs and expectations shared by tests/test_fp64_cases_host.py (CPU: the oracle and the case list
alone), tests/test_gpu_fp64_weighted.py and tests/test_gpu_sum_order.py (GPU).  Not a test module: nothing here needs a GPU.

Part A -- the fp64 engine with weight tables.  ``ldpc_decoder_create`` takes LDPC_F64 with any NMS / OMS descriptor; the
decoder classes only ever hand it beta = 0.7 in one slot and alpha = 1.  The cases here fill every sharing type's tables with
seeded float64 draws (NOT float32 values widened: an operand narrowed to float anywhere then changes the result) and decode a
permuted half low / half high SNR mix of which the host test establishes that the oracle decodes some rows and not others.

Part B -- the association order of the variable sums.  Two generated graphs hold one variable of every degree at which
``sum_rt`` / ``sum_ct`` (csrc/ldpc_kernels.hip) change block: N = dv for the posterior, N = dv - 1 for the leave-one-out sums,
numpy order (8 accumulators, remainder) on the fp64 graph and torch order (8 lanes, ILP-4 groups of 32, remainder) on the
fp32 graph, up to the degrees the engine admits (128 / 575).

Expectations come from ``oracle.decode`` (SUM_NUMPY for float64, SUM_TORCH for float32), computed once per process and
read-only.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np

import layered_minsum_cases as lm

F32, F64 = np.float32, np.float64


def seed_of(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


# =========================================================================================================================
# Part A
# =========================================================================================================================
B = 37
TILE_BATCHES = (1, 64, 65, 128, 129, 130)         # fp64 streaming layout: 64-codeword tiles up to 64, 128-codeword tiles above
# code -> (shipped name or builder, T, (low, high) SNR in dB).  The SNR pairs were picked on the CPU from the oracle's counts
# alone (tests/test_fp64_cases_host.py holds the conditions): with random weights (1998,1512) needs T = 10 to decode at all
CODES = {"small": ("small_96_48", 6, (1.0, 5.0)),
         "ira": ("ira_1998_1512", 10, (3.0, 5.75)),
         "wide": (lm.wide_check_code, 6, (4.0, 8.0))}

# form: "nms" | "oms" (seeded tables of sharing type wtype) | "basic" (beta = 0.7 in one slot, alpha = 1: what
# BasicMinSumDecoder builds).  resident: the planner takes fp64 NMS with one beta per check only, so types 2-4 and Basic
# may run LDS-resident and type 1 / OMS must not
Case = namedtuple("Case", "form wtype code")
PLAIN = ("small", "ira")
NMS_RESIDENT = [Case("nms", w, c) for w in (2, 3, 4) for c in PLAIN]
NMS_STREAM_ONLY = [Case("nms", 1, c) for c in PLAIN]
OMS = [Case("oms", w, c) for w in (2, 1) for c in PLAIN]
WIDE = Case("nms", 2, "wide")
BASIC = [Case("basic", 0, c) for c in PLAIN]
WEIGHTED = NMS_RESIDENT + NMS_STREAM_ONLY + OMS + [WIDE]
DECODE_CASES = WEIGHTED + BASIC
TILE_CASES = [Case("nms", 2, "small"), Case("oms", 2, "small")]
CAP_CASE = Case("nms", 2, "ira")
SET_WEIGHTS_CASES = [Case("nms", 2, "ira"), Case("oms", 2, "ira")]


def case_id(c):
    return f"{c.form}{c.wtype or ''}-{c.code}"


def T_of(code_name):
    return CODES[code_name][1]


def caps(case):
    T = T_of(case.code)
    return (1, 2, T - 1)


@functools.lru_cache(maxsize=None)
def load_code(name):
    import codes
    src, T, _ = CODES[name]
    return src() if callable(src) else codes.load_code(src, T)


_graphs = {}


def oracle_graph(oracle_mod, tanner):
    """the oracle's own graph object of a TannerGraph (one per graph and process)"""
    if id(tanner) not in _graphs:
        _graphs[id(tanner)] = (tanner, oracle_mod.OracleGraph(n=tanner.n, check_ptr=tanner.check_ptr, var_idx=tanner.var_idx))
    return _graphs[id(tanner)][1]


# beta, alpha [T, slots] float64 and their int32 slot arrays; oms_alpha / oms_alpha_slot None for the normalised form
Tables = namedtuple("Tables", "beta beta_slot alpha alpha_slot oms_alpha oms_alpha_slot")
RANGES = {"nms": ((0.5, 1.0), (0.8, 1.2)), "oms": ((0.0, 0.6), (0.8, 1.2))}     # (beta, alpha); oms_alpha in [0, 0.3]


def draw_tables(oracle_mod, og, form, wtype, T, seed):
    """seeded float64 tables on the slot arrays of sharing type `wtype` (oracle.weight_tables; None: one beta and one alpha
    slot); the offset form's check-side alpha sits on the beta slots"""
    if wtype is None:                                          # one beta and one alpha slot
        bt, bs, at, as_ = np.zeros((T, 1)), np.zeros(og.E, np.int32), np.zeros((T, 1)), np.zeros(og.n, np.int32)
    else:
        bt, bs, at, as_ = oracle_mod.weight_tables(og, wtype, T, {}, {}, dtype=np.float64)
    rng = np.random.default_rng(seed)
    (blo, bhi), (alo, ahi) = RANGES[form]
    beta, alpha = rng.uniform(blo, bhi, bt.shape), rng.uniform(alo, ahi, at.shape)
    oa, oas = (rng.uniform(0.0, 0.3, bt.shape), bs.copy()) if form == "oms" else (None, None)
    return Tables(*frozen(beta, bs, alpha, as_, oa, oas))


_tables = {}


def tables(oracle_mod, case, variant=0):
    """the case's tables; variant > 0: another seeded draw on the same slots (what a weight update uploads)"""
    key = (case, variant)
    if key not in _tables:
        og, T = oracle_graph(oracle_mod, load_code(case.code).tanner_graph()), T_of(case.code)
        if case.form == "basic":
            _tables[key] = Tables(*frozen(np.full((T, 1), 0.7), np.zeros(og.E, np.int32), np.ones((T, 1)),
                                          np.zeros(og.n, np.int32), None, None))
        else:
            _tables[key] = draw_tables(oracle_mod, og, case.form, case.wtype, T, seed_of("tables", *case, variant))
    return _tables[key]


def unit_alpha(t):
    return t._replace(alpha=frozen(np.ones_like(t.alpha))[0])


def awgn(rng, rows, n, snr_db):
    s2 = 10.0 ** (-snr_db / 10.0)
    return 2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((rows, n))) / s2


@functools.lru_cache(maxsize=None)
def llrs(code_name, batch=B):
    """float64 [batch, n]: the first batch - batch/2 rows at the code's low SNR, the others at its high one, permuted"""
    n, (lo, hi) = load_code(code_name).n, CODES[code_name][2]
    rng = np.random.default_rng(seed_of("llr", code_name, batch))
    x = np.concatenate([awgn(rng, batch - batch // 2, n, lo), awgn(rng, batch // 2, n, hi)])[rng.permutation(batch)]
    return frozen(np.ascontiguousarray(x))[0]


def oracle_decode(oracle_mod, og, llr, form, t, T, early_stop=True, sum_order=None):
    """``oracle.decode`` of llr (its dtype is the arithmetic) under tables `t`; T below the tables' rows is a capped decode"""
    o = oracle_mod
    if sum_order is None:
        sum_order = o.SUM_NUMPY if llr.dtype == np.float64 else o.SUM_TORCH
    kw = dict(oms_alpha=t.oms_alpha, oms_alpha_slot=t.oms_alpha_slot) if form == "oms" else {}
    return o.decode(og, llr, T=T, early_stop=early_stop, c2v_form=o.C2V_OMS if form == "oms" else o.C2V_NMS,
                    sum_order=sum_order, beta=t.beta, beta_slot=t.beta_slot, alpha=t.alpha, alpha_slot=t.alpha_slot, **kw)


Expected = namedtuple("Expected", "bits posterior iterations success")
_expected = {}


def expected(oracle_mod, case, early_stop=True, cap=None, batch=B, variant=0, unit=False):
    """what a decode of the case must return, the same for every engine form.  cap: the oracle run for `cap` iterations with
    the T-row tables (ldpc_decode_capped); variant / unit: under the tables a weight update put in force"""
    key = (case, early_stop, cap, batch, variant, unit)
    if key not in _expected:
        og = oracle_graph(oracle_mod, load_code(case.code).tanner_graph())
        t = tables(oracle_mod, case, variant)
        out = oracle_decode(oracle_mod, og, llrs(case.code, batch), case.form, unit_alpha(t) if unit else t,
                            cap or T_of(case.code), early_stop)
        _expected[key] = Expected(*frozen(*out))
    return _expected[key]


# =========================================================================================================================
# Part B
# =========================================================================================================================
FILLER = 40
# name -> (dtype, rows m, seed, the degrees that get one variable each).  N = dv - 1 and N = dv fall on both sides of every
# block edge: numpy 8 / 16 / 24 / 32 / 64 / 128 and the remainder, torch 8 lanes, 32 / 64 / 256 / 512 and both remainders
SUM_GRAPHS = {
    "f64": (F64, 128, 3, (1, 2, 7, 8, 9, 10, 15, 16, 17, 18, 24, 25, 32, 33, 64, 65, 120, 127, 128)),
    "f32": (F32, 575, 3, (7, 8, 9, 12, 13, 31, 32, 33, 39, 40, 41, 63, 64, 65, 255, 256, 257, 511, 512, 574, 575)),
}
SUM_DECODERS = {"f64": ("nms1", "nms2", "oms2"), "f32": ("nms1", "nms2")}      # form + sharing type of the slot arrays
SUM_BATCH = 16
SUM_WIDE_BATCH = {"f64": 130, "f32": 300}         # 128- and 256-codeword tiles: sum_rt at VEC = 2 and VEC = 4
SUM_T = (1, 3)


def degree_graph(m, degrees, seed, filler=FILLER):
    """dense H [m, len(degrees) + filler]: column k has exactly degrees[k] ones, the filler columns three, every column's
    checks drawn without replacement"""
    rng = np.random.default_rng(seed)
    H = np.zeros((m, len(degrees) + filler), dtype=np.int64)
    for j, d in enumerate(list(degrees) + [3] * filler):
        H[rng.choice(m, size=d, replace=False), j] = 1
    return H


@functools.lru_cache(maxsize=None)
def sum_graph(name):
    """the TannerGraph of a sum-order graph (one object per process: the engines share its device copy)"""
    from tanner_graph import TannerGraph
    _, m, seed, degrees = SUM_GRAPHS[name]
    return TannerGraph.from_dense(degree_graph(m, degrees, seed))


@functools.lru_cache(maxsize=None)
def refused_graph(degree):
    """one variable on all of `degree` checks beside eight filler variables: a graph only its largest degree can get refused"""
    from tanner_graph import TannerGraph
    return TannerGraph.from_dense(degree_graph(degree, (degree,), 7, filler=8))


def sum_tables(oracle_mod, name, decoder, T):
    og = oracle_graph(oracle_mod, sum_graph(name))
    key = ("sum", name, decoder, T)
    if key not in _tables:
        _tables[key] = draw_tables(oracle_mod, og, decoder[:3], None if decoder[3] == "1" else 2, T, seed_of(*key))
    return _tables[key]


@functools.lru_cache(maxsize=None)
def sum_llrs(name, batch=SUM_BATCH):
    dtype, m, seed, degrees = SUM_GRAPHS[name]
    rng = np.random.default_rng(seed_of("sum-llr", name, batch))
    x = (2.5 * rng.standard_normal((batch, len(degrees) + FILLER)) + 1.0).astype(dtype)
    return frozen(np.ascontiguousarray(x))[0]


def sum_expected(oracle_mod, name, decoder, T, batch=SUM_BATCH, sum_order=None):
    """fixed-T decode of the graph's inputs by the oracle in the graph's arithmetic (sum_order: the other order, host test)"""
    key = ("sum", name, decoder, T, batch, sum_order)
    if key not in _expected:
        og = oracle_graph(oracle_mod, sum_graph(name))
        out = oracle_decode(oracle_mod, og, sum_llrs(name, batch), decoder[:3], sum_tables(oracle_mod, name, decoder, T), T,
                            early_stop=False, sum_order=sum_order)
        _expected[key] = Expected(*frozen(*out))
    return _expected[key]


def differing_degrees(name, got, want):
    """sorted degrees of the variables at which two posteriors [B, n] differ as values"""
    dv = sum_graph(name).dv
    return sorted({int(d) for d in dv[np.flatnonzero((np.asarray(got) != np.asarray(want)).any(axis=0))]})
