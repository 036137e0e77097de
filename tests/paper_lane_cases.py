"""
Cases shared by tests/test_paper_lanes_host.py (CPU) and tests/test_gpu_paper_lanes.py (GPU): the paper-schedule layered RCQ
decoders -- RCQMinSumDecoder(layered="paper") and WeightedRCQDecoder(layered="paper") -- on the LDS-resident kernel
layered_paper_lds<LW, NL, ES, WB> (csrc/ldpc_layered.hip) at the shapes no other test reaches:

  lane    lw1 .. lw64: layered_minsum_cases.lane_width_code(lw) -- the widest check fills the row, one degree-1 and one
          degree-0 check, odd m and odd n; bc = 3 (the compile-time four-level quantiser)
  quant   lw8 and lw64 under bc = 3 (NL = 4), bc = 4 (eight levels: the p4..p7 / c4..c7 select trees), bc = 5 (sixteen
          levels: the global-table branch) and a quantiser whose level 0 is not zero (gamma = 0)
  geom    random graphs of a given (n, m, max check degree) that put the host's codewords-per-wave search
          (build_layered_plan, csrc/ldpc_hip.hip) in each of its outcomes: a full wave, a count that is no power of two, one
          codeword with shadow lane groups, and the refusal (fewer than four workgroups per CU: the streaming kernel)

Every case has a plain and a weighted decoder (sharing type 1, ``randomise_betas``: zeros and negatives), T = 6.

Inputs: a pool of POOL rows per case, the all-zero codeword over AWGN at two SNRs assigned by ``row % 2`` -- neighbouring
lane groups of a wave then hold a fast and a slow codeword; row 0 starts with three exact zeros, row 1 is rounded (ties),
row 2 is |llr| + 4 (it stops at once).  Rows decode independently, so a batch is a prefix of the pool and the references are
computed once on the whole pool.  The SNR pairs were chosen on the CPU from the references alone until ``degeneracy`` below
finds nothing (tests/test_paper_lanes_host.py asserts it).  Not a test module: nothing here needs a GPU.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import layered_minsum_cases as lmc
from test_gpu_layered_weighted import QP, edge_betas, randomise_betas, restate

T = 6
POOL = 70
QP_GAMMA0 = [(1.5, 0.0), (3.0, 1.3), (2.0, 0.0)]               # tests/test_gpu_parity.py "gamma0": every level of quantisers 0 and 2 is C

# ---- the host rule restated (build_layered_plan, LDPC_SCHED_LAYERED with the RCQ form) ----------------------------------
LDS_BYTES = 160 * 1024
MIN_WORKGROUPS = 4                                              # kLayPaperMinWaves


def lane_width(max_dc):
    lw = 1
    while lw < max_dc:
        lw <<= 1
    return lw


def row_bytes(n, m, lw):
    """LDS bytes of one codeword: n posteriors and the +inf word, then one code byte per plan entry (m padded to 4 rows)"""
    m_pad = (m + 3) // 4 * 4
    return 4 * (n + 1) + (m_pad * lw + 3) // 4 * 4


def plan_of(n, m, lw):
    """-> (codewords per wave, workgroups per CU) the rule as written gives; cw = 0: the streaming kernel"""
    rb = row_bytes(n, m, lw)
    cw = 64 // lw
    while cw > 1 and cw * rb > LDS_BYTES:
        cw >>= 1
    if cw * rb > LDS_BYTES:
        return 0, 0
    best, best_cu = cw, 0
    for c in range(cw, 0, -1):
        per_cu = c * (LDS_BYTES // (c * rb))
        if per_cu > best_cu:
            best, best_cu = c, per_cu
    if LDS_BYTES // (best * rb) < MIN_WORKGROUPS:
        return 0, 0
    return best, LDS_BYTES // (best * rb)


FULL, NPOT, SINGLE, STREAM = "full wave", "not a power of two", "single codeword", "streaming kernel"


def class_of(cw, lw):
    """the class of a codewords-per-wave count beside 64 / lw lane groups (None: a partial power of two, no class of the table)"""
    if cw == 0:
        return STREAM
    if cw == 64 // lw:
        return FULL
    if cw & (cw - 1):
        return NPOT
    return SINGLE if cw == 1 else None


# ---- cases ------------------------------------------------------------------------------------------------------------------
# kind: "lane" / "quant" / "geom"; code: a layered_minsum_cases name or (n, m, max check degree); klass: geometry class or None;
# snr: (dB of the even rows, dB of the odd rows)
Case = namedtuple("Case", "name kind code lw bc qp klass seed snr")

# (n, m, max dc) -> class, as the table of the rule gives them (plan_of restates the rule; the host test checks the table)
GEOMETRY = [
    ((500, 250, 6), FULL),          # LW 8: 8 of 8
    ((100, 25, 12), FULL),          # LW 16: 4 of 4
    ((100, 25, 24), FULL),          # LW 32: 2 of 2
    ((1300, 325, 3), NPOT),         # LW 4: 5 of 16
    ((500, 250, 2), NPOT),          # LW 2: 13 of 32
    ((1100, 275, 1), NPOT),         # LW 1: 7 of 64
    ((300, 75, 12), SINGLE),        # LW 16: 1 of 4, three shadow groups
    ((1200, 600, 40), STREAM),      # LW 64: three workgroups per CU
]

# SNR pairs (even rows, odd rows) in dB, chosen on the CPU (module docstring)
SNR = {
    "lw1": (-6.0, 8.0), "lw2": (-5.0, -4.0), "lw4": (-4.0, 7.0), "lw8": (-1.0, 8.0), "lw16": (-1.0, 8.0),
    "lw32": (4.0, 9.0), "lw64": (7.0, 9.0),
    "lw8-bc3": (1.0, 8.0), "lw8-bc4": (-1.0, 8.0), "lw8-bc5": (-5.0, 8.0), "lw8-gamma0": (-4.0, 7.0),
    "lw64-bc3": (3.0, 9.0), "lw64-bc4": (2.0, 8.0), "lw64-bc5": (3.0, 9.0), "lw64-gamma0": (5.0, 9.0),
    "g500x250-dc6": (4.0, 10.0), "g100x25-dc12": (4.0, 9.0), "g100x25-dc24": (3.0, 10.0), "g1300x325-dc3": (7.0, 11.0),
    "g500x250-dc2": (6.0, 11.0), "g1100x275-dc1": (-6.0, 11.0), "g300x75-dc12": (5.0, 11.0), "g1200x600-dc40": (4.0, 13.0),
}


def _cases():
    out = []
    for lw in lmc.LANE_WIDTHS:
        out.append(("lw%d" % lw, "lane", "lw%d" % lw, lw, 3, QP, None))
    for lw in (8, 64):
        for tag, bc, qp in (("bc3", 3, QP), ("bc4", 4, QP), ("bc5", 5, QP), ("gamma0", 3, QP_GAMMA0)):
            out.append(("lw%d-%s" % (lw, tag), "quant", "lw%d" % lw, lw, bc, qp, None))
    for (n, m, dmax), klass in GEOMETRY:
        out.append(("g%dx%d-dc%d" % (n, m, dmax), "geom", (n, m, dmax), lane_width(dmax), 3, QP, klass))
    return [Case(*c, seed=4000 + 17 * i, snr=SNR[c[0]]) for i, c in enumerate(out)]


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def geometry_code(n, m, max_dc, seed):
    """random graph: every check degree in 1 .. max_dc, check 0 of a random order attains max_dc; n and m exact"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(seed)
    degs = rng.integers(1, max_dc + 1, size=m)
    degs[int(rng.integers(m))] = max_dc
    H = np.zeros((m, n), dtype=np.int64)
    for i in range(m):
        H[i, rng.choice(n, size=int(degs[i]), replace=False)] = 1
    return LDPCCode(n=n, k=n - m, H=H, max_iterations=T)


@functools.lru_cache(maxsize=None)
def code_of(name):
    c = BY_NAME[name]
    if c.kind == "geom":
        return geometry_code(*c.code, seed=c.seed)
    return lmc.with_iterations(lmc.load(c.code), T)


def n_levels(c):
    return 2 ** (c.bc - 1)


@functools.lru_cache(maxsize=None)
def decoders(name):
    """-> (plain decoder, weighted decoder with seeded betas, its per-edge beta table [T, E])"""
    from rcq_decoder import RCQMinSumDecoder, WeightedRCQDecoder
    c, code = BY_NAME[name], code_of(name)
    plain = RCQMinSumDecoder(code, c.bc, 8, c.qp, max_iterations=T, layered="paper")
    torch.manual_seed(c.seed)                                   # the init draws that randomise_betas perturbs
    weighted = WeightedRCQDecoder(code, c.bc, 8, c.qp, weight_sharing_type=1, max_iterations=T, layered="paper")
    randomise_betas(weighted, np.random.default_rng(c.seed + 1))
    beta_e = edge_betas(weighted, T)
    beta_e.setflags(write=False)
    return plain, weighted, beta_e


def pool_llr(c, snr=None):
    """the POOL rows of a case (``snr``: another pair than the case's own, for choosing one)"""
    n = code_of(c.name).n
    z = np.random.default_rng(c.seed + 2).standard_normal((POOL, n))
    s2 = (10.0 ** (-np.asarray(snr or c.snr, dtype=np.float64) / 10.0))[np.arange(POOL) % 2][:, None]
    llr = (2.0 * (1.0 + np.sqrt(s2) * z) / s2).astype(np.float32)
    llr[0, :3] = 0.0
    llr[1] = np.round(llr[1])
    llr[2] = np.abs(llr[2]) + np.float32(4.0)
    return llr


@functools.lru_cache(maxsize=None)
def inputs(name):
    llr = pool_llr(BY_NAME[name])
    llr.setflags(write=False)
    return llr


def oracle_graph(oracle_mod, name):
    g = code_of(name).tanner_graph()
    return oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)


_REF = {}


def reference(oracle_mod, name, weighted, early_stop=True):
    """(bits, posterior, iterations, success) of the whole pool, computed once and read-only.  Weighted: the restatement of
    tests/test_gpu_layered_weighted.py under the decoder's betas.  Plain, early stop: oracle.rcq_layered(paper=True).  Plain,
    fixed T (the oracle has no such mode): the restatement at unit beta, which the host test shows equal to the oracle under
    early stop on every case."""
    key = (name, bool(weighted), bool(early_stop))
    if key not in _REF:
        c, code = BY_NAME[name], code_of(name)
        if weighted or not early_stop:
            beta_e = decoders(name)[2] if weighted else np.ones((T, code.tanner_graph().E), dtype=np.float32)
            out = restate(code, inputs(name), c.bc, c.qp, T, beta_e, early_stop=early_stop)
        else:
            out = oracle_mod.rcq_layered(oracle_graph(oracle_mod, name), inputs(name), c.bc, c.qp, T, paper=True)
        for a in out:
            a.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def static_decode(name):
    """every check has at most one edge (LW = 1).  A degree-1 check sends beta * |u| quantised, and Q rounds magnitudes down:
    with |beta| <= 1 (``randomise_betas`` draws |beta| < 0.8) |message| <= |u| and P = u + message keeps the sign of u, which
    is the LLR plus the variable's other such messages.  No hard decision ever changes: a codeword stops after iteration 1
    or never, whatever the channel, so "two distinct stop iterations" cannot be asked of these codes"""
    return code_of(name).tanner_graph().dc.max() <= 1


def degeneracy(name, iters, succ, cw=None):
    """what makes the early-stop reference of a case a weak test -> list of complaints (empty: none).
    Every case: a row stops before T, a row does not stop, two distinct stop iterations occur (not asked where no decode can
    give them, see ``static_decode``).  cw > 1: an aligned group of cw consecutive rows of the largest batch,
    min(3 cw - 1, POOL) rows, holds a stopped row and an open one."""
    out = []
    if not (succ & (iters < T)).any():
        out.append("no row stops before T")
    if succ.all():
        out.append("every row stops")
    if np.unique(iters[succ]).size < 2 and not static_decode(name):
        out.append("one stop iteration only: %s" % np.unique(iters[succ]))
    if cw is not None and cw > 1:
        B = min(3 * cw - 1, POOL)
        s = succ[:B]
        if not any(s[a:a + cw].any() and not s[a:a + cw].all() for a in range(0, B, cw)):
            out.append("no wave of %d rows holds a stopped and an open row" % cw)
    return out


def batches(cw):
    """rows of the decodes of a case on a kernel that takes `cw` codewords per workgroup: one row, one more than a wave, one
    short of three waves, and the whole pool -- at one or two codewords per wave the first three are rows 0 and 1 alone, and what
    ``degeneracy`` establishes is a property of the pool"""
    return sorted({1, min(cw + 1, POOL), min(max(3 * cw - 1, 1), POOL), POOL})
