"""
Codes, families, batches and pointer placements shared by tests/test_row_alignment_host.py (CPU: the oracle and the case
list alone) and tests/test_gpu_row_alignment.py (GPU): a streaming decode changes layout at both ends, and the kernels that
do it are picked from the row length and from the address of each caller pointer (csrc/ldpc_hip.hip, boundary_kernels).
Three row lengths give the three residues of 4n mod 16; a placement puts llr, posterior and bits each at its own byte
offset behind a 256-byte-aligned guard.  Not a test module: nothing here needs a GPU.

Families, weights, inputs (`llrs`: a permuted half low / half high SNR mix, row 3 a strongly sent codeword) and expected
outputs are those of tests/dirty_state_cases.py, on the codes registered here.
"""
import functools
from collections import namedtuple

import numpy as np

import dirty_state_cases as ds
from dirty_state_cases import F32, F64, Case, awgn, expected, oracle_capped, seed_of   # noqa: F401  (what the tests use)

T = 10


def generated_code(n, m):
    """column weight 3, check degrees within one of each other: every column's three ones go to the currently least
    loaded checks, ties broken at random (seeded by n) -- so dv = 3 <= 8 and dc <= 32, and the pair, gather and
    fused-entrance forms and the LDS-resident engine all take the code"""
    from ldpc_decoder import LDPCCode
    rng = np.random.default_rng(n)
    H = np.zeros((m, n), dtype=np.int64)
    load = np.zeros(m, dtype=np.int64)
    for j in range(n):
        pick = np.lexsort((rng.random(m), load))[:3]
        H[pick, j] = 1
        load[pick] += 1
    return LDPCCode(n=n, k=n - m, H=H, max_iterations=T)


# 4n mod 16 == 0 (the shipped 96 x 48 code) | == 8 | n odd: two full 64-variable chunks and a ragged one of three
# variables; with fp64 its rows are 8-byte.  (low, high) SNR chosen on the CPU from the oracle's counts alone
# (tests/test_row_alignment_host.py holds the conditions).  The shipped code has a name of its own here: at the (0, 6) dB
# of dirty_state_cases' "small" the stopped rows of a layered batch of 65 show two stop iterations only
ds.register_code("small96", "small_96_48", T, (0.0, 4.0))
ds.register_code("g134", functools.partial(generated_code, 134, 66), T, (0.0, 4.0))
ds.register_code("g131", functools.partial(generated_code, 131, 64), T, (0.0, 4.0))
CODES = ("small96", "g134", "g131")
ODD = "g131"
assert all(ds.T_OF[c] == T for c in CODES)

# all on the streaming engine; the two layered ones run VEC = 1 at every batch, layout pass at both ends
FAMILIES = ("basic32", "n2d2", "offset2", "rcq-sweeps", "rcq-gather", "rcq-pair", "wrcq-q4", "basic64", "lay-nms", "lay-paper")
PAIR_Q4 = ("rcq-pair", "wrcq-q4")            # code-pair form: the fused entrance pass on 16-byte rows at VEC = 4
BATCHES = {F32: (1, 64, 65, 257), F64: (1, 64, 129)}
STOPS = ds.STOPS                             # early stop | fixed T | early stop capped at ds.CAP
FAMILY_CODES = [(f, c) for f in FAMILIES for c in CODES]


def dtype_of(family):
    return ds.FAMILIES[family].dtype


def layered(family):
    return ds.FAMILIES[family].kind.startswith("lay")


def cases(family, code):
    return [Case(family, code, B) for B in BATCHES[dtype_of(family)]]


# ---- placements ----------------------------------------------------------------------------------------------------------
# byte offsets of llr, posterior and bits behind the guard of their buffers; None: that output pointer is NULL
Placement = namedtuple("Placement", "name llr posterior bits")
PLACEMENTS = {
    F32: [Placement("aligned", 0, 0, 0)]
    + [Placement(f"llr+{k}", k, 0, 0) for k in (4, 8, 12)]
    + [Placement(f"out+{k}", 0, k, k) for k in (4, 8, 12)]
    + [Placement("bits+4", 0, 0, 4), Placement("post+4", 0, 4, 0), Placement("post+8,bits+4", 0, 8, 4),
       Placement("llr+4,post+12,bits+8", 4, 12, 8), Placement("post-null,bits+4", 0, None, 4),
       Placement("bits-null,post+4", 0, 4, None), Placement("both-null", 0, None, None)],
    F64: [Placement("aligned", 0, 0, 0)] + [Placement(f"llr+8,post+8,bits+{k}", 8, 8, k) for k in (4, 8, 12)],
}
MAX_OFFSET = 16


def placements(family):
    return PLACEMENTS[dtype_of(family)]


# ---- what a placement is built for: the boundary kernels, restated -----------------------------------------------------------
Kernels = namedtuple("Kernels", "vec in_bytes fused_in out_path out_bytes")


def width(elem, n, *offsets):
    """the widest of 16 / 8 / 4 bytes, not below one element, that divides the row length in bytes and every offset"""
    for vb in (16, 8, 4):
        if vb >= elem and (n * elem) % vb == 0 and all(o % vb == 0 for o in offsets):
            return vb
    return 0


def kernels(family, n, B, pl, saving=False):
    """what a decode of B rows of length n at placement pl launches at its two ends"""
    f64, lay = dtype_of(family) is F64, layered(family)
    elem = 8 if f64 else 4
    vec = 1 if lay or B <= 64 else 2 if f64 else 4
    rows4 = vec == 4 and not saving                    # fp32 flooding, 256-codeword tiles, not the training forward
    win = width(elem, n, pl.llr)
    if pl.posterior is None and pl.bits is None:
        path, wout = "none", 0
    else:
        wout = width(elem, n, pl.posterior or 0, pl.bits or 0)
        path = "last-rows" if rows4 and wout >= 4 else "layout"
    return Kernels(vec, win, rows4 and family in PAIR_Q4 and win == 16, path, wout)


def reachable(family):
    """-> (set of (vec, in_bytes), set of (vec, out_path, out_bytes)) a decode of the family can take through ldpc_decode"""
    if dtype_of(family) is F64:
        return ({(v, w) for v in (1, 2) for w in (16, 8)},
                {(v, "layout", w) for v in (1, 2) for w in (16, 8, 0)})
    if layered(family):
        return {(1, w) for w in (16, 8, 4)}, {(1, "layout", w) for w in (16, 8, 4)} | {(1, "none", 0)}
    return ({(v, w) for v in (1, 4) for w in (16, 8, 4)},
            {(1, "layout", w) for w in (16, 8, 4)} | {(4, "last-rows", w) for w in (16, 8, 4)} | {(1, "none", 0), (4, "none", 0)})


def tile_rows(family, B):
    return 64 if layered(family) or B <= 64 else 128 if dtype_of(family) is F64 else 256
